"""
The text key dictionary in front of GpuPreAgg (strom_textdict_*), the parts that need no GPU:
the C ABI, the fixed device program for gfx950, the refusals made before a device is looked at,
and the pin that motivates the operator -- GpuPreAgg's own code generator still refuses a text key.
"""
import ctypes
import os
import re

import pytest

from pg_strom_amd import runtime, textdict
from pg_strom_amd._lib import lib, PROTOTYPES
from pg_strom_amd.gpupreagg import codegen_gpupreagg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_REQUEST = 101


def test_symbols_resolve_and_have_prototypes():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    declared = set(re.findall(r"\b(strom_textdict_\w+)\s*\(", header))
    assert declared == {"strom_textdict_create", "strom_textdict_num_keys", "strom_textdict_encode",
                        "strom_textdict_fetch", "strom_textdict_kernel_ns", "strom_textdict_program",
                        "strom_textdict_reset",
                        "strom_textdict_release"}
    for name in declared:
        assert name in PROTOTYPES, name
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("hash_bits", [None, 4])
def test_fixed_program_compiles_for_gfx950(hash_bits):
    src = textdict.program_source(block=None, hash_bits=hash_bits)
    assert '#include "strom_textdict.h"' in src
    prog = runtime.DevProgram(src, 0).wait()
    assert prog.state() == 1
    prog.release()


def test_refusals_that_need_no_device():
    err = ctypes.c_int(0)
    # neither text nor character(n)
    for oid in (23, 1042, 17, 0):
        assert not lib.strom_textdict_create(oid, 0, 0, ctypes.byref(err))
        assert err.value == BAD_REQUEST
    # without a resident chunk there is nothing to encode, whatever else is passed (a chunk handle
    # needs a device: the refusals of a NULL dictionary, of key counts outside 1..8 and of the
    # wrong kinds of column are in tests/test_textdict_gpu.py)
    one = (ctypes.c_void_p * 1)(None)
    col = (ctypes.c_int32 * 1)(0)
    for dicts in (one, None):
        err.value = 0
        assert not lib.strom_textdict_encode(dicts, col, 1, None, None, 0, ctypes.byref(err))
        assert err.value == BAD_REQUEST
    assert lib.strom_textdict_num_keys(None) == 0
    assert lib.strom_textdict_fetch(None, None, 0, None, 0, None) == -BAD_REQUEST
    assert lib.strom_textdict_kernel_ns(None, None) == BAD_REQUEST
    assert lib.strom_textdict_program(None) == 0
    lib.strom_textdict_reset(None)
    lib.strom_textdict_release(None)


def test_gpupreagg_codegen_still_refuses_a_text_key():
    """the dictionary exists BECAUSE the emitter keeps to fixed-width key images"""
    with pytest.raises(ValueError):
        codegen_gpupreagg("(gpupreagg (key (var 1 text)) (nrows))")
    with pytest.raises(ValueError):
        codegen_gpupreagg("(gpupreagg (key (var 1 character)) (nrows))")
    # ... and takes the ids the dictionary makes of such a column
    assert codegen_gpupreagg("(gpupreagg (key (var 1 int4)) (nrows))").targets[0][1] == 23
