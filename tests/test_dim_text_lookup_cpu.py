"""
A dimension's text column as a coded column (strom_textdict_encode_table), the parts that need no GPU: the
symbol, the dictionary's fixed program with the textdict_table_* kernels compiled for gfx950 as the
runtime compiles it (no scratch, no LDS), the patch kernel in a join program, and the register figures
of the two walks that were there before -- textdict_probe and keyunion_probe keep what
profiles/textdict_resources.txt said before the third walk was written out next to them.
"""
import ast
import ctypes
import importlib.util
import os
import re

from pg_strom_amd import runtime, textdict
from pg_strom_amd._lib import lib, PROTOTYPES
from pg_strom_amd.gpuhashjoin import codegen_gpuhashjoin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_REQUEST = 101
TABLE_KERNELS = ("textdict_table_offsets", "textdict_table_probe", "textdict_table_settle", "textdict_table_emit")
# what the file said before the table kernels were added: (vgpr, agpr, sgpr, LDS bytes, scratch bytes)
BEFORE = {"textdict_probe": (40, 0, 98, 0, 0), "keyunion_probe": (44, 0, 89, 0, 0)}
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _resources_module():
    spec = importlib.util.spec_from_file_location(
        "_star_lookup_resources", os.path.join(ROOT, "scripts", "star_lookup_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _profile():
    """{kernel: (vgpr, agpr, sgpr, LDS, scratch)} of profiles/textdict_resources.txt"""
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "textdict_resources.txt")):
        m = re.match(r"(\w+) (\{.*\})\s*$", line)
        if m:
            vals = ast.literal_eval(m.group(2))
            out[m.group(1)] = tuple(int(vals[f]) for f in FIELDS)
    return out


def _compiled():
    """the default program's kernels, from the code object the runtime's compiler wrote"""
    prog = runtime.DevProgram(textdict.program_source(block=None, hash_bits=None), 0).wait()
    try:
        assert prog.state() == 1
        path = os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)
        return {k: tuple(v[f] for f in FIELDS) for k, v in _resources_module().kernel_resources(path).items()}
    finally:
        prog.release()


def test_symbol_is_exported_declared_and_refuses_null_handles():
    assert "strom_textdict_encode_table" in PROTOTYPES
    assert getattr(lib, "strom_textdict_encode_table") is not None
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    own = open(os.path.join(ROOT, "include", "strom_textdict_table.h")).read()
    assert '#include "strom_textdict_table.h"' in header
    assert re.search(r"\bint\s+strom_textdict_encode_table\s*\(\s*strom_textdict \*dict, strom_hashjoin_table \*tbl, int colidx\)", own)
    assert lib.strom_textdict_encode_table(None, None, 0) == -BAD_REQUEST
    assert hasattr(textdict.TextDictionary, "encode_table") and hasattr(textdict, "group_by_dimension_text")


def test_table_kernels_compile_for_gfx950_without_scratch_or_lds(monkeypatch):
    monkeypatch.delenv("STROM_TEXTDICT_BLOCK", raising=False)
    monkeypatch.delenv("STROM_TEXTDICT_HASH_BITS", raising=False)
    res = _compiled()
    for k in TABLE_KERNELS:
        assert k in res, k
        print(k, res[k])
        assert res[k][3] == 0 and res[k][4] == 0, (k, res[k])      # less than keyunion_count's 48 bytes of LDS: none
    # the program the tests build with 4 hash bits and 64 lanes compiles as well
    prog = runtime.DevProgram(textdict.program_source(block=64, hash_bits=4), 0).wait()
    assert prog.state() == 1
    prog.release()


def test_the_walks_that_were_there_keep_their_figures(monkeypatch):
    monkeypatch.delenv("STROM_TEXTDICT_BLOCK", raising=False)
    monkeypatch.delenv("STROM_TEXTDICT_HASH_BITS", raising=False)
    prof = _profile()
    for k, want in BEFORE.items():
        assert prof[k] == want, (k, prof[k])
    for k in TABLE_KERNELS:
        assert prof[k][3] == 0 and prof[k][4] == 0, (k, prof[k])
    # ... and the file is what the compiler gives for this tree
    assert prof == _compiled()


def test_patch_kernel_is_in_a_join_program_and_uses_no_scratch():
    cg = codegen_gpuhashjoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))")
    cg = cg[0] if isinstance(cg, tuple) else cg
    prog = runtime.DevProgram(cg.source, cg.extra_flags).wait()
    try:
        path = os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)
        r = _resources_module().kernel_resources(path)["hashjoin_patch_dimrec_kernel"]
        print(r)
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, r
    finally:
        prog.release()


class TableArgs(ctypes.Structure):
    """textdict_table_args of strom_ctl.h, field by field"""
    _fields_ = [("kmhash", ctypes.c_uint64), ("hjidx", ctypes.c_uint64), ("datum_off", ctypes.c_uint64),
                ("out_ids", ctypes.c_uint64), ("out_isnull", ctypes.c_uint64), ("tbl_nslots", ctypes.c_uint32),
                ("colidx", ctypes.c_int32)]


def test_control_block_matches_its_static_assert():
    text = open(os.path.join(ROOT, "pg_strom_amd", "csrc", "devlib", "strom_ctl.h")).read()
    m = re.search(r"static_assert\(sizeof\(textdict_table_args\) == (\d+),", text)
    assert m and int(m.group(1)) == ctypes.sizeof(TableArgs)
    body = re.search(r"struct textdict_table_args \{(.*?)\n\};", text, re.S).group(1)
    assert re.findall(r"\bcl_u?(?:int|long)\s+(\w+);", body) == [n for n, _ in TableArgs._fields_]
    # the blocks that were there keep their sizes
    for name, size in (("textdict_args", 104), ("textdict_ctl", 32), ("hashjoin_dimrec_spec", 264)):
        assert re.search(r"static_assert\(sizeof\(%s\) == %d," % (name, size), text), name
