"""
The union of key dictionaries (strom_keyunion_*, strom_keymap_*), the parts that need no GPU: the
C ABI, the refusals made before a device is looked at, the new kernels in the dictionary's fixed
program for gfx950, and the one thing real ranks add -- the all-gather of the key images -- over
gloo.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from pg_strom_amd import runtime, textdict
from pg_strom_amd._lib import lib, PROTOTYPES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAD_REQUEST = 101
NAMES = {"strom_keyunion_absorb", "strom_keyunion_absorb_dict", "strom_keyunion_recode",
         "strom_keyunion_kernel_ns", "strom_keymap_size", "strom_keymap_fetch", "strom_keymap_release"}
KERNELS = ["keyunion_probe", "keyunion_count", "keyunion_offsets", "keyunion_settle", "keyunion_emit",
           "keyunion_recode"]


def test_symbols_are_declared_resolve_and_have_prototypes():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(strom_key(?:union|map)_\w+)\s*\(", header))
    assert declared == NAMES
    assert "typedef struct strom_keymap strom_keymap;" in header
    for name in NAMES:
        assert name in PROTOTYPES, name
        assert getattr(lib, name) is not None


def test_refusals_that_need_no_device():
    err = ctypes.c_int(0)
    heap = (ctypes.c_char * 4)(b"\x05", b"a", b"\0", b"\0")
    offs = (ctypes.c_uint64 * 1)(0)
    assert not lib.strom_keyunion_absorb(None, heap, 4, offs, 1, ctypes.byref(err))
    assert err.value == BAD_REQUEST
    err.value = 0
    assert not lib.strom_keyunion_absorb(None, None, 0, None, 0, None)            # no errcode asked for
    assert not lib.strom_keyunion_absorb_dict(None, None, ctypes.byref(err))
    assert err.value == BAD_REQUEST
    assert lib.strom_keymap_size(None) == 0
    out = (ctypes.c_int32 * 1)()
    assert lib.strom_keymap_fetch(None, out, 1) == BAD_REQUEST
    lib.strom_keymap_release(None)
    col = (ctypes.c_int32 * 1)(0)
    one = (ctypes.c_void_p * 1)(None)
    assert lib.strom_keyunion_recode(None, col, one, 1) == BAD_REQUEST
    assert lib.strom_keyunion_kernel_ns(None, None) == BAD_REQUEST


@pytest.mark.parametrize("hash_bits", [None, 4])
def test_fixed_program_has_the_new_kernels(hash_bits):
    src = textdict.program_source(block=None, hash_bits=hash_bits)
    prog = runtime.DevProgram(src, 0).wait()
    try:
        assert prog.state() == 1
        path = os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)
        code = open(path, "rb").read()
        for name in KERNELS + ["textdict_probe", "textdict_settle", "textdict_emit", "textdict_rebuild"]:
            assert name.encode() + b".kd" in code, name
    finally:
        prog.release()


# ---- the ranks' key images over gloo ------------------------------------------------------------------
def _rank_words(rank):
    """every rank knows every rank's words: what arrives can be checked against what was sent"""
    import text_cases
    w = text_cases.WORDS
    return [w[(5 * rank + 3 * i) % len(w)] for i in range(12 + rank)] + [b"rank %d" % rank] + [b"x" * (125 + rank)]


def _image_of(words):
    from pg_strom_amd import kds
    heap, offs = b"", []
    for p in words:
        offs.append(len(heap))
        d = kds.varlena_datum(p)
        heap += d + b"\0" * (-len(d) % 4)
    return heap, np.array(offs, dtype=np.uint64)


def _keys_of(image):
    heap, offs = image
    out = []
    for at in offs:
        at = int(at)
        if heap[at] & 1:
            out.append(heap[at + 1:at + ((heap[at] >> 1) & 0x7f)])
        else:
            size = int.from_bytes(heap[at:at + 4], "little") >> 2
            out.append(heap[at + 4:at + size])
    return out


def _gather_worker(rank, world, port, outq):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch.distributed as dist
    from pg_strom_amd import parallel
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        images = parallel.allgather_key_images(_image_of(_rank_words(rank)))
        ok = len(images) == world
        for r, (heap, offs) in enumerate(images):                  # in rank order, byte for byte
            want_heap, want_offs = _image_of(_rank_words(r))
            ok = ok and bytes(heap) == want_heap and np.array_equal(offs, want_offs) and offs.dtype == np.uint64
        ids = {}
        for image in images:                                        # what absorbing them in order gives
            for k in _keys_of(image):
                ids.setdefault(bytes(k), len(ids))
        outq.put((rank, bool(ok), ids))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_key_images_arrive_in_rank_order_and_unite_alike(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    want = {}
    for r in range(world):
        for k in _rank_words(r):
            want.setdefault(k, len(want))
    assert sorted(r for r, _, _ in results) == list(range(world))
    for _, ok, ids in results:
        assert ok
        assert ids == want and list(ids) == list(want)
