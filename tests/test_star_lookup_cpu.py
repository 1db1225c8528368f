"""
The star lookup (strom_submit_gpupreagg_lookup_star), the parts that need no GPU: the symbol, the
define block of a mapping, and the condition its kernels live under -- at 1024 threads a wave has
128 VGPRs, and gpupreagg_dense_lookup_star / gpupreagg_packed_lookup_star must hold the keys,
slots and record words of every relation of a tile without scratch memory.  The three mappings
(scripts/star_lookup_resources.py): two narrow relations; an 8-byte and a 16-byte record; four
narrow relations, one keyed by int8.  Each program is compiled for gfx950 from the text the
runtime builds (gpupreagg.lookup_star_defines + the session's source) and the registers are read
from the code object.
"""
import importlib.util
import os
import re

import pytest

from pg_strom_amd import gpupreagg
from pg_strom_amd._lib import lib, PROTOTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resources_module():
    spec = importlib.util.spec_from_file_location(
        "_star_lookup_resources", os.path.join(ROOT, "scripts", "star_lookup_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RES = _resources_module()


def test_symbols_are_declared_and_resolve():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    for name in ("strom_submit_gpupreagg_lookup_star", "strom_gpupreagg_lookup_star_defines"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in PROTOTYPES and getattr(lib, name) is not None
    assert re.search(r"#define\s+STROM_LOOKUP_STAR_MAXRELS\s+4\b", header)


def test_the_three_mappings_are_the_issues():
    rels = [m[2] for m in RES.MAPPINGS]
    assert len(rels) == 3
    assert len(rels[0]) == 2 and all(narrow for _, _, narrow, _ in rels[0])
    assert [(reclen, narrow) for _, reclen, narrow, _ in rels[1]] == [(8, False), (16, False)]
    assert len(rels[2]) == 4 and all(narrow for _, _, narrow, _ in rels[2])
    assert sorted(keylen for keylen, _, _, _ in rels[2]) == [4, 4, 4, 8]


def test_define_block_of_a_mapping():
    text = gpupreagg.lookup_star_defines([(4, 2, True, [0]), (8, 16, False, [3, 5])])
    assert text.splitlines() == [
        "#define GPUPREAGG_LOOKUP_ONLY 1", "#define GPUPREAGG_STAR_NRELS 2",
        "#define GPUPREAGG_STAR_RECLEN_1 2", "#define GPUPREAGG_STAR_NARROW_1 1",
        "#define GPUPREAGG_STAR_KEYLEN_1 4", "#define GPUPREAGG_STAR_INNER_MASK_1 0x1UL",
        "#define GPUPREAGG_STAR_RECLEN_2 16", "#define GPUPREAGG_STAR_NARROW_2 0",
        "#define GPUPREAGG_STAR_KEYLEN_2 8", "#define GPUPREAGG_STAR_INNER_MASK_2 0x28UL"]
    for bad in ([],                                                     # no relation
                [(4, 2, True, [0])] * 5,                                # more than STROM_LOOKUP_STAR_MAXRELS
                [(4, 2, True, [0]), (2, 2, True, [1])],                 # a 2-byte key
                [(4, 32, False, [0]), (4, 2, True, [1])],               # a record longer than 16 bytes
                [(4, 16, False, [0]), (4, 16, False, [1]), (4, 2, True, [2])],  # more than 32 bytes a row
                [(4, 8, True, [0]), (4, 2, True, [1])],                 # narrow records are 2 or 4 bytes
                [(4, 2, True, [0]), (4, 2, True, [0])]):                # a column with two sources
        with pytest.raises(ValueError):
            gpupreagg.lookup_star_defines(bad)


@pytest.mark.parametrize("mapping", range(3))
def test_star_kernels_hold_a_tile_without_scratch(mapping):
    name, spec, relations = RES.MAPPINGS[mapping]
    prog, path = RES.build(spec, relations)
    try:
        code = open(path, "rb").read()
        res = RES.kernel_resources(path)
        for kernel in RES.KERNELS:
            assert kernel.encode() + b".kd" in code, (name, kernel)
            r = res[kernel]
            print(name, kernel, r)
            assert r["private_segment_fixed_size"] == 0, (name, kernel, r)
            assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, kernel, r)
        # built FOR the mapping: only the lookup family and the merge kernels are in it
        assert b"gpupreagg_dense_column.kd" not in code
    finally:
        prog.release()
