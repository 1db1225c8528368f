"""
LEFT / SEMI / ANTI relations in the fused lookup and star folds (strom_submit_gpupreagg_lookup_typed),
the parts that need no GPU: the symbols, the define block of a typed mapping, the registers of the
typed kernels (scripts/lookup_join_types_resources.py compiles them for gfx950 from the text the
runtime builds; the bars are test_star_lookup_cpu.py's: no scratch, VGPR + AGPR <= 128), and the
numpy fold rule of test_lookup_join_types_gpu.py held against the nested-loop join_model.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

import join_model as jm
from pg_strom_amd import gpupreagg
from pg_strom_amd._lib import lib, PROTOTYPES
from test_lookup_join_types_gpu import fold_rule
from test_star_lookup_gpu import Dim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resources_module():
    spec = importlib.util.spec_from_file_location(
        "_lookup_join_types_resources", os.path.join(ROOT, "scripts", "lookup_join_types_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RES = _resources_module()


def test_symbols_are_declared_and_resolve():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    for name in ("strom_submit_gpupreagg_lookup_typed", "strom_gpupreagg_lookup_typed_defines",
                 "strom_gpupreagg_mapping_defines"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in PROTOTYPES and getattr(lib, name) is not None
    assert hasattr(gpupreagg.GpuPreAgg, "submit_lookup_typed")


STAR_RELS = [(4, 2, True, [0]), (8, 16, False, [3, 5])]


def test_an_all_inner_block_is_the_stars_byte_for_byte():
    want = gpupreagg.lookup_star_defines(STAR_RELS)
    assert gpupreagg.lookup_typed_defines(STAR_RELS, ["inner", "inner"]) == want
    assert gpupreagg.lookup_typed_defines(STAR_RELS, [0, 0]) == want
    for _, _, relations in RES.STAR.MAPPINGS:
        assert gpupreagg.lookup_typed_defines(relations, [0] * len(relations)) == gpupreagg.lookup_star_defines(relations)
    # one relation: the one-table kernels' block, as the runtime has always built it for an inner mapping
    assert gpupreagg.lookup_typed_defines([(4, 4, True, [0])], ["inner"]) == RES.ONE_TABLE_INNER_DEFINES


def test_define_block_of_a_mixed_mapping():
    rels = [(4, 2, True, []), (4, 4, True, [3, 4]), (8, 2, True, []), (4, 16, False, [5])]
    text = gpupreagg.lookup_typed_defines(rels, ["semi", "left", "anti", "inner"])
    assert text.splitlines() == [
        "#define GPUPREAGG_LOOKUP_ONLY 1", "#define GPUPREAGG_STAR_NRELS 4",
        "#define GPUPREAGG_STAR_RECLEN_1 2", "#define GPUPREAGG_STAR_NARROW_1 1",
        "#define GPUPREAGG_STAR_KEYLEN_1 4", "#define GPUPREAGG_STAR_INNER_MASK_1 0x0UL",
        "#define GPUPREAGG_STAR_JOINTYPE_1 2",
        "#define GPUPREAGG_STAR_RECLEN_2 4", "#define GPUPREAGG_STAR_NARROW_2 1",
        "#define GPUPREAGG_STAR_KEYLEN_2 4", "#define GPUPREAGG_STAR_INNER_MASK_2 0x18UL",
        "#define GPUPREAGG_STAR_JOINTYPE_2 1",
        "#define GPUPREAGG_STAR_RECLEN_3 2", "#define GPUPREAGG_STAR_NARROW_3 1",
        "#define GPUPREAGG_STAR_KEYLEN_3 8", "#define GPUPREAGG_STAR_INNER_MASK_3 0x0UL",
        "#define GPUPREAGG_STAR_JOINTYPE_3 3",
        "#define GPUPREAGG_STAR_RECLEN_4 16", "#define GPUPREAGG_STAR_NARROW_4 0",
        "#define GPUPREAGG_STAR_KEYLEN_4 4", "#define GPUPREAGG_STAR_INNER_MASK_4 0x20UL"]
    # one table: a 32-byte record is the one-table kernel's to read; the type is one more line
    assert gpupreagg.lookup_typed_defines([(8, 32, False, [0, 3])], ["left"]).splitlines() == [
        "#define GPUPREAGG_LOOKUP_ONLY 1", "#define GPUPREAGG_LOOKUP_INNER_MASK 0x9UL",
        "#define GPUPREAGG_LOOKUP_RECLEN 32", "#define GPUPREAGG_LOOKUP_NARROW 0",
        "#define GPUPREAGG_LOOKUP_KEYLEN 8", "#define GPUPREAGG_LOOKUP_JOINTYPE 1"]
    assert gpupreagg.lookup_typed_defines([(4, 2, True, [])], ["anti"]).endswith("#define GPUPREAGG_LOOKUP_JOINTYPE 3\n")


def test_define_block_refusals():
    two = [(4, 2, True, [0]), (4, 2, True, [1])]
    for rels, jts in [(two, ["left", 4]), (two, [-1, 0]),                   # a join type outside 0 .. 3
                      (two, ["left", "semi"]), (two, ["anti", "left"]),     # a column under a semi / anti relation
                      ([(4, 2, True, [0])], ["semi"]), ([(4, 2, True, [0])], [4]),
                      (two, ["left"]),                                      # one type per relation
                      # every case the star block refuses (test_star_lookup_cpu.py), here under a join type
                      ([], []),
                      ([(4, 2, True, [0])] * 5, ["left"] * 5),
                      ([(4, 2, True, [0]), (2, 2, True, [1])], ["left", "left"]),
                      ([(4, 32, False, [0]), (4, 2, True, [1])], ["left", "left"]),
                      ([(4, 16, False, [0]), (4, 16, False, [1]), (4, 2, True, [2])], ["left"] * 3),
                      ([(4, 8, True, [0]), (4, 2, True, [1])], ["left", "left"]),
                      ([(4, 2, True, [0]), (4, 2, True, [0])], ["left", "left"])]:
        with pytest.raises(ValueError):
            gpupreagg.lookup_typed_defines(rels, jts)
    with pytest.raises(ValueError):
        gpupreagg.lookup_typed_defines(two, ["left", "outer"])


def test_the_typed_mappings_are_the_issues():
    shapes = [(len(m[2]), list(m[3])) for m in RES.TYPED_MAPPINGS]
    assert shapes == [(1, ["left"]), (1, ["anti"]), (4, ["semi", "left", "anti", "inner"])]
    assert sorted(keylen for keylen, _, _, _ in RES.TYPED_MAPPINGS[2][2]) == [4, 4, 4, 8]


@pytest.mark.parametrize("mapping", range(3))
def test_typed_kernels_hold_a_tile_without_scratch(mapping):
    name, spec, relations, jointypes, kernels = RES.TYPED_MAPPINGS[mapping]
    prog, path = RES.build(spec, relations, jointypes)
    try:
        code = open(path, "rb").read()
        res = RES.kernel_resources(path)
        for kernel in kernels:
            assert kernel.encode() + b".kd" in code, (name, kernel)
            r = res[kernel]
            print(name, kernel, r)
            assert r["private_segment_fixed_size"] == 0, (name, kernel, r)
            assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, kernel, r)
        assert b"gpupreagg_dense_column.kd" not in code
    finally:
        prog.release()


def test_the_fold_rule_agrees_with_the_nested_loop_model():
    """all four types over one small fact table: NULL keys, keys below and above the range, holes"""
    rng = np.random.default_rng(77)
    n = 400
    dims = [Dim(rng, 30, key_lo=lo, holes=1.5) for lo in (-5, 3, 100, 0)]
    jts = ["left", "semi", "anti", "inner"]
    fk = [d.fact_keys(rng, n, True) for d in dims]
    partners = [d.partner(k, kn) for d, (k, kn) in zip(dims, fk)]
    for d, (k, kn), p in zip(dims, fk, partners):
        off = k.astype(np.int64) - d.key_lo
        assert kn.any() and (off < 0).any() and (off >= d.span).any()
        assert np.count_nonzero((p < 0) & ~kn & (off >= 0) & (off < d.span)) > 0 and (p >= 0).any()
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):                 # the relations commute
        rels = [jm.Rel(dims[r].nd, [jm.Key(jm.outer_column(fk[r][0], fk[r][1]), dims[r].key)], jts[r]) for r in order]
        recs = jm.join_model(np.arange(n), rels)
        keep = fold_rule(partners, jts)
        assert 0 < np.count_nonzero(keep) < n
        assert np.array_equal(np.sort(recs[:, 0] - 1), np.flatnonzero(keep))   # unique keys: a row at most once
        # the left relation's entry: the partner, or none
        left_at = 1 + order.index(0)
        by_row = dict(zip((recs[:, 0] - 1).tolist(), recs[:, left_at].tolist()))
        assert all(by_row[i] == partners[0][i] for i in np.flatnonzero(keep).tolist())
    for jt in jts:                                                           # and one relation alone
        rels = [jm.Rel(dims[0].nd, [jm.Key(jm.outer_column(fk[0][0], fk[0][1]), dims[0].key)], jt)]
        recs = jm.join_model(np.arange(n), rels)
        assert np.array_equal(np.sort(recs[:, 0] - 1), np.flatnonzero(fold_rule(partners[:1], [jt])))
