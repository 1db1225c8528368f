"""
RIGHT and FULL joins in the fused lookup and star folds (strom_submit_gpupreagg_lookup_tracked /
_lookup_unmatched), the parts that need no GPU: the symbols, the define blocks, the registers of the tracked
kernels and of the unmatched kernel (scripts/lookup_tracked_resources.py compiles them for gfx950 from the
text the runtime builds; the bars are test_lookup_join_types_cpu.py's: no scratch, VGPR + AGPR <= 128), and
the numpy model of tests/tracked_fold_model.py held against tests/outer_join_model.py over the nested-loop
join_model.  The parent of this change has none of the symbols: every test here fails there.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

import join_model as jm
import outer_join_model as om
import tracked_fold_model as tm
from pg_strom_amd import gpupreagg
from pg_strom_amd._lib import lib, PROTOTYPES
from test_star_lookup_gpu import Dim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RES = _module("lookup_tracked_resources")
JT = RES.JT

SYMBOLS = ("strom_submit_gpupreagg_lookup_tracked", "strom_submit_gpupreagg_lookup_unmatched",
           "strom_gpupreagg_lookup_tracked_defines", "strom_gpupreagg_lookup_unmatched_defines",
           "strom_gpupreagg_lookup_matches_length", "strom_gpupreagg_lookup_matches_fetch",
           "strom_gpupreagg_lookup_matches_merge", "strom_gpupreagg_lookup_reset_matches")


def test_symbols_are_declared_and_resolve():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in PROTOTYPES and getattr(lib, name) is not None
    for name in ("submit_lookup_tracked", "submit_lookup_unmatched", "lookup_matches", "merge_lookup_matches",
                 "reset_lookup_matches"):
        assert hasattr(gpupreagg.GpuPreAgg, name)
    # the calls that need no session refuse a NULL one
    assert lib.strom_gpupreagg_lookup_matches_length(None) == 0
    assert lib.strom_gpupreagg_lookup_matches_fetch(None, None, 0) == 101
    assert lib.strom_gpupreagg_lookup_matches_merge(None, None, 0) == 101
    assert lib.strom_gpupreagg_lookup_reset_matches(None) == 101


def test_nothing_tracked_is_the_typed_block_byte_for_byte():
    for _, _, relations, jointypes, _ in JT.TYPED_MAPPINGS:
        assert gpupreagg.lookup_tracked_defines(relations, jointypes, 0) == \
            gpupreagg.lookup_typed_defines(relations, jointypes)
    for _, _, relations in JT.STAR.MAPPINGS:
        assert gpupreagg.lookup_tracked_defines(relations, [0] * len(relations), 0) == \
            gpupreagg.lookup_star_defines(relations)
    assert gpupreagg.lookup_tracked_defines([(4, 4, True, [0])], ["inner"], 0) == JT.ONE_TABLE_INNER_DEFINES


def test_a_tracked_block_is_the_typed_block_and_one_line():
    one = [(4, 4, True, [0])]
    for jt in ("inner", "left"):
        assert gpupreagg.lookup_tracked_defines(one, [jt], 1) == \
            gpupreagg.lookup_typed_defines(one, [jt]) + "#define GPUPREAGG_LOOKUP_TRACK 1\n"
    rels = [(4, 2, True, []), (4, 4, True, [3, 4]), (8, 2, True, []), (4, 16, False, [5])]
    jts = ["semi", "left", "anti", "inner"]
    for d in (2, 4):
        assert gpupreagg.lookup_tracked_defines(rels, jts, d) == \
            gpupreagg.lookup_typed_defines(rels, jts) + "#define GPUPREAGG_STAR_TRACK_REL %d\n" % d
    # an all-inner star with a tracked relation: the star's block and the line
    two = [(4, 2, True, [0]), (4, 4, True, [3])]
    assert gpupreagg.lookup_tracked_defines(two, [0, 0], 1) == \
        gpupreagg.lookup_star_defines(two) + "#define GPUPREAGG_STAR_TRACK_REL 1\n"


def test_the_unmatched_block_holds_the_record_facts_only():
    assert gpupreagg.lookup_unmatched_defines((8, 4, True, [0, 3])).splitlines() == [
        "#define GPUPREAGG_LOOKUP_ONLY 1", "#define GPUPREAGG_UNMATCHED_RECLEN 4",
        "#define GPUPREAGG_UNMATCHED_NARROW 1", "#define GPUPREAGG_UNMATCHED_INNER_MASK 0x9UL"]
    # (no key width in it: the same text whatever the key)
    assert gpupreagg.lookup_unmatched_defines((4, 32, False, [1])) == gpupreagg.lookup_unmatched_defines((8, 32, False, [1]))
    for bad in [(4, 3, True, [0]), (4, 8, True, [0]), (4, 6, False, [0]), (4, 4, False, [0])]:
        with pytest.raises(ValueError):
            gpupreagg.lookup_unmatched_defines(bad)


def test_define_block_refusals():
    rels = [(4, 2, True, []), (4, 4, True, [3, 4]), (8, 2, True, []), (4, 2, True, [5])]
    jts = ["semi", "left", "anti", "inner"]
    for tracked in (-1, 5, 1, 3):                       # out of range; a semi and an anti relation
        with pytest.raises(ValueError):
            gpupreagg.lookup_tracked_defines(rels, jts, tracked)
    for jt, tracked in (("semi", 1), ("anti", 1), ("left", 2), ("inner", -1)):
        with pytest.raises(ValueError):
            gpupreagg.lookup_tracked_defines([(4, 2, True, [])], [jt], tracked)
    with pytest.raises(ValueError):                     # what the typed block refuses stays refused
        gpupreagg.lookup_tracked_defines([(4, 2, True, [0])], ["semi"], 0)
    with pytest.raises(ValueError):
        gpupreagg.lookup_tracked_defines(rels, jts[:3], 2)


def test_the_tracked_mappings_are_the_issues():
    shapes = [(len(m[2]), list(m[3]), m[4]) for m in RES.TRACKED_MAPPINGS]
    assert shapes == [(1, ["inner"], 1), (1, ["left"], 1), (4, ["semi", "left", "anti", "inner"], 2)]


@pytest.mark.parametrize("mapping", range(3))
def test_tracked_and_unmatched_kernels_hold_a_tile_without_scratch(mapping):
    name, spec, relations, jointypes, tracked, kernels = RES.TRACKED_MAPPINGS[mapping]
    for prog, path, names in [RES.build_tracked(spec, relations, jointypes, tracked) + (kernels,),
                              RES.build_unmatched(spec, relations[tracked - 1]) + (RES.UNMATCHED_KERNELS,)]:
        try:
            code = open(path, "rb").read()
            res = RES.kernel_resources(path)
            for kernel in names:
                assert kernel.encode() + b".kd" in code, (name, kernel)
                r = res[kernel]
                print(name, kernel, r)
                assert r["private_segment_fixed_size"] == 0, (name, kernel, r)
                assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, kernel, r)
            assert b"gpupreagg_dense_column.kd" not in code
            if names is RES.UNMATCHED_KERNELS:          # the pass's program holds no chunk fold
                assert b"gpupreagg_dense_lookup.kd" not in code
        finally:
            prog.release()


@pytest.mark.parametrize("tracked_type", ["inner", "left"])
def test_the_model_agrees_with_the_nested_loop_unmatched_model(tracked_type):
    """about 400 rows in two chunks, four 30-row dimensions with NULL keys, keys below and above the range
    and holes; every join type for the other relations, the tracked relation joined last"""
    rng = np.random.default_rng(91)
    n = 400
    dims = [Dim(rng, 30, key_lo=lo, holes=1.5) for lo in (-5, 3, 100, 0)]
    fk = [d.fact_keys(rng, n, True) for d in dims]
    partners = [d.partner(k, kn) for d, (k, kn) in zip(dims, fk)]
    for d, (k, kn), p in zip(dims, fk, partners):
        off = k.astype(np.int64) - d.key_lo
        assert kn.any() and (off < 0).any() and (off >= d.span).any()
        assert np.count_nonzero((p < 0) & ~kn & (off >= 0) & (off < d.span)) > 0 and (p >= 0).any()
    bounds = [(0, 170), (170, n)]
    seen_some = 0
    for others in (["left", "semi", "anti"], ["anti", "inner", "left"], ["semi", "semi", "inner"], ["inner"], []):
        for tracked in range(1, len(others) + 2):
            jts = others[:tracked - 1] + [tracked_type] + others[tracked - 1:]
            R = len(jts)
            chunks = [[p[lo:hi] for p in partners[:R]] for lo, hi in bounds]
            matched, folded, unmatched = tm.tracked_model(chunks, dims[:R], jts, tracked)
            # the nested-loop model joins in program order: the tracked relation goes last
            order = [q for q in range(R) if q != tracked - 1] + [tracked - 1]
            rels = [jm.Rel(dims[q].nd, [jm.Key(jm.outer_column(fk[q][0], fk[q][1]), dims[q].key)], jts[q]) for q in order]
            feeds = [(np.arange(lo, hi), rels) for lo, hi in bounds]
            assert np.array_equal(matched, om.matched_rowids(feeds)), (jts, tracked)
            assert np.array_equal(unmatched, om.unmatched_rowids(dims[tracked - 1].nd, feeds)), (jts, tracked)
            assert len(matched) + len(unmatched) == dims[tracked - 1].nd
            seen_some += (0 < len(unmatched) < dims[tracked - 1].nd)
            # the per-chunk fold is the typed fold of the same join types
            for (lo, hi), keep in zip(bounds, folded):
                recs = jm.join_model(np.arange(lo, hi), rels)
                assert np.array_equal(np.sort(recs[:, 0] - 1), lo + np.flatnonzero(keep))
            # the image: one byte per slot, matched rows at key - smallest key
            img = tm.matches_image(dims[tracked - 1], matched)
            assert img.dtype == np.uint8 and img.sum() == len(matched)
            assert len(img) == dims[tracked - 1].key.max() - dims[tracked - 1].key.min() + 1
    assert seen_some > 5
