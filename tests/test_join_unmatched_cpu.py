"""
RIGHT and FULL joins through matched-entry flags, the parts that need no GPU: what the code generator
accepts, emits and refuses for (track_matches), that a program without the item gets no new define,
that (jointype right|full) stay refused, the new ABI symbols, the model of tests/outer_join_model.py
on a hand-made case, and the tracked kernels compiled for gfx950 as the runtime compiles them (no
scratch memory, the LDS of the untracked program).
"""
import importlib.util
import os
import re

import numpy as np
import pytest

import join_model as jm
import outer_join_model as ojm
from pg_strom_amd import runtime
from pg_strom_amd._lib import lib, PROTOTYPES
from pg_strom_amd.gpuhashjoin import codegen_gpuhashjoin, GpuHashJoin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_PASS = ("gpuhashjoin_main_fast", "gpuhashjoin_main_fast_narrow", "gpuhashjoin_main_fast_lds",
            "gpuhashjoin_main_fast_keyed")
KEY = "(hashkey (var 1 int4) 1 int4)"
NEW_SYMBOLS = ("strom_submit_gpuhashjoin_unmatched", "strom_submit_gpuhashjoin_unmatched_projection",
               "strom_hashjoin_table_tracked_depth", "strom_hashjoin_table_reset_matches",
               "strom_hashjoin_table_matches_length", "strom_hashjoin_table_matches_fetch",
               "strom_hashjoin_table_matches_merge")


def tracked_spec(jointype=None):
    return "(gpuhashjoin (rel %s%s (track_matches)))" % (KEY, "" if jointype is None else " (jointype %s)" % jointype)


def source_of(spec):
    return codegen_gpuhashjoin(spec).source


def defines_of(source):
    return dict(re.findall(r"^#define (HASHJOIN_\w+) (-?\d+)$", source, re.M))


def refusal(spec):
    with pytest.raises(ValueError) as ei:
        codegen_gpuhashjoin(spec)
    return str(ei.value)


# ---------------------------------------------------------------------------------------------
# the code generator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("position", [0, 1, 2])
@pytest.mark.parametrize("jointype,number", [(None, 0), ("inner", 0), ("left", 1)])
def test_track_matches_in_any_item_position(jointype, number, position):
    items = [KEY] + (["(jointype %s)" % jointype] if jointype else ["(qual (int4lt (var 2 int4) (ivar 1 2 int4)))"])
    items.insert(position, "(track_matches)")
    src = source_of("(gpuhashjoin (rel %s))" % " ".join(items))
    d = defines_of(src)
    assert d["HASHJOIN_TRACK_DEPTH"] == "1" and d["HASHJOIN_JOIN_TYPE_1"] == str(number)
    # the count pass flags the candidate, the emit pass does not
    assert src.count("hashjoin_flag_matched(hjidx, off_1)") == 1
    assert "if (!rbuffer && off_1 != 0)" in src


def test_the_per_chunk_program_is_the_inner_or_left_program():
    """the tracked text = the untracked text + one define + the flag in the count pass"""
    for jointype in ("inner", "left"):
        plain = source_of(jm.one_rel_spec(jointype)).splitlines()
        tracked = source_of(tracked_spec(jointype)).splitlines()
        extra = [line for line in tracked if line not in plain]
        assert [e.strip() for e in extra] == ["#define HASHJOIN_TRACK_DEPTH 1", "if (!rbuffer && off_1 != 0)",
                                              "hashjoin_flag_matched(hjidx, off_1);"]
        assert [line for line in tracked if line not in extra] == plain
        d = defines_of("\n".join(tracked))
        # a tracked INNER program stays "all inner" and one-pass eligible; a tracked LEFT one is one-pass LEFT
        assert d["HASHJOIN_FAST_ELIGIBLE"] == ("1" if jointype == "inner" else "0")
        assert d["HASHJOIN_FAST_JOINTYPE"] == ("0" if jointype == "inner" else "1")


def test_the_last_of_several_relations():
    for t1 in ("inner", "left", "semi", "anti"):
        for t2 in ("inner", "left"):
            spec = jm.two_rel_spec(t1, t2)[:-2] + " (track_matches)))"
            src = source_of(spec)
            assert defines_of(src)["HASHJOIN_TRACK_DEPTH"] == "2"
            assert src.count("hashjoin_flag_matched(hjidx, off_2)") == 1 and "hashjoin_flag_matched(hjidx, off_1)" not in src


def test_a_program_without_the_item_has_no_such_define():
    for spec in (jm.one_rel_spec(), jm.one_rel_spec("left"), jm.one_rel_spec("semi"), jm.two_rel_spec("left", "inner"),
                 jm.THREE_REL_SPEC):
        src = source_of(spec)
        assert "HASHJOIN_TRACK_DEPTH" not in src and "hashjoin_flag_matched" not in src


def test_refusals_name_their_cause():
    assert "duplicate track_matches" in refusal("(gpuhashjoin (rel (track_matches) %s (track_matches)))" % KEY)
    msg = refusal("(gpuhashjoin (rel %s (track_matches)) (rel (hashkey (var 2 int4) 1 int4)))" % KEY)
    assert "track_matches on rel 1" in msg and "only the last relation" in msg
    for t in ("semi", "anti"):
        msg = refusal("(gpuhashjoin (rel %s (jointype %s) (track_matches)))" % (KEY, t))
        assert ("track_matches on a %s relation" % t) in msg
        msg = refusal("(gpuhashjoin (rel (track_matches) (jointype %s) %s))" % (t, KEY))
        assert ("track_matches on a %s relation" % t) in msg
    assert "takes no argument" in refusal("(gpuhashjoin (rel %s (track_matches 1)))" % KEY)
    # the join types themselves stay refused, tracked or not
    for name in ("right", "full"):
        for item in ("", " (track_matches)"):
            msg = refusal("(gpuhashjoin (rel %s (jointype %s)%s))" % (KEY, name, item))
            assert ("jointype %s is not supported" % name) in msg


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def test_model_on_a_hand_made_case():
    """inner keys {1, 1, 2, NULL, 7}; two chunks: keys {1, 3} and {NULL, 2}"""
    pk, pkn = np.array([1, 1, 2, 0, 7]), np.array([False, False, False, True, False])
    fk, fkn = np.array([1, 3, 0, 2]), np.array([False, False, True, False])
    for jointype in ("inner", "left"):
        rels = [jm.Rel(5, [jm.Key(jm.outer_column(fk, fkn), pk, pkn)], jointype)]
        assert ojm.unmatched_rowids(5, []).tolist() == [0, 1, 2, 3, 4]
        assert ojm.unmatched_rowids(5, [(np.array([0, 1]), rels)]).tolist() == [2, 3, 4]
        assert ojm.unmatched_rowids(5, [(np.array([0, 1]), rels), (np.array([2, 3]), rels)]).tolist() == [3, 4]
    # a qual that rejects entry 1: it stays unmatched although its key is equal
    rels = [jm.Rel(5, [jm.Key(jm.outer_column(fk, fkn), pk, pkn)], "left", lambda orow, irows, e: e != 1)]
    assert ojm.unmatched_rowids(5, [(np.arange(4), rels)]).tolist() == [1, 3, 4]


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_resolve():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*strom_hashjoin_table \*tbl" % name, header), name
        assert name in PROTOTYPES and getattr(lib, name) is not None, name
    assert "OFFSET 0 IS NEVER AN ENTRY" in header and "RIGHT and FULL joins are out of scope" in header
    assert 'WORD 0 == 0 MEANS "NO' in header
    for method in ("unmatched", "unmatched_project", "unmatched_project_rows", "unmatched_to_column",
                   "reset_matches", "matches_image", "merge_matches"):
        assert callable(getattr(GpuHashJoin, method))
    # a NULL table is refused, not followed
    assert lib.strom_hashjoin_table_tracked_depth(None) == 0
    assert lib.strom_hashjoin_table_matches_length(None) == 0
    assert lib.strom_hashjoin_table_reset_matches(None) != 0


def test_every_consumer_of_a_join_task_knows_the_unmatched_pass():
    """A task of the unmatched pass is a join task whose records have word 0 == 0.  Each call that takes
    a join task either serves such records or refuses them before anything is launched (the refusals
    themselves run in test_join_unmatched_gpu.py; here: that no consumer was forgotten)."""
    csrc = os.path.join(ROOT, "pg_strom_amd", "csrc")
    consumers = {}
    for name in ("gpuhashjoin.cpp", "gpupreagg.cpp"):
        text = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r"->res_is_join(?! = true)", text):      # the readers, not the launch that sets it
            # the statement that reads res_is_join, and the few lines behind it
            consumers[(name, text.count("\n", 0, m.start()) + 1)] = text[m.start() - 400:m.start() + 900]
    assert len(consumers) == 3, sorted(consumers)        # project_column, rowmap_from_join_task, the joined fold
    for where, body in consumers.items():
        assert "res_is_unmatched" in body or "jointype != 2 && jointype != 3" in body, where
    fold = [b for (name, _), b in consumers.items() if name == "gpupreagg.cpp"][0]
    assert re.search(r"ok = ok && !\(jtask && jtask->res_is_unmatched\)", fold)
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    assert "refuses a task of the unmatched pass" in header and "strom_multihash_build()" in header


# ---------------------------------------------------------------------------------------------
# compiled for gfx950 as the runtime compiles it
# ---------------------------------------------------------------------------------------------
def _resources_module():
    spec = importlib.util.spec_from_file_location(
        "_star_lookup_resources", os.path.join(ROOT, "scripts", "star_lookup_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compiled_resources(spec):
    cg = codegen_gpuhashjoin(spec)
    prog = runtime.DevProgram(cg.source, cg.extra_flags).wait()
    try:
        path = os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)
        return _resources_module().kernel_resources(path)
    finally:
        prog.release()


@pytest.mark.parametrize("jointype", ["inner", "left"])
def test_tracked_kernels_use_no_scratch_and_the_same_lds(jointype):
    plain = compiled_resources(jm.one_rel_spec(jointype))
    tracked = compiled_resources(tracked_spec(jointype))
    assert "gpuhashjoin_unmatched" not in plain and "hashjoin_matches_kernel" not in plain
    for k in ONE_PASS:
        print(jointype, k, plain[k], tracked[k])
        assert tracked[k]["private_segment_fixed_size"] == 0, (k, tracked[k])
        assert tracked[k]["group_segment_fixed_size"] == plain[k]["group_segment_fixed_size"], k
    assert tracked["gpuhashjoin_unmatched"]["private_segment_fixed_size"] == 0, tracked["gpuhashjoin_unmatched"]
    assert tracked["hashjoin_matches_kernel"]["private_segment_fixed_size"] == 0
    # the stage of the one-pass kernels, nothing beside it
    assert tracked["gpuhashjoin_unmatched"]["group_segment_fixed_size"] <= plain["gpuhashjoin_main_fast"]["group_segment_fixed_size"]
