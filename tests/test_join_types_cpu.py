"""
GpuHashJoin's join types, the parts that need no GPU: the numpy model of tests/join_model.py tied
to the CPU oracle (which knows inner joins only), what the code generator accepts, emits and
refuses for (jointype inner|left|semi|anti), that an all-inner program's text is the text it was,
the one-pass kernels of each join type compiled for gfx950 as the runtime compiles them (no scratch
memory, the LDS of the inner program), and the new ABI symbol.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

import join_model as jm
import oracle_binding as oracle
from pg_strom_amd import runtime
from pg_strom_amd._lib import lib, PROTOTYPES
from pg_strom_amd.gpuhashjoin import codegen_gpuhashjoin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ONE_PASS = ("gpuhashjoin_main_fast", "gpuhashjoin_main_fast_narrow", "gpuhashjoin_main_fast_lds",
            "gpuhashjoin_main_fast_keyed")
NEW_DEFINES = ("#define HASHJOIN_JOIN_TYPE_", "#define HASHJOIN_ALL_INNER", "#define HASHJOIN_FAST_JOINTYPE")
C3_SPEC = "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))"
TWO_REL_SPEC = ("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (hashkey (int8 (var 2 int2)) 2 int8)"
                " (qual (float8gt (ivar 1 3 float8) (var 3 float8))))"
                " (rel (hashkey (ivar 1 4 int4) 1 int4) (qual (int2lt (ivar 2 2 int2) (param 0 int2)))))")


def source_of(spec):
    return codegen_gpuhashjoin(spec).source


def defines_of(source):
    return dict(re.findall(r"^#define (HASHJOIN_\w+) (-?\d+)$", source, re.M))


def refusal(spec):
    with pytest.raises(ValueError) as ei:
        codegen_gpuhashjoin(spec)
    return str(ei.value)


# ---------------------------------------------------------------------------------------------
# the model, with every type inner, is the oracle
# ---------------------------------------------------------------------------------------------
def test_model_equals_oracle_one_relation_duplicates_and_null_keys():
    case = jm.duplicates_case()
    assert case["pkn"].any() and case["fkn"].any()
    assert len(np.unique(case["pk"])) < len(case["pk"])
    stats = []
    want = jm.join_model(np.arange(len(case["fk"])), jm.one_rel_model(case, "inner"), stats=stats)
    assert jm.prefix_kinds(stats[0])
    rc, n, recs = oracle.gpuhashjoin(C3_SPEC, case["outer"](), [case["inner"]])
    assert rc == 0 and n == len(want) > 0
    assert np.array_equal(jm.sorted_records(recs.astype(np.int64)), jm.sorted_records(want))


@pytest.mark.parametrize("fmt", ["row", "column"])
def test_model_equals_oracle_two_relations(fmt):
    d = jm.general_data()
    outer, inners = jm.general_chunks(d, fmt)
    assert jm.two_rel_spec(None, None) == TWO_REL_SPEC
    stats = []
    want = jm.join_model(np.arange(len(d["fa"])), jm.two_rel_model(d, None, None), stats=stats)
    assert jm.prefix_kinds(stats[0]) and jm.prefix_kinds(stats[1])
    rc, n, recs = oracle.gpuhashjoin(TWO_REL_SPEC, outer, inners[:2], [np.int16(jm.PARAM_V2)])
    assert rc == 0 and n == len(want) > 0
    assert np.array_equal(jm.sorted_records(recs.astype(np.int64)), jm.sorted_records(want))


def test_model_join_types_on_a_hand_made_case():
    """four outer rows against keys {1, 1, 2, NULL}: two partners, one, none, a NULL key"""
    fk, fkn = np.array([1, 2, 3, 0]), np.array([False, False, False, True])
    pk, pkn = np.array([1, 1, 2, 0]), np.array([False, False, False, True])
    rel = lambda t: [jm.Rel(4, [jm.Key(jm.outer_column(fk, fkn), pk, pkn)], t)]
    rows = np.arange(4)
    assert jm.sorted_records(jm.join_model(rows, rel("inner"))).tolist() == [[1, 0], [1, 1], [2, 2]]
    assert jm.sorted_records(jm.join_model(rows, rel("left"))).tolist() == [[1, 0], [1, 1], [2, 2], [3, -1], [4, -1]]
    assert jm.sorted_records(jm.join_model(rows, rel("semi"))).tolist() == [[1, -1], [2, -1]]
    # NOT EXISTS, not NOT IN: the row with the NULL key survives
    assert jm.sorted_records(jm.join_model(rows, rel("anti"))).tolist() == [[3, -1], [4, -1]]


# ---------------------------------------------------------------------------------------------
# the code generator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("position", [0, 1, 2])
@pytest.mark.parametrize("jointype,number", [("inner", 0), ("left", 1), ("semi", 2), ("anti", 3)])
def test_all_four_names_in_any_item_position(jointype, number, position):
    items = ["(hashkey (var 1 int4) 1 int4)", "(qual (int4lt (var 2 int4) (ivar 1 2 int4)))"]
    items.insert(position, "(jointype %s)" % jointype)
    d = defines_of(source_of("(gpuhashjoin (rel %s))" % " ".join(items)))
    assert d["HASHJOIN_JOIN_TYPE_1"] == str(number)
    assert d["HASHJOIN_ALL_INNER"] == ("1" if jointype == "inner" else "0")


def test_defines_of_the_one_pass_programs():
    for jointype, number in (("left", 1), ("semi", 2), ("anti", 3)):
        src = source_of(jm.one_rel_spec(jointype))
        d = defines_of(src)
        assert d["HASHJOIN_FAST_JOINTYPE"] == str(number) and d["HASHJOIN_FAST_ELIGIBLE"] == "0"
        assert d["HASHJOIN_ALL_INNER"] == "0" and d["HASHJOIN_FAST_OUTER_QUAL"] == "0"
        # hashjoin_fast_outer_key is emitted as for a fast inner program: it reads the key
        body = re.search(r"hashjoin_fast_outer_key\(.*?\n\{(.*?)\n\}", src, re.S).group(1)
        assert "KVAR_1" in body and "return false" not in body
    d = defines_of(source_of(C3_SPEC))
    assert d["HASHJOIN_FAST_JOINTYPE"] == "0" and d["HASHJOIN_FAST_ELIGIBLE"] == "1" and d["HASHJOIN_ALL_INNER"] == "1"


@pytest.mark.parametrize("jointype", ["left", "semi", "anti"])
def test_a_qual_sends_a_non_inner_join_to_the_general_kernel(jointype):
    """... a qual over outer columns only included: the pulled-up-qual rule does not carry over"""
    for qual in ("(int4lt (var 2 int4) (const int4 5))", "(int4lt (ivar 1 2 int4) (const int4 5))"):
        d = defines_of(source_of("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (qual %s) (jointype %s)))"
                                 % (qual, jointype)))
        assert d["HASHJOIN_FAST_JOINTYPE"] == "0" and d["HASHJOIN_FAST_ELIGIBLE"] == "0"
        assert d["HASHJOIN_FAST_OUTER_QUAL"] == "0"
    # a text key, two keys, two relations: not the one-pass shape either
    for spec in ("(gpuhashjoin (rel (hashkey (var 1 text) 1 text) (jointype %s)))",
                 "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (hashkey (var 2 int4) 2 int4) (jointype %s)))",
                 "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (jointype %s)) (rel (hashkey (var 2 int4) 1 int4)))"):
        d = defines_of(source_of(spec % jointype))
        assert d["HASHJOIN_FAST_JOINTYPE"] == "0" and d["HASHJOIN_FAST_ELIGIBLE"] == "0"


def test_defines_of_a_three_relation_program():
    d = defines_of(source_of(jm.THREE_REL_SPEC))
    assert [d["HASHJOIN_JOIN_TYPE_%d" % i] for i in (1, 2, 3)] == ["1", "2", "3"]
    assert d["HASHJOIN_ALL_INNER"] == "0" and d["HASHJOIN_FAST_JOINTYPE"] == "0" and d["HASHJOIN_NRELS"] == "3"


def test_refusals_name_their_cause():
    key = "(hashkey (var 1 int4) 1 int4)"
    msg = refusal("(gpuhashjoin (rel (jointype semi) %s (jointype semi)))" % key)
    assert "duplicate jointype" in msg
    msg = refusal("(gpuhashjoin (rel %s (jointype inner) (jointype left)))" % key)
    assert "duplicate jointype" in msg
    for name in ("right", "full"):
        msg = refusal("(gpuhashjoin (rel %s (jointype %s)))" % (key, name))
        assert ("jointype %s is not supported" % name) in msg
    assert "unknown jointype cross" in refusal("(gpuhashjoin (rel %s (jointype cross)))" % key)
    for hidden in ("semi", "anti"):
        # ... in a key of depth d + 1, and in a qual two depths down
        msg = refusal("(gpuhashjoin (rel (jointype %s) %s) (rel (hashkey (ivar 1 2 int4) 1 int4)))" % (hidden, key))
        assert "a semi/anti relation exposes no columns" in msg and "(ivar 1 ..)" in msg
        msg = refusal("(gpuhashjoin (rel %s) (rel %s (jointype %s)) (rel %s (qual (int4lt (ivar 2 2 int4) (var 2 int4)))))"
                      % (key, key, hidden, key))
        assert "a semi/anti relation exposes no columns" in msg and "(ivar 2 ..)" in msg
        # the relation's own qual may read it
        codegen_gpuhashjoin("(gpuhashjoin (rel (jointype %s) %s (qual (int4lt (ivar 1 2 int4) (var 2 int4)))))" % (hidden, key))


def without_new_defines(source):
    return [line for line in source.splitlines() if not line.startswith(NEW_DEFINES)]


@pytest.mark.parametrize("golden,spec,named", [
    ("hashjoin_codegen_inner_one_rel.txt", C3_SPEC, jm.one_rel_spec("inner")),
    ("hashjoin_codegen_inner_two_rel.txt", TWO_REL_SPEC, jm.two_rel_spec("inner", "inner")),
])
def test_an_inner_program_is_the_text_it_was(golden, spec, named):
    """tests/golden holds what the generator emitted for these specs before it knew join types"""
    before = open(os.path.join(GOLDEN, golden)).read()
    assert not any(line.startswith(NEW_DEFINES) for line in before.splitlines())
    plain, with_name = source_of(spec), source_of(named)
    assert any(line.startswith(NEW_DEFINES) for line in plain.splitlines())
    assert without_new_defines(plain) == before.splitlines()
    assert without_new_defines(with_name) == before.splitlines()
    assert plain == with_name


def test_eight_left_relations_emit_the_innermost_block_once():
    spec = "(gpuhashjoin%s)" % "".join(" (rel (jointype left) (hashkey (var %d int4) 1 int4))" % (i + 1) for i in range(8))
    src = source_of(spec)
    assert src.count("rbuffer += 9;") == 1
    assert src.count("n_matches++;") == 1
    assert src.count("hashjoin_first(hjidx, ") == 8          # one chain walk per relation


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


def test_one_pass_kernels_of_every_join_type_use_no_scratch_and_the_same_lds():
    inner = compiled_resources(C3_SPEC)
    for k in ONE_PASS:
        assert inner[k]["private_segment_fixed_size"] == 0, (k, inner[k])
    for spec in (jm.one_rel_spec("left"), jm.one_rel_spec("semi"), jm.one_rel_spec("anti"), jm.THREE_REL_SPEC):
        res = compiled_resources(spec)
        for k in ONE_PASS:
            print(spec[:40], k, res[k])
            assert res[k]["private_segment_fixed_size"] == 0, (spec, k, res[k])
            assert res[k]["group_segment_fixed_size"] == inner[k]["group_segment_fixed_size"], (spec, k)
        assert "gpuhashjoin_main" in res


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
def test_rowmap_from_join_task_is_declared_and_resolves():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    name = "strom_rowmap_from_join_task"
    assert re.search(r"\b%s\s*\(\s*strom_task \*\w+,\s*strom_hashjoin_table \*\w+,\s*int \*\w+\)" % name, header)
    assert name in PROTOTYPES and getattr(lib, name) is not None
    assert "rowmap_from_join_results" in open(os.path.join(ROOT, "pg_strom_amd", "csrc", "devlib", "strom_rowmap.h")).read()
    # the header states what 0 means in a record, and what is out of scope
    assert "OFFSET 0 IS NEVER AN ENTRY" in header and "RIGHT and FULL joins are out of scope" in header
