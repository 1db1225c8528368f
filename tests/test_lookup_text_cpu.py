"""
Text / character(n) fact columns in the fused join-and-aggregate kernels, the parts that need no
GPU: the program text of a text mapping builds for gfx950 through the route
tests/test_star_lookup_cpu.py uses (the define block the runtime puts in front of the session's
source, hiprtc cross-compiling), the five kernels are in the code objects -- and the kernels of
the mappings WITHOUT text still hold a tile without scratch memory under the new device library.
"""
import importlib.util
import os

import pytest

from pg_strom_amd import gpupreagg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


STAR_RES = _script("star_lookup_resources")
TEXT_RES = _script("lookup_text_resources")


def test_the_generated_program_lists_its_text_variables():
    """what csrc/gpupreagg.cpp reads the text variables from, and what compiles the conversion away"""
    src = gpupreagg.codegen_gpupreagg(TEXT_RES.TEXT_SPEC).source
    lists = [line for line in src.splitlines() if line.startswith("#define STROM_KVARLENA_LIST(X)")]
    assert len(lists) == 1                                              # (entries in the order of first use)
    assert sorted(lists[0].split()[2:]) == ["X(4,text)", "X(5,bpcharn)"]
    assert "STROM_KVARLENA_LIST" not in gpupreagg.codegen_gpupreagg(TEXT_RES.DEFAULT_SPEC).source


def test_text_mappings_build_and_the_five_kernels_resolve():
    """the one-table defines, the session's own program (run-time mapping, the joined kernel) and a
    two-relation lookup_star_defines block in front of a program with text variables"""
    seen = set()
    for title, spec, defines, kernels in TEXT_RES.text_programs(ROOT):
        prog, path = TEXT_RES.build_text(ROOT, spec, defines)
        try:
            code = open(path, "rb").read()
            res = STAR_RES.kernel_resources(path)
            for kernel in kernels:
                assert kernel.encode() + b".kd" in code, (title, kernel)
                r = res[kernel]
                print(title, kernel, r)
                assert r["vgpr_count"] + r["agpr_count"] <= 128, (title, kernel, r)
                seen.add(kernel)
        finally:
            prog.release()
    assert seen == set(TEXT_RES.ONE + TEXT_RES.STAR + TEXT_RES.JOINED)


@pytest.mark.parametrize("mapping", range(3))
def test_star_kernels_without_text_still_hold_a_tile_without_scratch(mapping):
    name, spec, relations = STAR_RES.MAPPINGS[mapping]
    prog, path = STAR_RES.build(spec, relations)
    try:
        res = STAR_RES.kernel_resources(path)
        for kernel in STAR_RES.KERNELS:
            r = res[kernel]
            assert r["private_segment_fixed_size"] == 0, (name, kernel, r)
            assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, kernel, r)
    finally:
        prog.release()


def test_the_default_one_table_mapping_still_holds_a_tile_without_scratch():
    """the hot kernel: the canonical scan+join+group-by program built FOR its mapping"""
    prog, path = TEXT_RES.build_text(ROOT, TEXT_RES.DEFAULT_SPEC, TEXT_RES.one_table_defines([0], 2, True, 4))
    try:
        res = STAR_RES.kernel_resources(path)
        for kernel in TEXT_RES.ONE:
            r = res[kernel]
            assert r["private_segment_fixed_size"] == 0, (kernel, r)
            assert r["vgpr_count"] + r["agpr_count"] <= 128, (kernel, r)
    finally:
        prog.release()
