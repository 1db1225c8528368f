"""
The snowflake lookup (strom_submit_gpupreagg_lookup_snowflake), the parts that need no GPU: the
symbols, the planning function that says which star a tree flattens to
(strom_gpupreagg_lookup_snowflake_roots), the compose kernel in a join program compiled for gfx950
as the runtime compiles it (no scratch memory), and the size of the kernel's control block.
"""
import ctypes
import importlib.util
import os
import re

import pytest

from pg_strom_amd import gpupreagg, runtime
from pg_strom_amd._lib import lib, PROTOTYPES
from pg_strom_amd.gpuhashjoin import codegen_gpuhashjoin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMREC_MAXCOLS = 16                             # HASHJOIN_DIMREC_MAXCOLS


def _resources_module():
    spec = importlib.util.spec_from_file_location(
        "_star_lookup_resources", os.path.join(ROOT, "scripts", "star_lookup_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_symbols_are_declared_and_resolve():
    header = open(os.path.join(ROOT, "include", "strom_hip.h")).read()
    for name in ("strom_submit_gpupreagg_lookup_snowflake", "strom_gpupreagg_lookup_snowflake_roots"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in PROTOTYPES and getattr(lib, name) is not None
    assert re.search(r"#define\s+STROM_LOOKUP_SNOWFLAKE_MAXRELS\s+8\b", header)


def test_a_chain_is_one_root():
    assert gpupreagg.lookup_snowflake_roots([0, 1, 2], [0, 1, 2, 3, 0]) == (1, [1, 1, 1], [0, 1, 1, 1, 0])


def test_a_bushy_tree_has_a_root_per_fact_column():
    """fact -> d1 -> {d2, d3} and fact -> d4: the columns of relations 2 and 3 land on root 1, those
    of relation 4 on root 2"""
    nroots, root_of, col_root = gpupreagg.lookup_snowflake_roots([0, 1, 1, 0], [2, 3, 4, 0, 1])
    assert nroots == 2
    assert root_of == [1, 1, 1, 2]
    assert col_root == [1, 1, 2, 0, 1]


def test_a_star_is_the_identity():
    assert gpupreagg.lookup_snowflake_roots([0, 0, 0, 0], [4, 3, 2, 1, 0]) == (4, [1, 2, 3, 4], [4, 3, 2, 1, 0])
    assert gpupreagg.lookup_snowflake_roots([0], [1, 0]) == (1, [1], [1, 0])


@pytest.mark.parametrize("parents, depths", [
    ([1], [0]),                                 # parent[0] = 1: the first relation hangs on itself
    ([0, 3, 0], [0]),                           # a forward reference
    ([0, 2], [0]),                              # ... on itself
    ([0, -1], [0]),                             # a negative parent
    ([0, 0, 0, 0, 0], [0]),                     # five roots
    ([0, 1, 2, 3, 4, 5, 6, 7, 8], [0]),         # nine relations
    ([], [0]),                                  # none
    ([0, 1], [0, 3]),                           # a column depth above ntbls
    ([0, 1], [-1]),
])
def test_refused_trees(parents, depths):
    with pytest.raises(ValueError):
        gpupreagg.lookup_snowflake_roots(parents, depths)


def test_eight_relations_under_four_roots_are_accepted():
    nroots, root_of, _ = gpupreagg.lookup_snowflake_roots([0, 1, 2, 0, 4, 0, 0, 7], [])
    assert nroots == 4 and root_of == [1, 1, 1, 2, 2, 3, 4, 4]


def test_compose_kernel_is_in_a_join_program_and_uses_no_scratch():
    """a join program compiled for gfx950 as the runtime compiles it (no device)"""
    res_mod = _resources_module()
    cg = codegen_gpuhashjoin("(gpuhashjoin (rel (hashkey (var 3 int4) 1 int4)))")
    cg = cg[0] if isinstance(cg, tuple) else cg
    prog = runtime.DevProgram(cg.source, cg.extra_flags).wait()
    try:
        path = os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)
        code = open(path, "rb").read()
        assert b"hashjoin_compose_dimrec_kernel.kd" in code
        r = res_mod.kernel_resources(path)["hashjoin_compose_dimrec_kernel"]
        print(r)
        assert r["private_segment_fixed_size"] == 0, r
        assert r["group_segment_fixed_size"] == 0, r      # no wave waits on another: nothing is shared
    finally:
        prog.release()


class ComposeColumn(ctypes.Structure):
    _fields_ = [("from_child", ctypes.c_uint32), ("attlen", ctypes.c_int32), ("src_offset", ctypes.c_uint32),
                ("src_nullbit", ctypes.c_uint32), ("offset", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class ComposeSpec(ctypes.Structure):
    """hashjoin_compose_spec of strom_ctl.h, field by field"""
    _fields_ = [("ncols", ctypes.c_uint32), ("reclen", ctypes.c_uint32), ("parent_reclen", ctypes.c_uint32),
                ("child_reclen", ctypes.c_uint32), ("link_attlen", ctypes.c_int32), ("link_offset", ctypes.c_uint32),
                ("link_nullbit", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("c", ComposeColumn * DIMREC_MAXCOLS)]


def test_control_block_matches_its_static_assert():
    text = open(os.path.join(ROOT, "pg_strom_amd", "csrc", "devlib", "strom_ctl.h")).read()
    assert re.search(r"#define\s+HASHJOIN_DIMREC_MAXCOLS\s+%d\b" % DIMREC_MAXCOLS, text)
    m = re.search(r"static_assert\(sizeof\(hashjoin_compose_spec\) == (\d+),", text)
    assert m and int(m.group(1)) == ctypes.sizeof(ComposeSpec)
    body = re.search(r"struct hashjoin_compose_spec \{(.*?)\n\};", text, re.S).group(1)
    names = re.findall(r"\bcl_u?int\s+(\w+);", body)
    assert names == ["ncols", "reclen", "parent_reclen", "child_reclen", "link_attlen", "link_offset",
                     "link_nullbit", "__pad", "from_child", "attlen", "src_offset", "src_nullbit", "offset", "__pad"]
