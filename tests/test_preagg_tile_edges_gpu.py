"""
The streaming dense-id kernels at the edges of their tile reader (needs an MI355X: -m gpu).

reg1 / priv / dense / packed _column and the lookup variants read a COLUMN chunk through ONE
tile reader (strom_gpupreagg.h, "dense kernels: shared pieces": GPUPREAGG_TILE_LOAD): a tile is block x 4 x quads
rows, a full tile takes the straight-line loaders (without the bitmap words when no column has
a NULL bitmap), the ragged last one checks every row.  What that reader can get wrong shows at
the smallest shapes: one row, a tile less one, exactly a tile, a tile and one, two tiles and a
bit, and a work-group that walks several tiles and ends on a ragged one -- each without and
with a NULL bitmap in the chunk, for every kernel family.

The bars are those of test_gpupreagg_gpu.py (compare_with_oracle): keys, counts, integer sums
and min / max bit-exact against the oracle's partial rows, float8 sums within 1e-12 relative.
"""
import os

import pytest

from pg_strom_amd import kds, runtime
from test_chain_gpu import lookup_aggregate_against_numpy
from test_gpupreagg_gpu import C4_SPEC, c4_table, compare_with_oracle

pytestmark = pytest.mark.gpu

# what a session reads its geometry from (gpupreagg.cpp: strom_gpupreagg_create, and the program's
# -D options): the LDS-atomic kernels run STROM_GPUPREAGG_BLOCK threads, the register / lane-private
# kernels GPUPREAGG_REG_BLOCK = 256; a thread holds STROM_GPUPREAGG_QUADS quads of 4 rows
# Nothing hands a session's block, quads or kernel family to Python (the library's interface has
# no such call), so the tile sizes below repeat the host's defaults (gpupreagg.cpp: block = 1024,
# quads = 2; GPUPREAGG_REG_BLOCK 256 in strom_gpupreagg.h): a change there has to be repeated here, or
# the row counts stop sitting on the tile edges.  Likewise the families are reached by construction
# (setup_layout: one group -> reg1; <= 32 groups and <= 32 bytes of accumulators -> priv; an image
# beyond the LDS budget -> id-range roles); only the packed path reports itself (num_kern_prep).
BLOCK = int(os.environ.get("STROM_GPUPREAGG_BLOCK", "1024"))
QUADS = int(os.environ.get("STROM_GPUPREAGG_QUADS", "2"))
TILE_ROWS = BLOCK * 4 * QUADS               # GPUPREAGG_TILE_ROWS
REG_TILE_ROWS = 256 * 4 * QUADS             # GPUPREAGG_REG_TILE_ROWS

ALL_KINDS = ("(nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)) (pmin (var 2 int4)) (pmax (var 2 int4))"
             " (pmin (var 3 float8)) (pmax (var 3 float8)))")
# no key: one group, register accumulators -- every kind of the wave fold's LDS update
REG1_SPEC = "(gpupreagg " + ALL_KINDS
# 28 bytes of accumulators per group: within what the lane-private kernel takes (32) for <= 32 groups
KEYED_SPEC = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 3 float8)) (pmin (var 2 int4)) (pmax (var 3 float8)))"

# family: (spec, groups, tile rows, environment, packed path expected when no column has a NULL bitmap)
FAMILIES = {
    "reg1": (REG1_SPEC, 0, REG_TILE_ROWS, {}, False),
    "priv": (KEYED_SPEC, 3, REG_TILE_ROWS, {}, False),
    "dense": (KEYED_SPEC, 300, TILE_ROWS, {}, False),
    "dense_roles": (KEYED_SPEC, 400, TILE_ROWS, {"STROM_GPUPREAGG_LDS_BUDGET": "6000"}, False),
    "packed": (C4_SPEC, 10000, TILE_ROWS, {}, True),
}


def fold_and_compare(family, nrows, nulls, monkeypatch):
    spec, ngroups, _, env, packs = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cols = c4_table(nrows, 1000 + nrows % 997, max(ngroups, 1), nulls=0.1 if nulls else None)
    if nulls:
        cols[1].isnull[0] = True            # (a chunk without a NULL has no bitmap: also at one row)
    pfms = []
    compare_with_oracle(spec, [kds.build_kds("column", cols)], [(0, ngroups)] if ngroups else [], pfms=pfms)
    # the host packs the accumulators at every one of these row counts (the fields only get narrower
    # with fewer rows) -- and never when an input column has a NULL bitmap: the 10000 groups then
    # take the standard image with id-range roles, which is checked all the same
    assert pfms[0]["num_kern_prep"] == (1 if packs and not nulls else 0)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("where", ["one_row", "tile_less_one", "tile", "tile_and_one", "two_tiles_and_three"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_row_counts_around_one_tile(family, where, nulls, monkeypatch):
    T = FAMILIES[family][2]
    nrows = {"one_row": 1, "tile_less_one": T - 1, "tile": T, "tile_and_one": T + 1,
             "two_tiles_and_three": 2 * T + 3}[where]
    fold_and_compare(family, nrows, nulls, monkeypatch)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_work_group_walks_several_tiles_and_ends_on_a_ragged_one(family, nulls, monkeypatch):
    """one work-group per CU: a split then has at most as many work-groups as the chip has CUs (fewer
    with id-range roles, which share them out), so 2 x CUs x T + 5 rows give every work-group at least
    two tiles, and the last tile of the chunk has five rows"""
    monkeypatch.setenv("STROM_GPUPREAGG_BLOCKS_PER_CU", "1")
    runtime.init()
    W = runtime.device_info()["compute_units"]
    fold_and_compare(family, 2 * W * FAMILIES[family][2] + 5, nulls, monkeypatch)


@pytest.mark.parametrize("fact_nulls", [False, True])
@pytest.mark.parametrize("nrows", [TILE_ROWS - 1, TILE_ROWS + 1])
def test_lookup_row_counts_around_one_tile(nrows, fact_nulls):
    """the lookup variant keeps its own loader ladder (the key column, the inner columns it skips) and
    shares the tile's row assembly: a tile less one row is all ragged, a tile and one row is one
    straight-line tile and a one-row tail through the software pipeline"""
    lookup_aggregate_against_numpy(nrows, 53, "int4", fact_nulls=fact_nulls)
