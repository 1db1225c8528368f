"""
The row reader of the row-at-a-time kernels (csrc/devlib/strom_rowreader.h), HIP path vs CPU
oracle (needs an MI355X: -m gpu): every kernel that stands on it, over every chunk format, without
a row map and behind one.

One seeded chunk -- int2, int4, int8, float8 and numeric columns, NULLs in each; two tiles of the
largest row-at-a-time loop (16384 rows: the join's tile, the hashed scatter's) plus a ragged 37 --
is built as ROW, ROW_FLAT, TUPSLOT and COLUMN and sent through
  (a) gpuscan_qual_generic
  (b) gpuhashjoin_main against a dimension with duplicate keys (the emit pass reads rows again)
  (c) a dense GpuPreAgg session: gpupreagg_dense_generic, gpupreagg_census, gpupreagg_keyrange
  (d) a hashed session, table plan: gpupreagg_hash_check / _fold
  (e) the same with four hash roles (forced; COLUMN chunks take them, the other formats fold
      with one role whatever is asked): the roles' scan of the grouping columns or of the check
      pass's role map, and drain()
  (f) the partition plan: gpupreagg_hash_check_parts / _scatter_lds or _scatter / _fold_parts
and one COLUMN chunk with a text column through each operator's one-role path (text variables do
not go through the hash roles).

Bars as in the operators' own tests, whose comparisons these reuse: row sets, join records, group
keys, counts, integer sums and min / max bit-exact against the oracle; float8 sums relative 1e-12.
"""
import functools

import numpy as np
import pytest

import oracle_binding as oracle
import text_cases
from pg_strom_amd import kds
from pg_strom_amd.gpupreagg import GpuPreAgg
from test_gpuhashjoin_gpu import run_and_compare
from test_gpupreagg_gpu import assert_matches_oracle
from test_gpuscan_gpu import check

pytestmark = pytest.mark.gpu

NROWS = 2 * 16384 + 37
FORMATS = ("row", "row_flat", "tupslot", "column")
NKEY4, NKEY2 = 3000, 6

# reads every column
QUAL = ("(or (and (int2lt (var 1 int2) (const int2 4)) (int8gt (var 3 int8) (const int8 0)))"
        " (and (float8lt (var 4 float8) (const float8 30)) (int4gt (var 2 int4) (const int4 10)))"
        " (numeric_gt (var 5 numeric) (numeric (var 1 int2))))")
JOIN = "(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4) (qual %s)))" % QUAL
# the int8 sum has no static bound: the check passes and the dense row measure its inputs
AGG = ("(gpupreagg (qual (numeric_gt (var 5 numeric) (numeric (var 1 int2))))"
       " (key (var 2 int4)) (key (var 1 int2)) (nrows) (nrows (isnotnull (var 3 int8)))"
       " (psum (var 3 int8)) (pmin (var 3 int8)) (psum (var 4 float8)) (pmax (var 4 float8)))")
AGG_QUAL = "(numeric_gt (var 5 numeric) (numeric (var 1 int2)))"
TEXT_QUAL = "(and (text_lt (var 6 text) (const text 'm')) (int2lt (var 1 int2) (const int2 5)))"
TEXT_JOIN = "(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4) (qual %s)))" % TEXT_QUAL
TEXT_AGG = AGG.replace(AGG_QUAL, TEXT_QUAL)


@functools.lru_cache(maxsize=None)
def columns():
    rng = np.random.default_rng(20260)
    n = NROWS
    nulls = lambda: rng.random(n) < 0.04
    return (kds.Column("int2", rng.integers(0, NKEY2, n).astype(np.int16), nulls()),
            kds.Column("int4", rng.integers(0, NKEY4, n).astype(np.int32), nulls()),
            kds.Column("int8", rng.integers(-10**12, 10**12, n).astype(np.int64), nulls()),
            kds.Column("float8", rng.random(n) * 100, nulls()),
            kds.numeric_from_scaled(rng.integers(-300, 900, n), 2, nulls()))


@functools.lru_cache(maxsize=None)
def chunk(fmt):
    return kds.build_kds(fmt, list(columns()))


@functools.lru_cache(maxsize=None)
def text_chunk():
    rng = np.random.default_rng(20261)
    words = [text_cases.WORDS[i] for i in rng.integers(0, len(text_cases.WORDS), NROWS)]
    return kds.build_kds("column", list(columns()) + [kds.Column("text", words, rng.random(NROWS) < 0.04)])


@functools.lru_cache(maxsize=None)
def dimension():
    """every other key of the fact column, each three times"""
    pk = np.repeat(np.arange(0, NKEY4, 2, dtype=np.int32), 3)
    return kds.build_kds("row", [kds.Column("int4", pk), kds.Column("int4", np.arange(len(pk), dtype=np.int32))])


def row_map(mapped):
    """the odd rows, or none"""
    return np.arange(1, NROWS, 2, dtype=np.int32) if mapped else None


grid = pytest.mark.parametrize("fmt,mapped", [(f, m) for f in FORMATS for m in (False, True)])


@grid
def test_scan(fmt, mapped):
    res = check(QUAL, chunk(fmt), row_map=row_map(mapped))
    assert 0 < res.nitems < (NROWS // 2 if mapped else NROWS)


@grid
def test_join_general_kernel(fmt, mapped, monkeypatch):
    # the fast kernels take a COLUMN chunk without a row map when the keys are unique and the
    # program is a bare key comparison: neither holds here, and they are switched off as well
    monkeypatch.setenv("STROM_HASHJOIN_NO_FAST", "1")
    res, info = run_and_compare(JOIN, chunk(fmt), [dimension()], [[1]], row_map=row_map(mapped), ratio=3.0)
    assert not info[0]["unique"] and res.nitems > 0


@grid
def test_dense_session_fold_census_and_chunk_domain(fmt, mapped):
    buf, rmap = chunk(fmt), row_map(mapped)
    k2, k4 = columns()[0], columns()[1]
    rc, passed = oracle.gpuscan(AGG_QUAL, buf, [], row_map=rmap)
    assert rc == 0
    rows = np.abs(passed) - 1                                   # the rows the qual keeps
    agg = GpuPreAgg(AGG)
    # per key: min and max - min + 1 over the kept rows where the key is not NULL
    want = []
    for c in (k4, k2):
        v = c.values[rows][c.isnull[rows] == 0].astype(np.int64)
        want.append((int(v.min()), int(v.max() - v.min() + 1)))
    assert agg.chunk_domain(buf, row_map=rmap) == want
    agg.begin([(0, NKEY4), (0, NKEY2)])
    try:
        bitmap = agg.census(buf, row_map=rmap)
        dense = (np.where(k4.isnull != 0, NKEY4, k4.values.astype(np.int64))
                 + np.where(k2.isnull != 0, NKEY2, k2.values.astype(np.int64)) * (NKEY4 + 1))[rows]
        marked = np.zeros(len(bitmap) * 32, dtype=bool)
        marked[np.unique(dense)] = True
        assert np.array_equal(np.unpackbits(bitmap.view(np.uint8), bitorder="little").astype(bool), marked)
        assert agg.fold(buf, row_map=rmap)[0] == 0
        assert_matches_oracle(AGG, agg, [buf], agg.fetch(), row_maps=[rmap])
    finally:
        agg.end()


def hashed_fold(spec, buf, rmap, hint=0):
    agg = GpuPreAgg(spec).begin_hashed(ngroups_hint=hint)
    try:
        status, pfm = agg.fold(buf, row_map=rmap)
        assert status == 0
        assert_matches_oracle(spec, agg, [buf], agg.fetch(), row_maps=[rmap])
    finally:
        agg.end()
    return pfm


@grid
def test_hashed_session_table_plan(fmt, mapped):
    hashed_fold(AGG, chunk(fmt), row_map(mapped))


@pytest.fixture
def four_roles(monkeypatch):
    """the table plan with four hash roles, whatever the group count suggests"""
    monkeypatch.setenv("STROM_GPUPREAGG_HASH_ROLES", "4")
    monkeypatch.setenv("STROM_GPUPREAGG_HASH_NO_PARTS", "1")


@grid
def test_hashed_session_with_roles(four_roles, fmt, mapped):
    """COLUMN without a row map: the check pass leaves a role map (the hint says more groups than
    one LDS table takes), the roles scan that; behind a row map they scan the grouping columns.
    Only COLUMN chunks take roles: for the other three formats this is the table plan once more,
    with the request for roles that the host must not follow."""
    assert hashed_fold(AGG, chunk(fmt), row_map(mapped), hint=5000)["num_kern_prep"] == 0


def test_hashed_roles_scan_the_grouping_columns_without_a_role_map(four_roles, monkeypatch):
    monkeypatch.setenv("STROM_GPUPREAGG_HASH_NO_ROLEMAP", "1")
    assert hashed_fold(AGG, chunk("column"), None, hint=5000)["num_kern_prep"] == 0


@pytest.mark.parametrize("lds_scatter", [True, False])
@grid
def test_hashed_session_partition_plan(fmt, mapped, lds_scatter, monkeypatch):
    monkeypatch.setenv("STROM_GPUPREAGG_HASH_PARTS_MIN", "0")
    if not lds_scatter:
        monkeypatch.setenv("STROM_GPUPREAGG_HASH_NO_LDS_SCATTER", "1")
    assert hashed_fold(AGG, chunk(fmt), row_map(mapped))["num_kern_prep"] == 1


def test_text_variable_in_the_scan():
    check(TEXT_QUAL, text_chunk(), row_map=row_map(True))       # (a row map: not the streaming kernel)


def test_text_variable_in_the_join():
    run_and_compare(TEXT_JOIN, text_chunk(), [dimension()], [[1]], ratio=3.0)


def test_text_variable_in_the_aggregates():
    buf, rmap = text_chunk(), row_map(True)
    agg = GpuPreAgg(TEXT_AGG).begin([(0, NKEY4), (0, NKEY2)])
    try:
        assert agg.fold(buf, row_map=rmap)[0] == 0              # (a row map: not a streaming kernel)
        assert_matches_oracle(TEXT_AGG, agg, [buf], agg.fetch(), row_maps=[rmap])
    finally:
        agg.end()
    hashed_fold(TEXT_AGG, buf, None)                            # one role
    hashed_fold(TEXT_AGG, buf, rmap)
