"""
Star join as lookups inside the aggregate's pass (strom_submit_gpupreagg_lookup_star /
gpupreagg_dense_lookup_star, gpupreagg_packed_lookup_star; needs an MI355X: -m gpu).

"fact JOIN dim1 JOIN dim2 ... GROUP BY": every relation is a table of its own (DIRECT index,
unique keys) probed by its own fact column; a row is folded only if EVERY relation has a partner.
The model is numpy over the joined rows, as test_chain_gpu.lookup_aggregate_against_numpy does it,
and the bars are that file's: keys, counts, integer sums and min / max bit-exact, float8 sums
within rtol 1e-12.
"""
import ctypes
import os

import numpy as np
import pytest

from pg_strom_amd import kds, runtime
from pg_strom_amd._lib import lib
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpupreagg import GpuPreAgg

pytestmark = pytest.mark.gpu

# (the session's geometry is read from the environment, as test_preagg_tile_edges_gpu.py does)
BLOCK = int(os.environ.get("STROM_GPUPREAGG_BLOCK", "1024"))
QUADS = int(os.environ.get("STROM_GPUPREAGG_QUADS", "2"))
TILE_ROWS = BLOCK * 4 * QUADS
MAXRELS = 4                                     # STROM_LOOKUP_STAR_MAXRELS
BAD_REQUEST = 101
CPU_RECHECK = 2
QUAL = "(and (int4lt (var 2 int4) (param 0 int4)) (float8gt (var 3 float8) (param 1 float8)))"
EXT = [np.int32(2**30), 0.25]
NULLKEY = 10**9                                 # stands for a NULL group key in the model


class Dim(object):
    """a dimension: unique keys with holes in their range, columns [(sqltype, values, isnull)]"""

    def __init__(self, rng, nd, keytype="int4", key_lo=0, holes=1.3):
        self.nd, self.keytype = nd, keytype
        self.span = int(nd * holes)
        self.key_lo = key_lo
        self.key = key_lo + rng.permutation(self.span)[:nd].astype(np.int64)
        self.cols = []

    def add(self, sqltype, values, isnull=None):
        self.cols.append((sqltype, values, isnull if isnull is not None else np.zeros(self.nd, dtype=bool)))
        return self

    def chunk(self, fmt="row_flat"):
        kdt = np.int32 if self.keytype == "int4" else np.int64
        cols = [kds.Column(self.keytype, self.key.astype(kdt))]
        for t, v, isn in self.cols:
            cols.append(kds.Column(t, v, isn if isn.any() else None))
        return kds.build_kds(fmt, cols)

    def partner(self, fkey, fnull):
        """row of this dimension per fact row, -1 without a partner"""
        pos = np.full(self.span, -1, dtype=np.int64)
        pos[self.key - self.key_lo] = np.arange(self.nd)
        off = fkey.astype(np.int64) - self.key_lo
        ok = (~fnull) & (off >= 0) & (off < self.span)
        return np.where(ok, pos[np.clip(off, 0, self.span - 1)], -1)

    def fact_keys(self, rng, n, nulls):
        """fact keys: inside the range (holes included), below and above it, NULLs"""
        kdt = np.int32 if self.keytype == "int4" else np.int64
        k = (self.key_lo + rng.integers(-40, self.span + 40, n)).astype(kdt)
        isn = (rng.random(n) < 0.02) if nulls else np.zeros(n, dtype=bool)
        return k, isn


def open_joins(dims, key_attnos):
    """one table per relation; its program names the fact column that joins it"""
    joins = []
    for d, attno in zip(dims, key_attnos):
        km = build_multihash([(d.chunk(), [1])])
        j = GpuHashJoin("(gpuhashjoin (rel (hashkey (var %d %s) 1 %s)))" % (attno, d.keytype, d.keytype)).begin(km)
        info = j.table_info(1)
        assert info["mode"] == "direct" and info["unique"]
        joins.append(j)
    return joins


def partial_rows(pr, nkeys):
    """partial rows sorted by their keys: (keys [n, nkeys] with NULLKEY for NULL, [(values, isnull)] per column)"""
    keys = np.stack([np.where(pr.column(k)[1], NULLKEY, pr.column(k)[0].astype(np.int64)) for k in range(nkeys)], axis=1)
    order = np.lexsort(keys.T[::-1])
    cols = [(pr.column(c)[0][order], pr.column(c)[1][order]) for c in range(nkeys, len(pr.targets))]
    return keys[order], cols


def model_groups(keycols):
    """keycols: [(values, isnull)] over the joined rows -> (unique key rows, inverse)"""
    keys = np.stack([np.where(isn, NULLKEY, v.astype(np.int64)) for v, isn in keycols], axis=1)
    if len(keys) == 0:                          # (one row, and the WHERE dropped it)
        return keys, np.zeros(0, dtype=np.int64)
    uk, inv = np.unique(keys, axis=0, return_inverse=True)
    return uk, inv.reshape(-1)


def check_count_and_sums(cols, inv, ngroups, a_sel, b_sel, times=1):
    """nrows, psum(int8(a)), psum(b): the first three aggregates of every spec here"""
    assert np.array_equal(cols[0][0], times * np.bincount(inv, minlength=ngroups))
    sums = np.zeros(ngroups, dtype=np.int64)
    np.add.at(sums, inv, a_sel.astype(np.int64))
    assert np.array_equal(cols[1][0], times * sums)
    assert np.allclose(cols[2][0], times * np.bincount(inv, weights=b_sel, minlength=ngroups), rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------
# two dimensions: the shape of cases 1, 3, 4
# ---------------------------------------------------------------------------------------------
TWO_SPEC = ("(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4)))"
            " (psum (var 3 float8)) (pmax (var 4 float8)))")
# var 1: dimension 1's group column; var 2, 3: fact columns 3, 4; var 4: dimension 2's float8 column
TWO_COLUMNS = [(1, 2, "int4"), (0, 3, "int4"), (0, 4, "float8"), (2, 2, "float8")]
_TWO_DIMS = {}


def two_dims(nd=3000, ngroups=53):
    """computed once, shared, left unchanged"""
    if (nd, ngroups) not in _TWO_DIMS:
        rng = np.random.default_rng(1201)
        d1 = Dim(rng, nd, key_lo=-700)
        d1.add("int4", (d1.key % ngroups).astype(np.int32), rng.random(nd) < 0.04)
        d2 = Dim(rng, nd, key_lo=100)
        d2.add("float8", rng.random(nd) * 10, rng.random(nd) < 0.05)       # 16-byte slot records
        _TWO_DIMS[(nd, ngroups)] = (d1, d2)
    return _TWO_DIMS[(nd, ngroups)]


def two_dimensions_against_numpy(n, fact_nulls=True, nchunks=1, classes=False, ngroups=53):
    runtime.init()
    d1, d2 = two_dims(ngroups=ngroups)
    rng = np.random.default_rng(7 + n)
    k1, k1n = d1.fact_keys(rng, n, fact_nulls)
    k2, k2n = d2.fact_keys(rng, n, fact_nulls)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    an = (rng.random(n) < 0.03) if fact_nulls else np.zeros(n, dtype=bool)
    b = rng.random(n)
    if fact_nulls and n >= 1:                   # (a chunk without a NULL has no bitmap: also at one row)
        an[0] = True
    fact = kds.build_kds("column", [kds.Column("int4", k1, k1n if fact_nulls else None),
                                    kds.Column("int4", k2, k2n if fact_nulls else None),
                                    kds.Column("int4", a, an if fact_nulls else None), kds.Column("float8", b)])
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d2], [1, 2])
    agg = GpuPreAgg(TWO_SPEC)
    try:
        agg.begin([(0, ngroups)], ext_params=EXT)
        for _ in range(nchunks):
            assert agg.collect(agg.submit_lookup_star(joins, ds, TWO_COLUMNS))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    p1, p2 = d1.partner(k1, k1n), d2.partner(k2, k2n)
    if classes:
        # the drop rule is only tested if every class of row occurs
        assert np.count_nonzero((p1 >= 0) & (p2 < 0)) > 0
        assert np.count_nonzero((p1 < 0) & (p2 >= 0)) > 0
        assert np.count_nonzero((p1 < 0) & (p2 < 0)) > 0
        assert np.count_nonzero((p1 >= 0) & (p2 >= 0)) > 0
        assert k1.min() < d1.key.min() and k1.max() > d1.key.max()
        assert k2.min() < d2.key.min() and k2.max() > d2.key.max()
    sel = np.flatnonzero((p1 >= 0) & (p2 >= 0) & (~an) & (a < EXT[0]) & (b > EXT[1]))
    i1, i2 = p1[sel], p2[sel]
    uk, inv = model_groups([(d1.cols[0][1][i1], d1.cols[0][2][i1])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), a[sel], b[sel], times=nchunks)
    wmax = np.full(len(uk), -np.inf)
    ok = ~d2.cols[0][2][i2]
    np.maximum.at(wmax, inv[ok], d2.cols[0][1][i2][ok])
    assert np.array_equal(cols[3][1], np.isinf(wmax))
    assert np.array_equal(cols[3][0][~np.isinf(wmax)], wmax[~np.isinf(wmax)])


def test_two_dimensions_with_holes_nulls_and_keys_outside_both_tables():
    """case 1: GROUP BY an int4 column of dimension 1 that has NULLs; nrows, psum of an outer int4
    and an outer float8, pmax of a float8 column of dimension 2 (16-byte record) that has NULLs;
    two chunks into one session; all four partner classes occur"""
    two_dimensions_against_numpy(60011, nchunks=2, classes=True)


@pytest.mark.parametrize("fact_nulls", [False, True])
@pytest.mark.parametrize("nrows", [1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 3])
def test_two_dimensions_around_one_tile(nrows, fact_nulls):
    """case 3: one row, a tile less one (all ragged), a tile (the straight-line loaders, bitmap-free
    without NULL bitmaps), a tile and one, two tiles and three"""
    two_dimensions_against_numpy(nrows, fact_nulls=fact_nulls)


def test_a_work_group_walks_several_tiles_and_ends_on_a_ragged_one(monkeypatch):
    """case 4: one work-group per CU and 2 x CUs x T + 5 rows: every work-group folds at least two
    tiles and the chunk's last tile has five rows"""
    monkeypatch.setenv("STROM_GPUPREAGG_BLOCKS_PER_CU", "1")
    runtime.init()
    W = runtime.device_info()["compute_units"]
    two_dimensions_against_numpy(2 * W * TILE_ROWS + 5)


# ---------------------------------------------------------------------------------------------
# case 2: the fixture's shape
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrow", [True, False])
def test_four_dimensions_one_keyed_by_int8(narrow, monkeypatch):
    """t0(aid, bid, cid, did, ...) against four 2000-row dimensions, the third keyed by int8; GROUP
    BY a column of dimension 1 and one of dimension 3 (a two-key dense domain); the WHERE reads
    dimension 2, pmin a column of dimension 4: every relation serves one integer column, so all
    records are narrow -- and 8 bytes each, 32 in all, with STROM_HASHJOIN_NO_NARROW_RECS"""
    if not narrow:
        monkeypatch.setenv("STROM_HASHJOIN_NO_NARROW_RECS", "1")
    runtime.init()
    n, nd = 50021, 2000
    rng = np.random.default_rng(1303)
    dims = [Dim(rng, nd, keytype=("int8" if r == 2 else "int4"), key_lo=(2**33 if r == 2 else 10 * r), holes=1.15)
            for r in range(MAXRELS)]
    dims[0].add("int4", (dims[0].key % 7).astype(np.int32), rng.random(nd) < 0.03)
    dims[1].add("int4", rng.integers(-5, 6, nd).astype(np.int32), rng.random(nd) < 0.03)
    dims[2].add("int4", ((dims[2].key - 2**33) % 5 - 2).astype(np.int32))
    dims[3].add("int4", rng.integers(-1000, 1000, nd).astype(np.int32), rng.random(nd) < 0.05)
    fk = [d.fact_keys(rng, n, True) for d in dims]
    a = rng.integers(-10**6, 10**6, n).astype(np.int32)
    b = rng.random(n)
    fact = kds.build_kds("column", [kds.Column(d.keytype, k, kn) for d, (k, kn) in zip(dims, fk)] +
                         [kds.Column("int4", a), kds.Column("float8", b)])
    spec = ("(gpupreagg (qual (int4gt (var 5 int4) (const int4 -4))) (key (var 1 int4)) (key (var 4 int4))"
            " (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)) (pmin (var 6 int4)))")
    columns = [(1, 2, "int4"), (0, 5, "int4"), (0, 6, "float8"), (3, 2, "int4"), (2, 2, "int4"), (4, 2, "int4")]
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins(dims, [1, 2, 3, 4])
    agg = GpuPreAgg(spec)
    try:
        agg.begin([(0, 7), (-2, 5)])
        assert agg.collect(agg.submit_lookup_star(joins, ds, columns))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    p = [d.partner(k, kn) for d, (k, kn) in zip(dims, fk)]
    alive = np.logical_and.reduce([x >= 0 for x in p])
    assert 0 < np.count_nonzero(alive) < n
    for r in range(MAXRELS):                    # every relation alone drops rows the others would keep
        others = np.logical_and.reduce([p[q] >= 0 for q in range(MAXRELS) if q != r])
        assert np.count_nonzero(others & (p[r] < 0)) > 0
    q2 = dims[1].cols[0]
    i2 = np.clip(p[1], 0, nd - 1)
    sel = np.flatnonzero(alive & ~q2[2][i2] & (q2[1][i2] > -4))
    i1, i3, i4 = p[0][sel], p[2][sel], p[3][sel]
    uk, inv = model_groups([(dims[0].cols[0][1][i1], dims[0].cols[0][2][i1]),
                            (dims[2].cols[0][1][i3], dims[2].cols[0][2][i3])])
    keys, cols = partial_rows(pr, 2)
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), a[sel], b[sel])
    wmin = np.full(len(uk), 2**40, dtype=np.int64)
    ok = ~dims[3].cols[0][2][i4]
    np.minimum.at(wmin, inv[ok], dims[3].cols[0][1][i4][ok].astype(np.int64))
    assert np.array_equal(cols[3][1], wmin == 2**40)
    assert np.array_equal(cols[3][0][wmin != 2**40].astype(np.int64), wmin[wmin != 2**40])


# ---------------------------------------------------------------------------------------------
# case 5: packed accumulators
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrow", [True, False])
def test_two_dimensions_with_packed_accumulators(narrow, monkeypatch):
    """1e4 groups, summed OUTER columns without NULLs: the packed LDS image
    (gpupreagg_packed_lookup_star; num_kern_prep reports it); the group key is a column of
    dimension 1 with NULLs, the WHERE also reads a column of dimension 2"""
    if not narrow:
        monkeypatch.setenv("STROM_HASHJOIN_NO_NARROW_RECS", "1")
    runtime.init()
    n, ngroups = 300007, 10000
    rng = np.random.default_rng(1409)
    d1 = Dim(rng, 40000, holes=1.25)
    d1.add("int4", (d1.key % ngroups).astype(np.int32), rng.random(d1.nd) < 0.02)
    d2 = Dim(rng, 3000, key_lo=50, holes=1.25)
    d2.add("int4", rng.integers(0, 10, d2.nd).astype(np.int32), rng.random(d2.nd) < 0.03)
    k1 = rng.integers(0, d1.span, n).astype(np.int32)
    k2 = (50 + rng.integers(0, d2.span, n)).astype(np.int32)
    a = rng.integers(-5 * 10**5, 2**20, n).astype(np.int32)
    b = rng.random(n)
    none = np.zeros(n, dtype=bool)
    fact = kds.build_kds("column", [kds.Column("int4", k1), kds.Column("int4", k2), kds.Column("int4", a),
                                    kds.Column("float8", b)])
    ext = [np.int32(2**19), 0.25]
    spec = ("(gpupreagg (qual (and " + QUAL + " (int4gt (var 4 int4) (const int4 1)))) (key (var 1 int4)) (nrows)"
            " (psum (int8 (var 2 int4))) (psum (var 3 float8)))")
    columns = [(1, 2, "int4"), (0, 3, "int4"), (0, 4, "float8"), (2, 2, "int4")]
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d2], [1, 2])
    agg = GpuPreAgg(spec)
    try:
        agg.begin([(0, ngroups)], ext_params=ext)
        pfms = []
        for _ in range(2):
            st, pfm = agg.collect(agg.submit_lookup_star(joins, ds, columns))
            assert st == 0
            pfms.append(pfm)
        pr = agg.fetch()
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    assert all(p["num_kern_prep"] == 1 for p in pfms)             # the packed path was taken
    p1, p2 = d1.partner(k1, none), d2.partner(k2, none)
    i2 = np.clip(p2, 0, d2.nd - 1)
    sel = np.flatnonzero((p1 >= 0) & (p2 >= 0) & (a < ext[0]) & (b > ext[1]) &
                         ~d2.cols[0][2][i2] & (d2.cols[0][1][i2] > 1))
    assert 0 < len(sel) < np.count_nonzero(p1 >= 0)
    i1 = p1[sel]
    uk, inv = model_groups([(d1.cols[0][1][i1], d1.cols[0][2][i1])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), a[sel], b[sel], times=2)


# ---------------------------------------------------------------------------------------------
# case 6: the qual
# ---------------------------------------------------------------------------------------------
OVERFLOW_QUAL = "(int4gt (int4pl (var 2 int4) (const int4 2147483000)) (const int4 0))"


@pytest.mark.parametrize("where", ["inner_of_relation_2", "outer_only"])
def test_the_qual_after_the_probes_and_before_them(where):
    runtime.init()
    n = 20011
    d1, d2 = two_dims()
    rng = np.random.default_rng(1511)
    k1, k1n = d1.fact_keys(rng, n, True)
    k2, k2n = d2.fact_keys(rng, n, True)
    a = rng.integers(-1000, 1000, n).astype(np.int32)
    b = rng.random(n)
    fact = kds.build_kds("column", [kds.Column("int4", k1, k1n), kds.Column("int4", k2, k2n),
                                    kds.Column("int4", a), kds.Column("float8", b)])
    qual = ("(float8gt (var 4 float8) (const float8 5.0))" if where == "inner_of_relation_2"
            else "(int4gt (var 2 int4) (const int4 -300))")
    spec = ("(gpupreagg (qual " + qual + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4)))"
            " (psum (var 3 float8)) (pmax (var 4 float8)))")
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d2], [1, 2])
    agg = GpuPreAgg(spec)
    try:
        agg.begin([(0, 53)])
        assert agg.collect(agg.submit_lookup_star(joins, ds, TWO_COLUMNS))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    p1, p2 = d1.partner(k1, k1n), d2.partner(k2, k2n)
    i2c = np.clip(p2, 0, d2.nd - 1)
    if where == "inner_of_relation_2":
        passes = ~d2.cols[0][2][i2c] & (d2.cols[0][1][i2c] > 5.0)
    else:
        passes = a > -300
    sel = np.flatnonzero((p1 >= 0) & (p2 >= 0) & passes)
    assert 0 < len(sel) < np.count_nonzero((p1 >= 0) & (p2 >= 0))
    i1, i2 = p1[sel], p2[sel]
    uk, inv = model_groups([(d1.cols[0][1][i1], d1.cols[0][2][i1])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), a[sel], b[sel])
    wmax = np.full(len(uk), -np.inf)
    ok = ~d2.cols[0][2][i2]
    np.maximum.at(wmax, inv[ok], d2.cols[0][1][i2][ok])
    assert np.array_equal(cols[3][1], np.isinf(wmax))
    assert np.array_equal(cols[3][0][~np.isinf(wmax)], wmax[~np.isinf(wmax)])


@pytest.mark.parametrize("partner_in_2", [True, False])
def test_an_error_in_an_outer_only_qual_needs_a_partner_in_every_relation(partner_in_2):
    """an int4 overflow in the qual-first: CpuReCheck when the row has partners in both relations,
    nothing (status 0, the row dropped) when relation 2 has none"""
    runtime.init()
    n = 9001
    d1, d2 = two_dims()
    rng = np.random.default_rng(1613)
    k1 = d1.key[rng.integers(0, d1.nd, n)].astype(np.int32)
    k2 = d2.key[rng.integers(0, d2.nd, n)].astype(np.int32)
    a = rng.integers(-500, 500, n).astype(np.int32)
    b = rng.random(n)
    bad = 4321
    a[bad] = 1000                                # 1000 + 2147483000 leaves int4
    if not partner_in_2:
        hole = np.setdiff1d(np.arange(d2.key_lo, d2.key_lo + d2.span), d2.key)[0]
        k2[bad] = hole
    fact = kds.build_kds("column", [kds.Column("int4", k1), kds.Column("int4", k2), kds.Column("int4", a),
                                    kds.Column("float8", b)])
    spec = ("(gpupreagg (qual " + OVERFLOW_QUAL + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4)))"
            " (psum (var 3 float8)) (pmax (var 4 float8)))")
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d2], [1, 2])
    agg = GpuPreAgg(spec)
    try:
        agg.begin([(0, 53)])
        st = agg.collect(agg.submit_lookup_star(joins, ds, TWO_COLUMNS))[0]
        pr = agg.fetch() if st == 0 else None
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    if partner_in_2:
        assert st == CPU_RECHECK
        return
    assert st == 0
    none = np.zeros(n, dtype=bool)
    p1, p2 = d1.partner(k1, none), d2.partner(k2, none)
    assert p1[bad] >= 0 and p2[bad] < 0
    sel = np.flatnonzero((p1 >= 0) & (p2 >= 0))      # (every other row passes: a + 2147483000 > 0)
    assert len(sel) == n - 1
    uk, inv = model_groups([(d1.cols[0][1][p1[sel]], d1.cols[0][2][p1[sel]])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), a[sel], b[sel])


# ---------------------------------------------------------------------------------------------
# case 7: one relation is the one-table call
# ---------------------------------------------------------------------------------------------
def test_one_relation_gives_the_partial_rows_of_submit_lookup():
    runtime.init()
    n = 30011
    d1, _ = two_dims()
    rng = np.random.default_rng(1709)
    k1, k1n = d1.fact_keys(rng, n, True)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    b = rng.random(n)
    fact = kds.build_kds("column", [kds.Column("int4", k1, k1n), kds.Column("int4", a), kds.Column("float8", b)])
    spec = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))"
    columns = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8")]
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1], [1])
    got = []
    try:
        for star in (True, False):
            agg = GpuPreAgg(spec)
            try:
                agg.begin([(0, 53)], ext_params=EXT)
                pending = (agg.submit_lookup_star(joins, ds, columns) if star
                           else agg.submit_lookup(joins[0], ds, columns))
                assert agg.collect(pending)[0] == 0
                got.append(partial_rows(agg.fetch(), 1))
            finally:
                agg.end()
    finally:
        joins[0].end()
        ds.release()
    (ks, cs), (kl, cl) = got
    assert len(ks) > 1 and np.array_equal(ks, kl)
    for (v1, n1), (v2, n2) in zip(cs, cl):
        assert not n1.any() and not n2.any()
    assert np.array_equal(cs[0][0], cl[0][0])                          # nrows
    assert np.array_equal(cs[1][0], cl[1][0])                          # integer sum
    # (a float8 sum is added up by LDS atomics in the order the waves arrive: two runs of the SAME
    # kernel differ in the last bits, so the bar is the file's 1e-12, not equal bits)
    assert np.allclose(cs[2][0], cl[2][0], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------
# case 8: the same query through what exists without the star call
# ---------------------------------------------------------------------------------------------
def test_same_answer_as_the_general_join_the_column_projection_and_a_plain_fold():
    runtime.init()
    n = 50021
    d1, d2 = two_dims()
    rng = np.random.default_rng(1811)
    k1, k1n = d1.fact_keys(rng, n, True)
    k2, k2n = d2.fact_keys(rng, n, True)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    an = rng.random(n) < 0.03
    b = rng.random(n)
    fact = kds.build_kds("column", [kds.Column("int4", k1, k1n), kds.Column("int4", k2, k2n),
                                    kds.Column("int4", a, an), kds.Column("float8", b)])
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d2], [1, 2])
    both = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)) (rel (hashkey (var 2 int4) 1 int4)))")
    both.begin(build_multihash([(d1.chunk(), [1]), (d2.chunk(), [1])]))
    got = []
    try:
        star = GpuPreAgg(TWO_SPEC)
        try:
            star.begin([(0, 53)], ext_params=EXT)
            assert star.collect(star.submit_lookup_star(joins, ds, TWO_COLUMNS))[0] == 0
            got.append(partial_rows(star.fetch(), 1))
        finally:
            star.end()
        joined, nitems = both.join_to_column(ds, TWO_COLUMNS)
        plain = GpuPreAgg(TWO_SPEC)
        try:
            plain.begin([(0, 53)], ext_params=EXT)
            assert plain.fold(joined)[0] == 0
            got.append(partial_rows(plain.fetch(), 1))
        finally:
            plain.end()
            joined.release()
    finally:
        both.end()
        for j in joins:
            j.end()
        ds.release()
    assert nitems == np.count_nonzero((d1.partner(k1, k1n) >= 0) & (d2.partner(k2, k2n) >= 0))
    (ks, cs), (kp, cp) = got
    assert len(ks) > 1 and np.array_equal(ks, kp)
    assert np.array_equal(cs[0][0], cp[0][0])                          # nrows
    assert np.array_equal(cs[1][0], cp[1][0])                          # integer sum
    assert np.allclose(cs[2][0], cp[2][0], rtol=1e-12, atol=0)         # float8 sum
    assert np.array_equal(cs[3][1], cp[3][1])                          # pmax: NULLs and values
    assert np.array_equal(cs[3][0][~cs[3][1]], cp[3][0][~cp[3][1]])


# ---------------------------------------------------------------------------------------------
# case 9: refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_session_usable():
    runtime.init()
    n = 5003
    d1, d2 = two_dims()
    rng = np.random.default_rng(1913)
    k1, k1n = d1.fact_keys(rng, n, True)
    k2, k2n = d2.fact_keys(rng, n, True)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    b = rng.random(n)
    k5 = rng.integers(0, 100, n).astype(np.int16)
    fact = kds.build_kds("column", [kds.Column("int4", k1, k1n), kds.Column("int4", k2, k2n),
                                    kds.Column("int4", a), kds.Column("float8", b), kds.Column("int2", k5)])
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d2], [1, 2])
    others = []

    def table(spec, dims_and_keys, fmt="row_flat"):
        j = GpuHashJoin(spec).begin(build_multihash([(d.chunk(fmt), keys) for d, keys in dims_and_keys]))
        others.append(j)
        return j

    # dimensions that fail the lookup's requirements
    dup = Dim(rng, 500)
    dup.key[:50] = dup.key[50:100]                                  # duplicate keys
    dup.add("int4", np.arange(500, dtype=np.int32))
    wide = Dim(rng, 500, key_lo=100)                                # two float8 columns: a 32-byte record
    wide.add("float8", rng.random(500)).add("float8", rng.random(500))
    f16 = [Dim(rng, 500, key_lo=100).add("float8", rng.random(500)) for _ in range(3)]      # 3 x 16 bytes
    small = Dim(rng, 80, keytype="int4", key_lo=0)
    small.add("int4", np.arange(80, dtype=np.int32))
    j_dup = table("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))", [(dup, [1])])
    j_qual = table("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4) (qual (int4lt (var 3 int4) (const int4 5)))))",
                   [(d2, [1])])
    j_two = table("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)) (rel (hashkey (var 2 int4) 1 int4)))",
                  [(d1, [1]), (d2, [1])])
    j_wide = table("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))", [(wide, [1])])
    j_f16 = [table("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))", [(d, [1])]) for d in f16]
    small2 = Dim(rng, 80, keytype="int2", key_lo=0)
    small2.cols = small.cols
    small2.chunk = lambda fmt="row_flat": kds.build_kds(fmt, [kds.Column("int2", small.key.astype(np.int16)),
                                                              kds.Column("int4", small.cols[0][1])])
    j_int2 = table("(gpuhashjoin (rel (hashkey (var 5 int2) 1 int2)))", [(small2, [1])])
    assert not j_dup.table_info(1)["unique"]

    agg = GpuPreAgg(TWO_SPEC).begin([(0, 53)], ext_params=EXT)
    hashed = GpuPreAgg(TWO_SPEC).begin_hashed(ext_params=EXT)
    text = GpuPreAgg("(gpupreagg (qual (texteq (var 5 text) (const text \"x\"))) (key (var 1 int4)) (nrows))")
    text.begin([(0, 53)])                                           # a program with a varlena variable
    # a session without a domain: the C call with no domain (the first chunk would fix it)
    err = ctypes.c_int(0)
    pb = ctypes.create_string_buffer(agg.parambuf, len(agg.parambuf))
    nodomain = lib.strom_gpupreagg_create(agg.program.key, agg.codegen._targets_c, len(agg.targets), pb,
                                          None, 0, ctypes.byref(err))
    assert nodomain

    def refused(session_owner, tbls, columns, session=None):
        saved = session_owner.session
        if session is not None:
            session_owner.session = session
        try:
            with pytest.raises(runtime.StromError) as ei:
                session_owner.submit_lookup_star(tbls, ds, columns)
            assert ei.value.errcode == BAD_REQUEST, ei.value
        finally:
            session_owner.session = saved

    try:
        refused(agg, [], TWO_COLUMNS)                                       # ntbls outside 1 .. MAXRELS
        refused(agg, joins + joins + [joins[0]], TWO_COLUMNS)
        refused(agg, joins, [(3, 2, "int4")] + TWO_COLUMNS[1:])             # a depth outside 0 .. ntbls
        refused(agg, joins, [(-1, 2, "int4")] + TWO_COLUMNS[1:])
        refused(agg, [joins[0], j_dup], TWO_COLUMNS[:3] + [(2, 2, "int4")])  # duplicate keys
        refused(agg, [joins[0], j_qual], TWO_COLUMNS)                       # a WHERE pulled up into the join program
        refused(agg, [joins[0], j_two], TWO_COLUMNS)                        # a table of two relations
        refused(agg, [joins[0], j_int2], TWO_COLUMNS[:3] + [(2, 2, "int4")])  # a 2-byte key
        refused(hashed, joins, TWO_COLUMNS)                                 # a hashed session
        refused(agg, joins, TWO_COLUMNS, session=nodomain)                  # a session without a domain
        refused(text, joins, [(1, 2, "int4"), (0, 3, "int4"), (0, 4, "float8"), (2, 2, "float8"), (0, 5, "int2")])
        # a 32-byte record; and 16 + 16 + 16 bytes over three relations
        refused(agg, [joins[0], j_wide], TWO_COLUMNS + [(2, 3, "float8")])
        refused(agg, j_f16, [(1, 2, "float8"), (0, 3, "int4"), (0, 4, "float8"), (2, 2, "float8"), (3, 2, "float8")])
        # nothing was folded (the counts below would show it), and the session still works
        assert agg.collect(agg.submit_lookup_star(joins, ds, TWO_COLUMNS))[0] == 0
        pr = agg.fetch()
    finally:
        lib.strom_gpupreagg_release(nodomain)
        agg.end()
        hashed.end()
        text.end()
        for j in joins + others:
            j.end()
        ds.release()
    p1, p2 = d1.partner(k1, k1n), d2.partner(k2, k2n)
    sel = np.flatnonzero((p1 >= 0) & (p2 >= 0) & (a < EXT[0]) & (b > EXT[1]))
    uk, inv = model_groups([(d1.cols[0][1][p1[sel]], d1.cols[0][2][p1[sel]])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), a[sel], b[sel])


# ---------------------------------------------------------------------------------------------
# integer sums the range proof does not cover: the mapping's own checked program
# ---------------------------------------------------------------------------------------------
def test_a_chunk_whose_integer_sums_are_unproven_is_folded_by_the_checked_star_program():
    """int8 inputs near 2^56 over a few thousand rows: rows x 2^bits passes 2^63, so the merge cannot
    prove that the chunk's sums stay in int8 and the chunk is folded again by the program built with
    GPUPREAGG_CHECKED -- for a star request the MAPPING's program (the session's own checked program
    has no star kernel).  The signs alternate, the sums fit: status 0 and exact totals."""
    runtime.init()
    n = 6007
    d1, d2 = two_dims()
    rng = np.random.default_rng(2017)
    k1, k1n = d1.fact_keys(rng, n, True)
    k2, k2n = d2.fact_keys(rng, n, True)
    x = (rng.integers(2**55, 2**56, n) * np.where(np.arange(n) % 2 == 0, 1, -1)).astype(np.int64)
    fact = kds.build_kds("column", [kds.Column("int4", k1, k1n), kds.Column("int4", k2, k2n), kds.Column("int8", x)])
    spec = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)) (pmax (var 3 float8)))"
    columns = [(1, 2, "int4"), (0, 3, "int8"), (2, 2, "float8")]
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d2], [1, 2])
    agg = GpuPreAgg(spec)
    try:
        agg.begin([(0, 53)])
        st = agg.collect(agg.submit_lookup_star(joins, ds, columns))[0]
        checked = agg.checked_folds()
        pr = agg.fetch()
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    assert st == 0 and checked >= 1
    p1, p2 = d1.partner(k1, k1n), d2.partner(k2, k2n)
    sel = np.flatnonzero((p1 >= 0) & (p2 >= 0))
    uk, inv = model_groups([(d1.cols[0][1][p1[sel]], d1.cols[0][2][p1[sel]])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    assert np.array_equal(cols[0][0], np.bincount(inv, minlength=len(uk)))
    want = [0] * len(uk)
    for g, v in zip(inv, x[sel]):
        want[g] += int(v)
    assert all(-2**63 <= w < 2**63 for w in want)
    assert [int(v) for v in cols[1][0]] == want
