"""
Snowflake joins flattened into slot records (strom_submit_gpupreagg_lookup_snowflake /
hashjoin_compose_dimrec_kernel; needs an MI355X: -m gpu).

A relation may be keyed by ANOTHER relation's column: the dimensions are joined to each other once,
into the root tables' slot records, and the fold is the one-table lookup (one root) or the star
(2 .. 4 roots).  The model is numpy over the joined rows; where said, the same query also runs as
the plan that exists without this call -- the multi-relation general join with an (ivar ..) key, the
COLUMN projection and a plain fold.  The bars are test_star_lookup_gpu.py's: keys, counts, integer
sums and min / max bit-exact, float8 sums within rtol 1e-12.
"""
import ctypes

import numpy as np
import pytest

from pg_strom_amd import kds, runtime
from pg_strom_amd._lib import lib
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpupreagg import GpuPreAgg
from test_star_lookup_gpu import (BAD_REQUEST, EXT, QUAL, TILE_ROWS, Dim, model_groups, open_joins, partial_rows)

pytestmark = pytest.mark.gpu

CORRUPTION = 300                                # StromError_DataStoreCorruption
AGGS = " (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"
# var 1: the group key; var 2, 3: the fact's summed columns (fact columns 3 and 4); var 4: one more inner column
SPEC_FMAX = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4))" + AGGS + " (pmax (var 4 float8)))"
SPEC_IMIN = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4))" + AGGS + " (pmin (var 4 int4)))"
SPEC_TWOKEYS = "(gpupreagg (key (var 1 int4)) (key (var 4 int4))" + AGGS + ")"
SPEC_BUSHY = ("(gpupreagg (qual (and " + QUAL + " (int4gt (var 5 int4) (const int4 1)))) (key (var 1 int4))" + AGGS +
              " (pmax (var 4 float8)))")
SPEC_PACKED = "(gpupreagg (qual (and " + QUAL + " (int4gt (var 4 int4) (const int4 1)))) (key (var 1 int4))" + AGGS + ")"
SPEC_CHECKED = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)) (pmax (var 3 float8)))"
FACT = [(0, 3, "int4"), (0, 4, "float8")]       # var 2, var 3 of every mapping here


class Tree(object):
    """dims[d - 1] is relation d; parents[d - 1] is 0 (keyed by fact column attnos[d - 1]) or p (keyed by
    column attnos[d - 1] of relation p, a column of the child's key type)"""

    def __init__(self, dims, parents, attnos):
        self.dims, self.parents, self.attnos = dims, parents, attnos
        self.link_types = [(d.keytype if p else None) for d, p in zip(dims, parents)]

    def open(self):
        return open_joins(self.dims, self.attnos)

    def general_join(self):
        """the same tree as ONE multi-relation join"""
        rels = ["(rel (hashkey (%s %d %s) 1 %s))" % ("ivar %d" % p if p else "var", a, d.keytype, d.keytype)
                for d, p, a in zip(self.dims, self.parents, self.attnos)]
        join = GpuHashJoin("(gpuhashjoin " + " ".join(rels) + ")")
        return join.begin(build_multihash([(d.chunk(), [1]) for d in self.dims]))

    def partners(self, fact_keys):
        """per relation the row that joins each fact row, -1 where the row has none there (or further up);
        fact_keys {fact attno: (values, isnull)}"""
        p = []
        for dim, par, attno in zip(self.dims, self.parents, self.attnos):
            if par == 0:
                k, kn = fact_keys[attno]
            else:
                k, kn = self.column(p, par, attno)
            p.append(dim.partner(k, kn))
        return p

    def column(self, p, depth, attno):
        """(values, isnull) of a relation's column over the fact rows; NULL where the row has no partner"""
        dim, rows = self.dims[depth - 1], p[depth - 1]
        idx = np.clip(rows, 0, dim.nd - 1)
        if attno == 1:
            return dim.key[idx], rows < 0
        _, v, isn = dim.cols[attno - 2]
        return v[idx], isn[idx] | (rows < 0)


def link_values(rng, parent, child, nulls=0.03):
    """values of a parent's link column: inside the child's range (its holes included), below it and
    above it, and NULLs"""
    v, _ = child.fact_keys(rng, parent.nd, False)
    return v, rng.random(parent.nd) < nulls


def make_fact(rng, n, roots, nulls=True, a_lo=0, a_hi=2**31):
    """fact(k1, k2, a, b): keys for up to two roots (k2 random where there is one), the summed columns"""
    keys = [r.fact_keys(rng, n, nulls) for r in roots]
    while len(keys) < 2:
        keys.append((rng.integers(0, 1000, n).astype(np.int32), np.zeros(n, dtype=bool)))
    a = rng.integers(a_lo, a_hi, n, dtype=np.int64).astype(np.int32)
    an = (rng.random(n) < 0.03) if nulls else np.zeros(n, dtype=bool)
    if nulls and n >= 1:
        an[0] = True
    b = rng.random(n)
    keytypes = [r.keytype for r in roots] + ["int4"]
    cols = [kds.Column(t, k, kn if nulls else None) for t, (k, kn) in zip(keytypes, keys)]
    cols += [kds.Column("int4", a, an if nulls else None), kds.Column("float8", b)]
    return kds.build_kds("column", cols), {1: keys[0], 2: keys[1]}, a, an, b


def fold(spec, domain, ext, submit, nchunks=1):
    """a fresh session, 'submit(agg)' nchunks times -> (statuses, perfmons, partial rows, checked folds)"""
    agg = GpuPreAgg(spec)
    try:
        agg.begin(domain, ext_params=ext)
        got = [agg.collect(submit(agg)) for _ in range(nchunks)]
        checked = agg.checked_folds()
        pr = agg.fetch()
    finally:
        agg.end()
    return [g[0] for g in got], [g[1] for g in got], pr, checked


def snowflake_rows(spec, domain, ext, tree, joins, ds, columns, nchunks=1):
    st, pfm, pr, _ = fold(spec, domain, ext,
                          lambda agg: agg.submit_lookup_snowflake(joins, tree.parents, ds, columns, tree.link_types), nchunks)
    assert st == [0] * nchunks
    return pr, pfm


def general_join_rows(spec, domain, ext, tree, ds, columns):
    both = tree.general_join()
    try:
        joined, nitems = both.join_to_column(ds, columns)
        try:
            st, _, pr, _ = fold(spec, domain, ext, lambda agg: agg.submit(joined))
        finally:
            joined.release()
    finally:
        both.end()
    assert st == [0]
    return pr, nitems


def same_rows(pr1, pr2, nkeys, float_sums=(2,)):
    (k1, c1), (k2, c2) = partial_rows(pr1, nkeys), partial_rows(pr2, nkeys)
    assert np.array_equal(k1, k2)
    for i, ((v1, n1), (v2, n2)) in enumerate(zip(c1, c2)):
        assert np.array_equal(n1, n2)
        if i in float_sums:
            assert np.allclose(v1[~n1], v2[~n2], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(v1[~n1], v2[~n2])
    return len(k1)


def check_rows(pr, keycols, sel, a, b, extreme=None, times=1):
    """against numpy: keycols [(values, isnull)] and the selection over the fact rows; extreme ("max" / "min",
    values, isnull) is the aggregate after the three common ones"""
    uk, inv = model_groups([(v[sel], isn[sel]) for v, isn in keycols])
    keys, cols = partial_rows(pr, len(keycols))
    assert np.array_equal(keys, uk)
    n = len(uk)
    assert np.array_equal(cols[0][0], times * np.bincount(inv, minlength=n))
    sums = np.zeros(n, dtype=np.int64)
    np.add.at(sums, inv, a[sel].astype(np.int64))
    assert np.array_equal(cols[1][0], times * sums)
    assert np.allclose(cols[2][0], times * np.bincount(inv, weights=b[sel], minlength=n), rtol=1e-12, atol=0)
    if extreme is not None:
        kind, v, isn = extreme
        v, ok = v[sel].astype(np.float64), ~isn[sel]
        want = np.full(n, -np.inf if kind == "max" else np.inf)
        (np.maximum if kind == "max" else np.minimum).at(want, inv[ok], v[ok])
        assert np.array_equal(cols[3][1], np.isinf(want))
        assert np.array_equal(cols[3][0][~np.isinf(want)].astype(np.float64), want[~np.isinf(want)])
    return n


def qual_passes(a, an, b, ext=EXT):
    return (~an) & (a < ext[0]) & (b > ext[1])


# ---------------------------------------------------------------------------------------------
# the chain fact -> d1 -> d2 of cases 1, 4, 5, 6, 7
# ---------------------------------------------------------------------------------------------
_CHAIN = {}


def chain(nd1=3000, nd2=700, holes1=1.3):
    """d1(key, g1 int4 nullable, x int4 nullable), d2(key, g2 int4 nullable, f float8 nullable); computed once"""
    if (nd1, nd2, holes1) not in _CHAIN:
        rng = np.random.default_rng(3001 + nd1 + nd2)
        d1 = Dim(rng, nd1, key_lo=-700, holes=holes1)
        d2 = Dim(rng, nd2, key_lo=100)
        d1.add("int4", (d1.key % 11).astype(np.int32), rng.random(nd1) < 0.04)
        x, xn = link_values(rng, d1, d2)
        x[0], xn[0] = d2.key[0], False          # (also a one-row d1 has a partner)
        d1.add("int4", x, xn)
        d2.add("int4", (d2.key % 53).astype(np.int32), rng.random(nd2) < 0.04)
        d2.add("float8", rng.random(nd2) * 10, rng.random(nd2) < 0.05)
        _CHAIN[(nd1, nd2, holes1)] = Tree([d1, d2], [0, 1], [1, 3])
    return _CHAIN[(nd1, nd2, holes1)]


CHAIN_FMAX = [(2, 2, "int4")] + FACT + [(2, 3, "float8")]          # GROUP BY d2.g2, pmax(d2.f)


def chain_against_numpy(n, tree=None, general=True, classes=False):
    runtime.init()
    tree = tree or chain()
    d1, d2 = tree.dims
    rng = np.random.default_rng(11 + n)
    fact, fkeys, a, an, b = make_fact(rng, n, [d1])
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        pr, _ = snowflake_rows(SPEC_FMAX, [(0, 53)], EXT, tree, joins, ds, CHAIN_FMAX)
        if general:
            pg, nitems = general_join_rows(SPEC_FMAX, [(0, 53)], EXT, tree, ds, CHAIN_FMAX)
    finally:
        for j in joins:
            j.end()
        ds.release()
    p = tree.partners(fkeys)
    alive = (p[0] >= 0) & (p[1] >= 0)
    if classes:
        # every way a parent row can miss the child occurs among the rows that reach d1
        x, xn = tree.column(p, 1, 3)
        reach = p[0] >= 0
        assert np.count_nonzero(reach & xn) > 0
        assert np.count_nonzero(reach & ~xn & (x < d2.key.min())) > 0
        assert np.count_nonzero(reach & ~xn & (x > d2.key.max())) > 0
        assert np.count_nonzero(reach & ~xn & (x >= d2.key.min()) & (x <= d2.key.max()) & (p[1] < 0)) > 0
        assert np.count_nonzero(alive) > 0
    sel = np.flatnonzero(alive & qual_passes(a, an, b))
    check_rows(pr, [tree.column(p, 2, 2)], sel, a, b, ("max",) + tree.column(p, 2, 3))
    if general:
        assert nitems == np.count_nonzero(alive)
        same_rows(pr, pg, 1)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("nrows", [1, TILE_ROWS - 1, TILE_ROWS + 1, 3 * TILE_ROWS + 5])
def test_chain_against_numpy_and_the_general_join(nrows, generic, monkeypatch):
    """case 1: GROUP BY d2.g2; nrows, psum of a fact int4 and a fact float8, pmax(d2.f): a float8 child column,
    the composed record is a standard 16-byte one (case 4 b); the mapping compiled in and the run-time form"""
    if generic:
        monkeypatch.setenv("STROM_GPUPREAGG_LOOKUP_GENERIC", "1")
    chain_against_numpy(nrows, classes=(nrows > TILE_ROWS + 1))


# ---------------------------------------------------------------------------------------------
# case 2: three levels
# ---------------------------------------------------------------------------------------------
def test_three_levels_with_an_int8_link_and_a_negative_key_range():
    """fact -> d1 -> d2 -> d3: d1.x is int8 (d2 is keyed by int8, below zero), d2.y is int4 (d3's keys start
    below zero too); GROUP BY a column of d1 and one of d3"""
    runtime.init()
    n = 3 * TILE_ROWS + 5
    rng = np.random.default_rng(3203)
    d1 = Dim(rng, 3000, key_lo=5)
    d2 = Dim(rng, 900, keytype="int8", key_lo=-2**33)
    d3 = Dim(rng, 300, key_lo=-500)
    d1.add("int4", (d1.key % 7).astype(np.int32), rng.random(d1.nd) < 0.03)
    d1.add("int8", *link_values(rng, d1, d2))
    d2.add("int4", *link_values(rng, d2, d3))
    d3.add("int4", (d3.key % 5 - 2).astype(np.int32), rng.random(d3.nd) < 0.03)
    tree = Tree([d1, d2, d3], [0, 1, 2], [1, 3, 2])
    columns = [(1, 2, "int4")] + FACT + [(3, 2, "int4")]
    fact, fkeys, a, an, b = make_fact(rng, n, [d1])
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        pr, _ = snowflake_rows(SPEC_TWOKEYS, [(0, 7), (-2, 5)], (), tree, joins, ds, columns)
        pg, nitems = general_join_rows(SPEC_TWOKEYS, [(0, 7), (-2, 5)], (), tree, ds, columns)
    finally:
        for j in joins:
            j.end()
        ds.release()
    p = tree.partners(fkeys)
    alive = np.logical_and.reduce([x >= 0 for x in p])
    assert 0 < np.count_nonzero(alive) < np.count_nonzero((p[0] >= 0) & (p[1] >= 0)) < np.count_nonzero(p[0] >= 0)
    sel = np.flatnonzero(alive & ~an)           # (a NULL summand is not summed, the row still counts)
    uk, inv = model_groups([(v[alive], isn[alive]) for v, isn in (tree.column(p, 1, 2), tree.column(p, 3, 2))])
    keys, cols = partial_rows(pr, 2)
    assert np.array_equal(keys, uk)
    assert np.array_equal(cols[0][0], np.bincount(inv, minlength=len(uk)))
    sums = np.zeros(len(uk), dtype=np.int64)
    np.add.at(sums, inv[~an[alive]], a[sel].astype(np.int64))
    assert np.array_equal(cols[1][1], np.bincount(inv[~an[alive]], minlength=len(uk)) == 0)
    assert np.array_equal(cols[1][0][~cols[1][1]], sums[~cols[1][1]])
    assert np.allclose(cols[2][0], np.bincount(inv, weights=b[alive], minlength=len(uk)), rtol=1e-12, atol=0)
    assert nitems == np.count_nonzero(alive)
    same_rows(pr, pg, 2)


# ---------------------------------------------------------------------------------------------
# case 3: bushy, two roots -- the star kernels
# ---------------------------------------------------------------------------------------------
def test_bushy_tree_with_two_roots_takes_the_star_kernel():
    """fact -> d1 -> {d2, d3} and fact -> d4, 53 groups (the dense plan): GROUP BY d2.g, the WHERE reads d3.h,
    pmax(d4.f); root 1's record is composed of two relations, root 2's is its own"""
    runtime.init()
    n = 3 * TILE_ROWS + 5
    rng = np.random.default_rng(3307)
    d1 = Dim(rng, 3000, key_lo=-700)
    d2 = Dim(rng, 700, key_lo=100)
    d3 = Dim(rng, 500, key_lo=-20)
    d4 = Dim(rng, 2000, key_lo=40)
    d1.add("int4", *link_values(rng, d1, d2)).add("int4", *link_values(rng, d1, d3))
    d2.add("int4", (d2.key % 53).astype(np.int32), rng.random(d2.nd) < 0.04)
    d3.add("int4", rng.integers(0, 10, d3.nd).astype(np.int32), rng.random(d3.nd) < 0.03)
    d4.add("float8", rng.random(d4.nd) * 10, rng.random(d4.nd) < 0.05)
    tree = Tree([d1, d2, d3, d4], [0, 1, 1, 0], [1, 2, 3, 2])
    columns = [(2, 2, "int4")] + FACT + [(4, 2, "float8"), (3, 2, "int4")]
    fact, fkeys, a, an, b = make_fact(rng, n, [d1, d4])
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        pr, pfm = snowflake_rows(SPEC_BUSHY, [(0, 53)], EXT, tree, joins, ds, columns)
        pg, nitems = general_join_rows(SPEC_BUSHY, [(0, 53)], EXT, tree, ds, columns)
    finally:
        for j in joins:
            j.end()
        ds.release()
    assert pfm[0]["num_kern_prep"] == 0                              # the dense kernel
    p = tree.partners(fkeys)
    alive = np.logical_and.reduce([x >= 0 for x in p])
    for r in range(4):                          # every relation alone drops rows the others would keep
        others = np.logical_and.reduce([p[q] >= 0 for q in range(4) if q != r and tree.parents[q] != r + 1])
        assert np.count_nonzero(others & (p[r] < 0)) > 0
    h, hn = tree.column(p, 3, 2)
    sel = np.flatnonzero(alive & qual_passes(a, an, b) & ~hn & (h > 1))
    assert 0 < len(sel) < np.count_nonzero(alive)
    check_rows(pr, [tree.column(p, 2, 2)], sel, a, b, ("max",) + tree.column(p, 4, 2))
    assert nitems == np.count_nonzero(alive)
    same_rows(pr, pg, 1)


def test_bushy_tree_with_packed_accumulators():
    """1e4 groups and summed OUTER columns without NULLs, as test_star_lookup_gpu's packed case arranges it:
    gpupreagg_packed_lookup_star (num_kern_prep reports it).  GROUP BY d2.g under root 1, d3 serves no column
    (a child that only filters), the WHERE reads root 2's column"""
    runtime.init()
    n, ngroups = 300007, 10000
    rng = np.random.default_rng(3409)
    d1 = Dim(rng, 40000, holes=1.25)
    d2 = Dim(rng, 12000, key_lo=50, holes=1.25)
    d3 = Dim(rng, 2500, key_lo=-20, holes=1.1)
    d4 = Dim(rng, 3000, key_lo=50, holes=1.25)
    d1.add("int4", (d2.key_lo + rng.integers(0, d2.span, d1.nd)).astype(np.int32))
    d1.add("int4", (d3.key_lo + rng.integers(0, d3.span, d1.nd)).astype(np.int32), rng.random(d1.nd) < 0.02)
    d2.add("int4", (d2.key % ngroups).astype(np.int32), rng.random(d2.nd) < 0.02)
    d3.add("int4", np.zeros(d3.nd, dtype=np.int32))
    d4.add("int4", rng.integers(0, 10, d4.nd).astype(np.int32), rng.random(d4.nd) < 0.03)
    tree = Tree([d1, d2, d3, d4], [0, 1, 1, 0], [1, 2, 3, 2])
    columns = [(2, 2, "int4")] + FACT + [(4, 2, "int4")]
    k1 = rng.integers(0, d1.span, n).astype(np.int32)
    k4 = (50 + rng.integers(0, d4.span, n)).astype(np.int32)
    a = rng.integers(-5 * 10**5, 2**20, n).astype(np.int32)
    b = rng.random(n)
    none = np.zeros(n, dtype=bool)
    fact = kds.build_kds("column", [kds.Column("int4", k1), kds.Column("int4", k4), kds.Column("int4", a),
                                    kds.Column("float8", b)])
    ext = [np.int32(2**19), 0.25]
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        pr, pfm = snowflake_rows(SPEC_PACKED, [(0, ngroups)], ext, tree, joins, ds, columns, nchunks=2)
    finally:
        for j in joins:
            j.end()
        ds.release()
    assert all(x["num_kern_prep"] == 1 for x in pfm)                 # the packed path was taken
    p = tree.partners({1: (k1, none), 2: (k4, none)})
    alive = np.logical_and.reduce([x >= 0 for x in p])
    assert np.count_nonzero((p[0] >= 0) & (p[1] >= 0) & (p[3] >= 0) & (p[2] < 0)) > 0      # d3 alone drops rows
    h, hn = tree.column(p, 4, 2)
    sel = np.flatnonzero(alive & qual_passes(a, none, b, ext) & ~hn & (h > 1))
    assert 0 < len(sel) < np.count_nonzero(alive)
    assert check_rows(pr, [tree.column(p, 2, 2)], sel, a, b, times=2) > 5000


# ---------------------------------------------------------------------------------------------
# case 4: records
# ---------------------------------------------------------------------------------------------
def chain_int_columns(columns, n=20011, seed=41):
    """SPEC_IMIN over the chain with a mapping of integer columns: (partial rows, model pieces)"""
    tree = chain()
    rng = np.random.default_rng(seed)
    fact, fkeys, a, an, b = make_fact(rng, n, [tree.dims[0]])
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        pr, _ = snowflake_rows(SPEC_IMIN, [(0, 53)], EXT, tree, joins, ds, columns)
    finally:
        for j in joins:
            j.end()
        ds.release()
    p = tree.partners(fkeys)
    sel = np.flatnonzero((p[0] >= 0) & (p[1] >= 0) & qual_passes(a, an, b))
    return pr, tree, p, sel, a, b


def test_integer_columns_narrow_records_and_standard_ones(monkeypatch):
    """case 4 a: GROUP BY d2.g2, pmin(d1.g1) -- every served column an integer: the composed record takes the
    narrow form; with STROM_HASHJOIN_NO_NARROW_RECS the standard one; the partial rows are equal"""
    runtime.init()
    columns = [(2, 2, "int4")] + FACT + [(1, 2, "int4")]
    pr, tree, p, sel, a, b = chain_int_columns(columns)
    check_rows(pr, [tree.column(p, 2, 2)], sel, a, b, ("min",) + tree.column(p, 1, 2))
    monkeypatch.setenv("STROM_HASHJOIN_NO_NARROW_RECS", "1")
    pr2 = chain_int_columns(columns)[0]
    assert same_rows(pr, pr2, 1) > 1


def test_the_link_column_is_also_served():
    """case 4 c: pmin(d1.x), the column that joins d2: it stays in the composed record"""
    runtime.init()
    pr, tree, p, sel, a, b = chain_int_columns([(2, 2, "int4")] + FACT + [(1, 3, "int4")])
    check_rows(pr, [tree.column(p, 2, 2)], sel, a, b, ("min",) + tree.column(p, 1, 3))


def test_a_child_that_serves_no_column_still_filters_rows():
    """case 4 d: GROUP BY d1.g1, pmin(d1.g1): d2 is an existence filter"""
    runtime.init()
    pr, tree, p, sel, a, b = chain_int_columns([(1, 2, "int4")] + FACT + [(1, 2, "int4")])
    assert np.count_nonzero((p[0] >= 0) & (p[1] < 0)) > 0
    check_rows(pr, [tree.column(p, 1, 2)], sel, a, b, ("min",) + tree.column(p, 1, 2))


# ---------------------------------------------------------------------------------------------
# case 5: compose edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nslots", [1, 255, 256, 257])
def test_parent_slot_counts_around_one_work_group(nslots):
    runtime.init()
    tree = chain(nd1=nslots, holes1=1.0)        # (no holes: as many slots as rows)
    joins = tree.open()
    try:
        assert joins[0].table_info(1)["nslots"] == nslots
    finally:
        for j in joins:
            j.end()
    chain_against_numpy(2003, tree=tree, general=False)


def test_a_child_with_one_slot():
    runtime.init()
    chain_against_numpy(2003, tree=chain(nd2=1), general=False)


def test_no_parent_row_has_a_partner_in_the_child():
    """zero partial rows, status 0"""
    runtime.init()
    rng = np.random.default_rng(3511)
    d1 = Dim(rng, 600)
    d2 = Dim(rng, 100, key_lo=1000)
    d1.add("int4", np.zeros(d1.nd, dtype=np.int32))
    d1.add("int4", rng.integers(-50, 900, d1.nd).astype(np.int32), rng.random(d1.nd) < 0.1)     # all below d2's keys
    d2.add("int4", (d2.key % 53).astype(np.int32)).add("float8", rng.random(d2.nd))
    tree = Tree([d1, d2], [0, 1], [1, 3])
    fact = make_fact(rng, 5003, [d1])[0]
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        pr, _ = snowflake_rows(SPEC_FMAX, [(0, 53)], EXT, tree, joins, ds, CHAIN_FMAX)
    finally:
        for j in joins:
            j.end()
        ds.release()
    assert len(pr) == 0


@pytest.mark.parametrize("max_grid", ["1", "3"])
def test_the_grid_stride_and_its_tail(max_grid, monkeypatch):
    """the 3000-row dimension has some 3900 slots: one work-group of 256 walks 15 strides and a tail, three
    walk 5 and a tail"""
    monkeypatch.setenv("STROM_HASHJOIN_DIMREC_MAX_GRID", max_grid)
    chain_against_numpy(TILE_ROWS + 1, general=False)


# ---------------------------------------------------------------------------------------------
# case 6: integer sums the range proof does not cover
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roots", [1, 2])
def test_unproven_integer_sums_are_folded_by_the_checked_program(roots):
    """int8 inputs near 2^56 with alternating signs, as test_star_lookup_gpu builds them: status 0, a checked
    fold, exact totals -- through the one-table lookup (a chain) and through the star (a second root)"""
    runtime.init()
    n = 6007
    tree = chain()
    rng = np.random.default_rng(3613)
    d4 = Dim(rng, 2000, key_lo=40).add("int4", np.zeros(2000, dtype=np.int32))
    if roots == 2:
        tree = Tree(tree.dims + [d4], [0, 1, 0], [1, 3, 2])
    k1, k1n = tree.dims[0].fact_keys(rng, n, True)
    k4, k4n = d4.fact_keys(rng, n, True)
    x = (rng.integers(2**55, 2**56, n) * np.where(np.arange(n) % 2 == 0, 1, -1)).astype(np.int64)
    fact = kds.build_kds("column", [kds.Column("int4", k1, k1n), kds.Column("int4", k4, k4n), kds.Column("int8", x)])
    columns = [(2, 2, "int4"), (0, 3, "int8"), (2, 3, "float8")]
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        st, _, pr, checked = fold(SPEC_CHECKED, [(0, 53)], (), lambda agg: agg.submit_lookup_snowflake(
            joins, tree.parents, ds, columns, tree.link_types))
    finally:
        for j in joins:
            j.end()
        ds.release()
    assert st == [0] and checked >= 1
    p = tree.partners({1: (k1, k1n), 2: (k4, k4n)})
    sel = np.flatnonzero(np.logical_and.reduce([q >= 0 for q in p]))
    g, gn = tree.column(p, 2, 2)
    uk, inv = model_groups([(g[sel], gn[sel])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    assert np.array_equal(cols[0][0], np.bincount(inv, minlength=len(uk)))
    want = [0] * len(uk)
    for grp, v in zip(inv, x[sel]):
        want[grp] += int(v)
    assert all(-2**63 <= w < 2**63 for w in want)
    assert [int(v) for v in cols[1][0]] == want


# ---------------------------------------------------------------------------------------------
# case 7: the composed-record cache and lifetimes
# ---------------------------------------------------------------------------------------------
def test_composed_records_follow_the_tables_they_were_made_from():
    runtime.init()
    n = 20011
    tree = chain()
    d1, d2 = tree.dims
    rng = np.random.default_rng(3719)
    fact, fkeys, a, an, b = make_fact(rng, n, [d1])
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    try:
        first = snowflake_rows(SPEC_FMAX, [(0, 53)], EXT, tree, joins, ds, CHAIN_FMAX)[0]
        again = snowflake_rows(SPEC_FMAX, [(0, 53)], EXT, tree, joins, ds, CHAIN_FMAX)[0]     # from the cache
        assert same_rows(first, again, 1) > 1
        # a new child in the old one's place (likely at its address): other group keys, other rows present
        joins[1].end()
        e2 = Dim(rng, d2.nd - 100, key_lo=d2.key_lo + 30)
        e2.add("int4", ((e2.key * 7 + 3) % 53).astype(np.int32), rng.random(e2.nd) < 0.04)
        e2.add("float8", rng.random(e2.nd) * 10, rng.random(e2.nd) < 0.05)
        tree2 = Tree([d1, e2], [0, 1], [1, 3])
        joins[1] = open_joins([e2], [3])[0]
        third = snowflake_rows(SPEC_FMAX, [(0, 53)], EXT, tree2, joins, ds, CHAIN_FMAX)[0]
        # releasing the session before the tables (above) and the tables before the session, child first or last
        agg = GpuPreAgg(SPEC_FMAX).begin([(0, 53)], ext_params=EXT)
        assert agg.collect(agg.submit_lookup_snowflake(joins, tree2.parents, ds, CHAIN_FMAX, tree2.link_types))[0] == 0
        joins[0].end()
        joins[1].end()
        joins = []
        last = agg.fetch()
        agg.end()
    finally:
        for j in joins:
            j.end()
        ds.release()
    for t, pr in ((tree, first), (tree2, third), (tree2, last)):
        p = t.partners(fkeys)
        sel = np.flatnonzero((p[0] >= 0) & (p[1] >= 0) & qual_passes(a, an, b))
        check_rows(pr, [t.column(p, 2, 2)], sel, a, b, ("max",) + t.column(p, 2, 3))


# ---------------------------------------------------------------------------------------------
# case 8: delegation
# ---------------------------------------------------------------------------------------------
def equal_rows(pr1, pr2, nkeys):
    """identical partial rows: the same code path ran (a float8 sum is added up in the order the waves
    arrive, so two runs of the SAME kernel agree to the file's 1e-12, not to the bit)"""
    assert same_rows(pr1, pr2, nkeys) > 1


def test_no_relation_on_another_is_the_star_call_and_one_relation_the_one_table_call():
    runtime.init()
    n = 30011
    rng = np.random.default_rng(3823)
    d1 = Dim(rng, 3000, key_lo=-700).add("int4", (np.arange(3000) % 53).astype(np.int32), rng.random(3000) < 0.04)
    d4 = Dim(rng, 2000, key_lo=40).add("float8", rng.random(2000) * 10, rng.random(2000) < 0.05)
    fact = make_fact(rng, n, [d1, d4])[0]
    two = [(1, 2, "int4")] + FACT + [(2, 2, "float8")]
    one = [(1, 2, "int4")] + FACT + [(1, 2, "int4")]
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins([d1, d4], [1, 2])
    try:
        star = fold(SPEC_FMAX, [(0, 53)], EXT, lambda agg: agg.submit_lookup_star(joins, ds, two))
        snow = fold(SPEC_FMAX, [(0, 53)], EXT, lambda agg: agg.submit_lookup_snowflake(joins, [0, 0], ds, two))
        assert star[0] == snow[0] == [0]
        equal_rows(star[2], snow[2], 1)
        look = fold(SPEC_IMIN, [(0, 53)], EXT, lambda agg: agg.submit_lookup(joins[0], ds, one))
        snow = fold(SPEC_IMIN, [(0, 53)], EXT, lambda agg: agg.submit_lookup_snowflake(joins[:1], [0], ds, one))
        assert look[0] == snow[0] == [0]
        equal_rows(look[2], snow[2], 1)
    finally:
        for j in joins:
            j.end()
        ds.release()


# ---------------------------------------------------------------------------------------------
# case 9: refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_session_usable():
    runtime.init()
    n = 5003
    tree = chain()
    d1, d2 = tree.dims
    rng = np.random.default_rng(3929)
    d4 = Dim(rng, 2000, key_lo=40).add("float8", rng.random(2000)).add("float8", rng.random(2000))
    fact, fkeys, a, an, b = make_fact(rng, n, [d1, d4])
    ds = runtime.DeviceStore.upload(fact)
    joins = tree.open()
    others = []

    def table(spec, dims_and_keys):
        j = GpuHashJoin(spec).begin(build_multihash([(d.chunk(), keys) for d, keys in dims_and_keys]))
        others.append(j)
        return j

    dup = Dim(rng, 500, key_lo=100)
    dup.key[:50] = dup.key[50:100]                                  # duplicate keys
    dup.add("int4", np.arange(500, dtype=np.int32)).add("float8", rng.random(500))
    small = Dim(rng, 80)
    small.chunk = lambda fmt="row_flat": kds.build_kds(fmt, [kds.Column("int2", small.key.astype(np.int16)),
                                                              kds.Column("int4", np.arange(80, dtype=np.int32))])
    j_dup = table("(gpuhashjoin (rel (hashkey (var 3 int4) 1 int4)))", [(dup, [1])])
    j_qual = table("(gpuhashjoin (rel (hashkey (var 3 int4) 1 int4) (qual (int4lt (var 2 int4) (const int4 5)))))",
                   [(d2, [1])])
    j_two = table("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)) (rel (hashkey (var 3 int4) 1 int4)))",
                  [(d1, [1]), (d2, [1])])
    j_int2 = table("(gpuhashjoin (rel (hashkey (var 2 int2) 1 int2)))", [(small, [1])])
    j_col9 = table("(gpuhashjoin (rel (hashkey (var 9 int4) 1 int4)))", [(d2, [1])])     # d1 has three columns
    j_d4 = table("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))", [(d4, [1])])
    f16 = [Dim(rng, 300, key_lo=40).add("float8", rng.random(300)) for _ in range(2)]
    j_f16 = [table("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))", [(d, [1])]) for d in f16]
    assert not j_dup.table_info(1)["unique"]

    agg = GpuPreAgg(SPEC_FMAX).begin([(0, 53)], ext_params=EXT)
    hashed = GpuPreAgg(SPEC_FMAX).begin_hashed(ext_params=EXT)
    text = GpuPreAgg("(gpupreagg (qual (texteq (var 5 text) (const text \"x\"))) (key (var 1 int4)) (nrows))")
    text.begin([(0, 53)])
    err = ctypes.c_int(0)
    pb = ctypes.create_string_buffer(agg.parambuf, len(agg.parambuf))
    nodomain = lib.strom_gpupreagg_create(agg.program.key, agg.codegen._targets_c, len(agg.targets), pb,
                                          None, 0, ctypes.byref(err))
    assert nodomain
    I4 = ["int4"] * 8

    def refused(owner, tbls, parents, columns, link_types=I4, session=None, code=BAD_REQUEST):
        saved = owner.session
        if session is not None:
            owner.session = session
        try:
            with pytest.raises(runtime.StromError) as ei:
                owner.submit_lookup_snowflake(tbls, parents, ds, columns, link_types[:len(tbls)])
            assert ei.value.errcode == code, ei.value
        finally:
            owner.session = saved

    def raw(parent, links, tbls=joins):
        """the C call with pointers as given"""
        depth = np.array([d for d, _, _ in CHAIN_FMAX], dtype=np.int32)
        colidx = np.array([c - 1 for _, c, _ in CHAIN_FMAX], dtype=np.int32)
        oids = np.array([kds.column_type_oid(t) for _, _, t in CHAIN_FMAX], dtype=np.int32)
        arr = (ctypes.c_void_p * 2)(*[j.table for j in joins]) if tbls is not None else None
        e = ctypes.c_int(0)
        task = lib.strom_submit_gpupreagg_lookup_snowflake(
            agg.session, arr, 2, parent.ctypes.data if parent is not None else None,
            links.ctypes.data if links is not None else None, ds.handle, 4, depth.ctypes.data, colidx.ctypes.data,
            oids.ctypes.data, None, None, ctypes.byref(e))
        assert not task and e.value == BAD_REQUEST

    try:
        par, lnk = np.array([0, 1], dtype=np.int32), np.array([0, kds.column_type_oid("int4")], dtype=np.int32)
        raw(None, lnk)                                                      # a NULL argument
        raw(par, None)
        raw(par, lnk, tbls=None)
        refused(agg, [], [], CHAIN_FMAX)                                    # ntbls outside 1 .. 8
        refused(agg, joins + [joins[1]] * 7, [0] + [1] * 8, CHAIN_FMAX, I4 + I4)
        refused(agg, joins, [1, 1], CHAIN_FMAX)                             # parent[d - 1] outside 0 .. d - 1
        refused(agg, joins, [0, 2], CHAIN_FMAX)
        refused(agg, joins, [0, -1], CHAIN_FMAX)
        refused(agg, joins + [j_d4] * 4, [0, 1, 0, 0, 0, 0], CHAIN_FMAX)    # five roots
        refused(agg, [joins[0], j_dup], [0, 1], CHAIN_FMAX)                 # a child with duplicate keys
        refused(agg, [joins[0], j_qual], [0, 1], CHAIN_FMAX)                # a WHERE pulled up into the join program
        refused(agg, [joins[0], j_two], [0, 1], CHAIN_FMAX)                 # a table of two relations
        refused(agg, joins, [0, 1], CHAIN_FMAX, ["int4", "int2"])           # a link type that is not 4 or 8 bytes wide
        refused(agg, [joins[0], j_int2], [0, 1], CHAIN_FMAX, ["int4", "int2"])
        # 16 columns of d1 and the link: 17 at the first step, though the composed record would hold 16
        refused(agg, joins, [0, 1], [(1, 2, "int4")] + FACT + [(0, 4, "float8")] + [(1, 2, "int4")] * 15)
        refused(agg, joins, [0, 1], [(3, 2, "int4")] + CHAIN_FMAX[1:])      # a depth outside 0 .. ntbls
        # two roots: a composed record longer than 16 bytes; 16 + 16 + 16 bytes over three roots
        refused(agg, joins + [j_d4], [0, 1, 0], CHAIN_FMAX + [(1, 2, "int4")])
        refused(agg, joins + j_f16, [0, 1, 0, 0], CHAIN_FMAX + [(3, 2, "float8"), (4, 2, "float8")])
        refused(text, joins, [0, 1], CHAIN_FMAX + [(2, 2, "int4")])         # a text variable not at depth 0
        refused(hashed, joins, [0, 1], CHAIN_FMAX)                          # a hashed session
        refused(agg, joins, [0, 1], CHAIN_FMAX, session=nodomain)           # a session without a domain
        # the link column: one the parent does not have; one of another width than its type says
        refused(agg, [joins[0], j_col9], [0, 1], CHAIN_FMAX, code=CORRUPTION)
        refused(agg, joins, [0, 1], CHAIN_FMAX, ["int4", "int8"], code=CORRUPTION)
        # nothing was folded (the counts below would show it), and the session still works
        assert agg.collect(agg.submit_lookup_snowflake(joins, [0, 1], ds, CHAIN_FMAX, tree.link_types))[0] == 0
        pr = agg.fetch()
    finally:
        lib.strom_gpupreagg_release(nodomain)
        agg.end()
        hashed.end()
        text.end()
        for j in joins + others:
            j.end()
        ds.release()
    p = tree.partners(fkeys)
    sel = np.flatnonzero((p[0] >= 0) & (p[1] >= 0) & qual_passes(a, an, b))
    check_rows(pr, [tree.column(p, 2, 2)], sel, a, b, ("max",) + tree.column(p, 2, 3))
