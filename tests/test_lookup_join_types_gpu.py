"""
LEFT, SEMI and ANTI relations in the fused lookup and star folds (strom_submit_gpupreagg_lookup_typed;
gpupreagg_dense_lookup / _packed_lookup with GPUPREAGG_LOOKUP_JOINTYPE, the _star kernels with
GPUPREAGG_STAR_JOINTYPE_<d>; needs an MI355X: -m gpu).  The parent of this change has no such symbol:
every test here fails there.

The rule (fold_rule below; test_lookup_join_types_cpu.py holds it against the nested-loop
join_model): a row has a partner in a relation when its key is not NULL, inside the key range, and
the slot is present -- Dim.partner() >= 0.  A row is folded iff every inner and semi relation has
a partner and no anti relation has one; the columns of a left relation are NULL without a partner.
What the kernel can get wrong is a row whose probe was masked: it reads slot 0, which is always
an occupied record.  So the one-table dimension's slot-0 row carries a group value and a column
value no other row has, and both would show in the NULL group and in a pmax.

Bars, the project's: keys, counts, integer sums and min / max bit-exact; float8 sums rtol 1e-12
(check_count_and_sums: a group sums at most ~1e5 values of [0, 1) in the order the LDS atomics
pick; worst case 1e5 * 2^-53 = 1.1e-11 only if every rounding went one way, sqrt(1e5) * 2^-53
= 3.5e-14 as a random walk).  Where two requests must give IDENTICAL partial rows (all-inner against the
existing calls, semi against the inner lookup) the fact's float8 column holds multiples of 2^-20, whose
sums are exact in any order, and every column is compared bit for bit.
"""
import numpy as np
import pytest

import join_model as jm
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpupreagg import GpuPreAgg, lookup_typed_defines
from test_star_lookup_gpu import (BAD_REQUEST, CPU_RECHECK, EXT, NULLKEY, OVERFLOW_QUAL, QUAL, TILE_ROWS, Dim,
                                  check_count_and_sums, model_groups, open_joins, partial_rows, two_dims)

pytestmark = pytest.mark.gpu

NG = 53                                         # groups of the dimension's column: 0 .. NG - 1, and NG at slot 0
FG = 17                                         # groups of the fact's own group column
SLOT0_MAX = 10**6                               # the slot-0 row's second column: above every other value


def fold_rule(partners, jointypes):
    """bool per fact row: folded?  partners[d]: Dim.partner() of relation d + 1"""
    keep = np.ones(len(partners[0]), dtype=bool)
    for p, jt in zip(partners, jointypes):
        if jt in ("inner", "semi"):
            keep &= (p >= 0)
        elif jt == "anti":
            keep &= (p < 0)
        else:
            assert jt == "left"
    return keep


def served(dim, colno, p):
    """(values, isnull) of a dimension column per fact row: NULL without a partner"""
    _, v, isn = dim.cols[colno]
    i = np.clip(p, 0, dim.nd - 1)
    return v[i], isn[i] | (p < 0)


_ONE = {}


def one_dim(form="narrow4"):
    """the one-table dimension per record form (computed once, shared, left unchanged): column 1 the
    group column with NULLs, column 2 the pmax column with NULLs; the row at slot 0 (the smallest
    key) has group NG and the largest column value, both not NULL"""
    if form not in _ONE:
        rng = np.random.default_rng(3001)
        d = Dim(rng, 3000, key_lo=-700)
        g = (d.key % NG).astype(np.int32)
        gn = rng.random(d.nd) < 0.04
        s0 = int(np.argmin(d.key))
        g[s0], gn[s0] = NG, False
        d.add("int4", g, gn)
        if form == "narrow2":                   # presence + 2 NULL bits + 6 + 3 bits: a 2-byte record
            v = rng.integers(0, 6, d.nd).astype(np.int32)
            v[s0] = 7
            d.add("int4", v, rng.random(d.nd) < 0.05)
        elif form in ("narrow4", "wide16"):     # 6 + 20 value bits: 4 bytes; plain: flags + 2 x int4 = 16
            v = rng.integers(-1000, 1000, d.nd).astype(np.int32)
            v[s0] = SLOT0_MAX
            d.add("int4", v, rng.random(d.nd) < 0.05)
        elif form == "wide8":                   # flags + one int4: 8 bytes (no second column)
            pass
        else:                                   # flags + int4 + 2 x float8: a 32-byte record
            v = rng.random(d.nd) * 10
            v[s0] = float(SLOT0_MAX)
            d.add("float8", v, rng.random(d.nd) < 0.05)
            d.add("float8", rng.random(d.nd))
        if len(d.cols) > 1:
            d.cols[1][2][s0] = False
        _ONE[form] = d
    return _ONE[form]


class Fact(object):
    """fact(k_1 .. k_R, a int4, b float8, g int4): keys from Dim.fact_keys"""

    def __init__(self, dims, n, seed, nulls=True, fgroups=FG, a_range=(0, 2**31), exact_b=False):
        rng = np.random.default_rng(seed)
        self.dims, self.n, self.nulls = dims, n, nulls
        self.fk = [d.fact_keys(rng, n, nulls) for d in dims]
        self.a = rng.integers(a_range[0], a_range[1], n, dtype=np.int64).astype(np.int32)
        self.an = (rng.random(n) < 0.03) if nulls else np.zeros(n, dtype=bool)
        if nulls and n >= 1:
            self.an[0] = True                   # (a chunk without a NULL has no bitmap: also at one row)
        self.b = rng.random(n)
        if exact_b:
            # multiples of 2^-20 in [0, 1): any sum of fewer than 2^33 of them is exact in float8, so the
            # order in which the LDS atomics add them up cannot show -- two requests can be compared bit for bit
            self.b = np.floor(self.b * 2**20) / 2**20
        self.g = rng.integers(0, fgroups, n).astype(np.int32)
        R = len(dims)
        self.A, self.B, self.G = R + 1, R + 2, R + 3        # attribute numbers

    def chunk(self):
        cols = [kds.Column(d.keytype, k, kn if self.nulls else None) for d, (k, kn) in zip(self.dims, self.fk)]
        cols += [kds.Column("int4", self.a, self.an if self.nulls else None), kds.Column("float8", self.b),
                 kds.Column("int4", self.g)]
        return kds.build_kds("column", cols)

    def partners(self):
        return [d.partner(k, kn) for d, (k, kn) in zip(self.dims, self.fk)]


LAST_DEFINES = []                               # the define blocks of the programs run()'s session built


def run(fact, jointypes, spec, columns, domain, ext=EXT, nchunks=1, call="typed", ds=None, joins=None):
    """the request(s) over the fact chunk: (status, PartialRows or None, [perfmon])"""
    runtime.init()
    own_ds, own_joins = ds is None, joins is None
    if own_ds:
        ds = runtime.DeviceStore.upload(fact.chunk())
    if own_joins:
        joins = open_joins(fact.dims, list(range(1, len(fact.dims) + 1)))
    agg = GpuPreAgg(spec)
    pfms, st, pr = [], 0, None
    del LAST_DEFINES[:]
    try:
        agg.begin(domain, ext_params=list(ext))
        for _ in range(nchunks):
            if call == "typed":
                pending = agg.submit_lookup_typed(joins, jointypes, ds, columns)
            elif call == "star":
                pending = agg.submit_lookup_star(joins, ds, columns)
            else:
                pending = agg.submit_lookup(joins[0], ds, columns)
            st, pfm = agg.collect(pending)
            pfms.append(pfm)
            if st != 0:
                break
        pr = agg.fetch() if st == 0 else None
        LAST_DEFINES.extend(agg.mapping_defines())
    finally:
        agg.end()
        if own_joins:
            for j in joins:
                j.end()
        if own_ds:
            ds.release()
    return st, pr, pfms


def check(pr, keycols, sel, fact, times=1, maxcol=None):
    """the partial rows against numpy over the folded rows `sel`: keys, nrows, psum(int8 a), psum(b),
    and pmax of maxcol = (values, isnull) over all fact rows when given"""
    uk, inv = model_groups([(v[sel], isn[sel]) for v, isn in keycols])
    keys, cols = partial_rows(pr, len(keycols))
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), fact.a[sel], fact.b[sel], times=times)
    if maxcol is not None:
        v, isn = maxcol[0][sel].astype(np.float64), maxcol[1][sel]
        wmax = np.full(len(uk), -np.inf)
        np.maximum.at(wmax, inv[~isn], v[~isn])
        assert np.array_equal(cols[3][1], np.isinf(wmax))
        assert np.array_equal(cols[3][0][~np.isinf(wmax)].astype(np.float64), wmax[~np.isinf(wmax)])
    return uk, inv


def qual_passes(fact):
    return (~fact.an) & (fact.a < EXT[0]) & (fact.b > EXT[1])


AGG3 = "(nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"
LEFT_SPEC = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) " + AGG3 + " (pmax (var 4 int4)))"
FACTKEY_SPEC = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) " + AGG3 + ")"


def one_columns(fact, jt, maxtype="int4"):
    if jt in ("left", "inner"):
        cols = [(1, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]
        return cols + ([(1, 3, maxtype)] if len(fact.dims[0].cols) > 1 else [])
    return [(0, fact.G, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]


def one_table_against_numpy(jt, n, nulls, form="narrow4", seed=None, exact_b=False):
    d = one_dim(form)
    s0 = int(np.argmin(d.key))
    assert d.cols[0][1][s0] == NG and not d.cols[0][2][s0] and np.count_nonzero(d.cols[0][1] == NG) == 1
    if len(d.cols) > 1:
        assert not d.cols[1][2][s0] and d.cols[1][1][s0] > np.delete(d.cols[1][1], s0).max()
    fact = Fact([d], n, (31 + n) if seed is None else seed, nulls, exact_b=exact_b)
    p = fact.partners()[0]
    k, kn = fact.fk[0]
    if n >= TILE_ROWS:                          # every partner class: a partner, a hole, below, above, NULL
        off = k.astype(np.int64) - d.key_lo
        assert np.count_nonzero(p >= 0) > 0 and np.count_nonzero((p < 0) & ~kn & (off >= 0) & (off < d.span)) > 0
        assert np.count_nonzero(~kn & (off < 0)) > 0 and np.count_nonzero(~kn & (off >= d.span)) > 0
        assert (not nulls) or np.count_nonzero(kn) > 0
    maxtype = d.cols[1][0] if len(d.cols) > 1 else None
    if jt == "left":
        spec = LEFT_SPEC.replace("(var 4 int4)", "(var 4 %s)" % maxtype) if maxtype else FACTKEY_SPEC
    else:
        spec = FACTKEY_SPEC
    columns = one_columns(fact, jt, maxtype)
    if jt == "left" and len(d.cols) > 2:        # a third served column: the record passes 16 bytes
        columns = columns + [(1, 4, d.cols[2][0])]
        spec = spec[:-1] + " (pmin (var 5 %s)))" % d.cols[2][0]
    st, pr, _ = run(fact, [jt], spec, columns, [(0, NG + 1)])
    assert st == 0
    sel = np.flatnonzero(fold_rule([p], [jt]) & qual_passes(fact))
    if jt == "left":
        uk, inv = check(pr, [served(d, 0, p)], sel, fact, maxcol=served(d, 1, p) if maxtype else None)
        if len(d.cols) > 2:
            v, isn = served(d, 2, p)
            wmin = np.full(len(uk), np.inf)
            np.minimum.at(wmin, inv[~isn[sel]], v[sel][~isn[sel]])
            got = partial_rows(pr, 1)[1][4]
            assert np.array_equal(got[1], np.isinf(wmin)) and np.array_equal(got[0][~got[1]], wmin[~np.isinf(wmin)])
    else:
        check(pr, [(fact.g, np.zeros(n, dtype=bool))], sel, fact)
    return fact, pr


# ---------------------------------------------------------------------------------------------
# case 1: one table, around one tile
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("nrows", [1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 3])
@pytest.mark.parametrize("jt", ["left", "semi", "anti"])
def test_one_table_around_one_tile(jt, nrows, nulls):
    """left groups by the dimension's column (partner-less rows and NULL columns share the NULL
    group) and takes pmax of a second dimension column; semi and anti group by a fact column"""
    # (semi: float8 inputs that sum exactly in any order, for the comparison below)
    fact, pr = one_table_against_numpy(jt, nrows, nulls, exact_b=(jt == "semi"))
    if jt != "semi":
        return
    # semi is the inner lookup with the same table serving no column: partial rows identical, floats included
    st, pi, _ = run(fact, None, FACTKEY_SPEC, one_columns(fact, "semi"), [(0, NG + 1)], call="lookup")
    assert st == 0
    (ks, cs), (ki, ci) = partial_rows(pr, 1), partial_rows(pi, 1)
    assert np.array_equal(ks, ki)
    assert len(cs) == len(ci) == 3
    for (vs, ns), (vi, ni) in zip(cs, ci):
        assert np.array_equal(ns, ni) and np.array_equal(vs, vi)


# ---------------------------------------------------------------------------------------------
# case 2: one table, LEFT, every record form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["narrow2", "narrow4", "wide8", "wide16", "wide32"])
def test_left_with_every_record_form(form, monkeypatch):
    """narrow 2- and 4-byte records; 8 and 16 bytes with STROM_HASHJOIN_NO_NARROW_RECS; a 32-byte
    record (two float8 columns: the kernel reads its columns behind the flags word)"""
    if form in ("wide8", "wide16"):
        monkeypatch.setenv("STROM_HASHJOIN_NO_NARROW_RECS", "1")
    one_table_against_numpy("left", 2 * TILE_ROWS + 3, True, form=form, seed=4001)
    # the table really gave that form: the program the session built is the one of this mapping
    reclen, narrow, served_cols = RECORD_FORMS[form]
    assert LAST_DEFINES == [lookup_typed_defines([(4, reclen, narrow, served_cols)], ["left"])], LAST_DEFINES


# form -> (slot record length, narrow?, the virtual columns the dimension serves)
RECORD_FORMS = {"narrow2": (2, True, [0, 3]), "narrow4": (4, True, [0, 3]), "wide8": (8, False, [0]),
                "wide16": (16, False, [0, 3]), "wide32": (32, False, [0, 3, 4])}


# ---------------------------------------------------------------------------------------------
# case 3: stars
# ---------------------------------------------------------------------------------------------
def two_relations_against_numpy(jts, n, nchunks=1):
    d1, d2 = two_dims()
    fact = Fact([d1, d2], n, 51 + n)
    p1, p2 = fact.partners()
    for c1 in (True, False):                    # all 2^2 partner classes
        for c2 in (True, False):
            assert np.count_nonzero(((p1 >= 0) == c1) & ((p2 >= 0) == c2)) > 0
    key1 = jts[0] in ("inner", "left")
    max2 = jts[1] in ("inner", "left")
    columns = [(1, 2, "int4") if key1 else (0, fact.G, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]
    spec = FACTKEY_SPEC
    if max2:
        columns.append((2, 2, "float8"))
        spec = LEFT_SPEC.replace("(var 4 int4)", "(var 4 float8)")
    st, pr, _ = run(fact, jts, spec, columns, [(0, NG)], nchunks=nchunks)
    assert st == 0
    sel = np.flatnonzero(fold_rule([p1, p2], jts) & qual_passes(fact))
    assert 0 < len(sel) < n
    keycol = served(d1, 0, p1) if key1 else (fact.g, np.zeros(n, dtype=bool))
    check(pr, [keycol], sel, fact, times=nchunks, maxcol=served(d2, 0, p2) if max2 else None)


@pytest.mark.parametrize("jts", [("inner", "left"), ("left", "anti"), ("semi", "anti"), ("left", "left")])
def test_star_pairs(jts):
    two_relations_against_numpy(list(jts), 2 * TILE_ROWS + 3)


@pytest.mark.parametrize("narrow", [True, False])
def test_star_semi_left_anti_inner_one_keyed_by_int8(narrow, monkeypatch):
    if not narrow:
        monkeypatch.setenv("STROM_HASHJOIN_NO_NARROW_RECS", "1")
    n, nd = 50021, 2000
    rng = np.random.default_rng(5003)
    dims = [Dim(rng, nd, keytype=("int8" if r == 2 else "int4"), key_lo=(2**33 if r == 2 else 10 * r), holes=1.15)
            for r in range(4)]
    dims[1].add("int4", rng.integers(-5, 6, nd).astype(np.int32), rng.random(nd) < 0.03)
    dims[3].add("int4", rng.integers(-5, 6, nd).astype(np.int32), rng.random(nd) < 0.03)
    jts = ["semi", "left", "anti", "inner"]
    fact = Fact(dims, n, 5005)
    spec = ("(gpupreagg (qual (int4gt (var 5 int4) (const int4 -4))) (key (var 1 int4)) (key (var 4 int4)) "
            + AGG3 + " (pmax (var 6 int4)))")
    # (six variables, 28 bytes a row: the code generator then folds one quad a thread; var 6 is a fact column,
    # so that the records stay 8 bytes each, 32 in all, without the narrow form)
    columns = [(0, fact.G, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8"), (2, 2, "int4"), (4, 2, "int4"),
               (0, fact.A, "int4")]
    st, pr, _ = run(fact, jts, spec, columns, [(0, FG), (-5, 11)], ext=())
    assert st == 0
    p = fact.partners()
    for r in range(4):                          # every relation alone decides rows the others would keep
        others = fold_rule([p[q] for q in range(4) if q != r], [jts[q] for q in range(4) if q != r])
        assert np.count_nonzero(others & (p[r] < 0)) > 0 and np.count_nonzero(others & (p[r] >= 0)) > 0
    v5, n5 = served(dims[3], 0, p[3])
    # (psum (int8 a)) skips a NULL a: the model sums a where it is not NULL, as check() does over sel
    sel = np.flatnonzero(fold_rule(p, jts) & ~n5 & (v5 > -4))
    assert 0 < len(sel) < n
    a_saved = fact.a
    fact.a = np.where(fact.an, 0, fact.a).astype(np.int32)
    try:
        check(pr, [(fact.g, np.zeros(n, dtype=bool)), served(dims[1], 0, p[1])], sel, fact,
              maxcol=(a_saved, fact.an))
    finally:
        fact.a = a_saved


# ---------------------------------------------------------------------------------------------
# case 4: one work-group per CU
# ---------------------------------------------------------------------------------------------
def test_a_work_group_walks_several_tiles_left_and_anti(monkeypatch):
    monkeypatch.setenv("STROM_GPUPREAGG_BLOCKS_PER_CU", "1")
    runtime.init()
    W = runtime.device_info()["compute_units"]
    two_relations_against_numpy(["left", "anti"], 2 * W * TILE_ROWS + 5)


# ---------------------------------------------------------------------------------------------
# case 5: packed accumulators
# ---------------------------------------------------------------------------------------------
_PACKED = {}


def packed_dims():
    if not _PACKED:
        rng = np.random.default_rng(6007)
        d1 = Dim(rng, 40000, holes=1.25)
        d1.add("int4", (d1.key % 10000).astype(np.int32), rng.random(d1.nd) < 0.02)
        d2 = Dim(rng, 3000, key_lo=50, holes=1.25)
        d2.add("int4", rng.integers(0, 10, d2.nd).astype(np.int32), rng.random(d2.nd) < 0.03)
        _PACKED["d"] = (d1, d2)
    return _PACKED["d"]


@pytest.mark.parametrize("shape", ["one_table_anti", "star_inner_left"])
def test_packed_accumulators(shape):
    """1e4 groups, summed OUTER columns without NULLs, two chunks into one session"""
    n, ngroups = 300007, 10000
    d1, d2 = packed_dims()
    ext = [np.int32(2**19), 0.25]
    if shape == "one_table_anti":
        fact = Fact([d2], n, 6011, nulls=False, fgroups=ngroups, a_range=(-5 * 10**5, 2**20))
        jts, spec = ["anti"], FACTKEY_SPEC
        columns = [(0, fact.G, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]
    else:
        fact = Fact([d1, d2], n, 6013, nulls=False, a_range=(-5 * 10**5, 2**20))
        jts = ["inner", "left"]
        spec = ("(gpupreagg (qual (and " + QUAL + " (or (isnull (var 4 int4)) (int4gt (var 4 int4) (const int4 1)))))"
                " (key (var 1 int4)) " + AGG3 + ")")
        columns = [(1, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8"), (2, 2, "int4")]
    st, pr, pfms = run(fact, jts, spec, columns, [(0, ngroups)], ext=ext, nchunks=2)
    assert st == 0
    assert len(pfms) == 2 and all(p["num_kern_prep"] == 1 for p in pfms)      # the packed path was taken
    p = fact.partners()
    passes = (fact.a < ext[0]) & (fact.b > ext[1])
    if shape == "one_table_anti":
        keycol = (fact.g, np.zeros(n, dtype=bool))
    else:
        v4, n4 = served(d2, 0, p[1])
        passes &= n4 | (v4 > 1)
        assert np.count_nonzero(passes & (p[0] >= 0) & (p[1] < 0)) > 0        # left keeps them, NULL column
        keycol = served(d1, 0, p[0])
    sel = np.flatnonzero(fold_rule(p, jts) & passes)
    assert 0 < len(sel) < n
    check(pr, [keycol], sel, fact, times=2)


# ---------------------------------------------------------------------------------------------
# case 6: quals
# ---------------------------------------------------------------------------------------------
def test_a_qual_over_a_left_column_drops_the_rows_without_a_partner():
    d = one_dim()
    n = 20011
    fact = Fact([d], n, 7001)
    spec = "(gpupreagg (qual (int4gt (var 4 int4) (const int4 -200))) (key (var 1 int4)) " + AGG3 + " (pmax (var 4 int4)))"
    st, pr, _ = run(fact, ["left"], spec, one_columns(fact, "left"), [(0, NG + 1)], ext=())
    assert st == 0
    p = fact.partners()[0]
    v4, n4 = served(d, 1, p)
    sel = np.flatnonzero(~n4 & (v4 > -200))
    assert np.all(p[sel] >= 0) and 0 < len(sel) < np.count_nonzero(p >= 0)
    _check_null_a(pr, [served(d, 0, p)], sel, fact, maxcol=(v4, n4))


def _check_null_a(pr, keycols, sel, fact, maxcol=None):
    """check() where the qual does not drop a NULL a: psum(int8 a) skips it"""
    a_saved = fact.a
    fact.a = np.where(fact.an, 0, fact.a).astype(np.int32)
    try:
        return check(pr, keycols, sel, fact, maxcol=maxcol)
    finally:
        fact.a = a_saved


@pytest.mark.parametrize("jt", ["left", "anti"])
def test_an_outer_only_qual_runs_before_the_probe(jt):
    d = one_dim()
    n = 20011
    fact = Fact([d], n, 7003, a_range=(-1000, 1000))
    qual = "(int4gt (var 2 int4) (const int4 -300))"
    if jt == "left":
        spec = "(gpupreagg (qual " + qual + ") (key (var 1 int4)) " + AGG3 + " (pmax (var 4 int4)))"
    else:
        spec = "(gpupreagg (qual " + qual + ") (key (var 1 int4)) " + AGG3 + ")"
    st, pr, _ = run(fact, [jt], spec, one_columns(fact, jt), [(0, NG + 1)], ext=())
    assert st == 0
    p = fact.partners()[0]
    folded = fold_rule([p], [jt])
    sel = np.flatnonzero(folded & ~fact.an & (fact.a > -300))
    assert 0 < len(sel) < np.count_nonzero(folded)                     # the selection is strictly between
    if jt == "left":
        check(pr, [served(d, 0, p)], sel, fact, maxcol=served(d, 1, p))
    else:
        check(pr, [(fact.g, np.zeros(n, dtype=bool))], sel, fact)


# ---------------------------------------------------------------------------------------------
# case 7: errors are raised for folded rows only
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jt,partner,recheck", [("left", False, True), ("anti", False, True),
                                                ("anti", True, False), ("semi", False, False)])
def test_an_overflow_in_the_qual_counts_only_for_a_folded_row(jt, partner, recheck):
    d = one_dim()
    n = 9001
    rng = np.random.default_rng(7007)
    fact = Fact([d], n, 7009, nulls=False, a_range=(-500, 500))
    k = d.key[rng.integers(0, d.nd, n)].astype(np.int32)
    hole = np.setdiff1d(np.arange(d.key_lo, d.key_lo + d.span), d.key)
    k[::3] = hole[rng.integers(0, len(hole), len(k[::3]))]            # a third of the rows have no partner
    bad = 4321
    fact.a[bad] = 1000                          # 1000 + 2147483000 leaves int4
    k[bad] = d.key[7] if partner else hole[0]
    fact.fk = [(k, np.zeros(n, dtype=bool))]
    if jt == "left":
        spec = "(gpupreagg (qual " + OVERFLOW_QUAL + ") (key (var 1 int4)) " + AGG3 + " (pmax (var 4 int4)))"
    else:
        spec = "(gpupreagg (qual " + OVERFLOW_QUAL + ") (key (var 1 int4)) " + AGG3 + ")"
    st, pr, _ = run(fact, [jt], spec, one_columns(fact, jt), [(0, NG + 1)], ext=())
    p = fact.partners()[0]
    assert (p[bad] >= 0) == partner
    folded = fold_rule([p], [jt])
    assert folded[bad] == recheck
    if recheck:
        assert st == CPU_RECHECK
        return
    assert st == 0
    sel = np.flatnonzero(folded)                # (every other row passes: a + 2147483000 > 0)
    assert bad not in sel and len(sel) > 0
    check(pr, [(fact.g, np.zeros(n, dtype=bool))], sel, fact)


# ---------------------------------------------------------------------------------------------
# case 8: a text fact column in the WHERE, a LEFT relation
# ---------------------------------------------------------------------------------------------
def test_a_text_fact_column_in_the_where_with_a_left_relation():
    import test_lookup_text_gpu as tx
    runtime.init()
    d1, _ = tx.dims()
    fact = tx.Fact(5003, 8001, [d1])
    qual, ext, passes = tx.QUALS["texteq"]
    ds = runtime.DeviceStore.upload(fact.chunk())
    joins = open_joins([d1], [1])
    agg = GpuPreAgg(tx.spec_of("texteq"))
    try:
        agg.begin([(0, tx.NGROUPS)], ext_params=list(ext))
        assert agg.collect(agg.submit_lookup_typed(joins, ["left"], ds, tx.ONE_COLUMNS))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        joins[0].end()
        ds.release()
    p = fact.partners()[0]
    sel = np.flatnonzero(passes(fact, None, None))
    assert np.count_nonzero(p[sel] < 0) > 0 and np.count_nonzero(p[sel] >= 0) > 0
    gv, gn = served(d1, 0, p)
    uk, inv = model_groups([(gv[sel], gn[sel])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk) and NULLKEY in uk[:, 0]
    check_count_and_sums(cols, inv, len(uk), fact.a[sel], fact.b[sel])


# ---------------------------------------------------------------------------------------------
# case 9: the same queries through the join with a (jointype ...) program, the COLUMN projection
# and a plain fold
# ---------------------------------------------------------------------------------------------
def _same_rows(got, want, nkeys, has_max):
    (ks, cs), (kp, cp) = partial_rows(got, nkeys), partial_rows(want, nkeys)
    assert len(ks) > 1 and np.array_equal(ks, kp)
    assert np.array_equal(cs[0][0], cp[0][0]) and np.array_equal(cs[1][0], cp[1][0])
    assert np.allclose(cs[2][0], cp[2][0], rtol=1e-12, atol=0)
    if has_max:
        assert np.array_equal(cs[3][1], cp[3][1])
        assert np.array_equal(cs[3][0][~cs[3][1]], cp[3][0][~cp[3][1]])


@pytest.mark.parametrize("jt", ["left", "semi", "anti"])
def test_one_relation_agrees_with_the_join_projection_and_plain_fold(jt):
    d = one_dim()
    fact = Fact([d], 50021, 9001)
    spec = LEFT_SPEC if jt == "left" else FACTKEY_SPEC
    columns = one_columns(fact, jt)
    runtime.init()
    ds = runtime.DeviceStore.upload(fact.chunk())
    join = GpuHashJoin(jm.one_rel_spec(jt)).begin(build_multihash([(d.chunk(), [1])]))
    try:
        st, pr, _ = run(fact, [jt], spec, columns, [(0, NG + 1)], ds=ds)
        assert st == 0
        joined, nitems = join.join_to_column(ds, columns)
        plain = GpuPreAgg(spec)
        try:
            plain.begin([(0, NG + 1)], ext_params=EXT)
            assert plain.fold(joined)[0] == 0
            want = plain.fetch()
        finally:
            plain.end()
            joined.release()
    finally:
        join.end()
        ds.release()
    assert nitems == np.count_nonzero(fold_rule(fact.partners(), [jt]))
    _same_rows(pr, want, 1, jt == "left")


def test_left_and_anti_agree_with_the_two_relation_join_projection_and_plain_fold():
    d1, d2 = two_dims()
    fact = Fact([d1, d2], 50021, 9003)
    columns = [(1, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]
    runtime.init()
    ds = runtime.DeviceStore.upload(fact.chunk())
    both = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (jointype left))"
                       " (rel (hashkey (var 2 int4) 1 int4) (jointype anti)))")
    both.begin(build_multihash([(d1.chunk(), [1]), (d2.chunk(), [1])]))
    try:
        st, pr, _ = run(fact, ["left", "anti"], FACTKEY_SPEC, columns, [(0, NG)], ds=ds)
        assert st == 0
        joined, nitems = both.join_to_column(ds, columns)
        plain = GpuPreAgg(FACTKEY_SPEC)
        try:
            plain.begin([(0, NG)], ext_params=EXT)
            assert plain.fold(joined)[0] == 0
            want = plain.fetch()
        finally:
            plain.end()
            joined.release()
    finally:
        both.end()
        ds.release()
    assert nitems == np.count_nonzero(fold_rule(fact.partners(), ["left", "anti"]))
    _same_rows(pr, want, 1, False)


# ---------------------------------------------------------------------------------------------
# case 10: all inner is the existing call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrels", [1, 2])
def test_all_inner_gives_the_partial_rows_of_the_existing_calls(nrels):
    d1, d2 = two_dims()
    dims = [d1, d2][:nrels]
    fact = Fact(dims, 30011, 10001, exact_b=True)   # (float8 inputs that sum exactly in any order)
    columns = [(1, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]
    st, pt, _ = run(fact, ["inner"] * nrels, FACTKEY_SPEC, columns, [(0, NG)])
    st2, pe, _ = run(fact, [0] * nrels, FACTKEY_SPEC, columns, [(0, NG)], call=("lookup" if nrels == 1 else "star"))
    assert st == 0 and st2 == 0
    # bit for bit, floats included
    (kt, ct), (ke, ce) = partial_rows(pt, 1), partial_rows(pe, 1)
    assert len(kt) > 1 and np.array_equal(kt, ke) and len(ct) == len(ce) == 3
    for (vt, nt), (ve, ne) in zip(ct, ce):
        assert np.array_equal(nt, ne) and np.array_equal(vt, ve)
    sel = np.flatnonzero(fold_rule(fact.partners(), ["inner"] * nrels) & qual_passes(fact))
    check(pt, [served(d1, 0, fact.partners()[0])], sel, fact)


# ---------------------------------------------------------------------------------------------
# case 11: refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_session_usable():
    runtime.init()
    d1, d2 = two_dims()
    fact = Fact([d1, d2], 5003, 11001)
    ds = runtime.DeviceStore.upload(fact.chunk())
    joins = open_joins([d1, d2], [1, 2])
    j_left = GpuHashJoin(jm.one_rel_spec("left")).begin(build_multihash([(d1.chunk(), [1])]))
    # (a RIGHT join's table: the inner program with (track_matches))
    j_full = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (jointype inner) (track_matches)))").begin(
        build_multihash([(d1.chunk(), [1])]))
    spec = LEFT_SPEC.replace("(var 4 int4)", "(var 4 float8)")
    columns = [(1, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8"), (2, 2, "float8")]
    agg = GpuPreAgg(spec).begin([(0, NG)], ext_params=EXT)
    hashed = GpuPreAgg(spec).begin_hashed(ext_params=EXT)

    def refused(owner, tbls, jts, cols):
        with pytest.raises(runtime.StromError) as ei:
            owner.submit_lookup_typed(tbls, jts, ds, cols)
        assert ei.value.errcode == BAD_REQUEST, ei.value

    try:
        refused(agg, joins, [1, 4], columns)                            # a join type of 4
        refused(agg, joins, [-1, 1], columns)
        refused(agg, joins, ["left", "semi"], columns)                  # a column under a semi relation
        refused(agg, joins, ["anti", "left"], columns)                  # ... under an anti relation
        refused(agg, [joins[1]], ["anti"], [(1, 2, "float8")] + columns[1:3] + [(0, fact.A, "int4")])
        refused(agg, [j_left, joins[1]], ["left", "left"], columns)     # a table of a (jointype left) program
        refused(agg, [j_full, joins[1]], ["left", "left"], columns)     # a tracked table
        refused(hashed, joins, ["left", "left"], columns)               # a hashed session
        refused(agg, joins + joins + [joins[0]], ["left"] * 5, columns)  # more than 4 relations
        # nothing was folded (the counts below would show it), and the session still works
        assert agg.collect(agg.submit_lookup_typed(joins, ["left", "left"], ds, columns))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        hashed.end()
        for j in joins + [j_left, j_full]:
            j.end()
        ds.release()
    p1, p2 = fact.partners()
    sel = np.flatnonzero(qual_passes(fact))
    check(pr, [served(d1, 0, p1)], sel, fact, maxcol=served(d2, 0, p2))


# ---------------------------------------------------------------------------------------------
# integer sums the range proof does not cover: the typed mapping's own checked program
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jts", [("left",), ("left", "anti")])
def test_a_chunk_whose_integer_sums_are_unproven_is_folded_by_the_checked_typed_program(jts):
    """int8 inputs near 2^56 (test_star_lookup_gpu.py's last case): the chunk is folded again by the
    program built with GPUPREAGG_CHECKED behind the SAME define block -- for one typed relation too,
    where an inner lookup would retry with the session's own source, whose kernel knows no join type"""
    runtime.init()
    n = 6007
    dims = list(two_dims())[:len(jts)]
    rng = np.random.default_rng(12001)
    fk = [d.fact_keys(rng, n, True) for d in dims]
    x = (rng.integers(2**55, 2**56, n) * np.where(np.arange(n) % 2 == 0, 1, -1)).astype(np.int64)
    fact = kds.build_kds("column", [kds.Column("int4", k, kn) for k, kn in fk] + [kds.Column("int8", x)])
    spec = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)))"
    columns = [(1, 2, "int4"), (0, len(dims) + 1, "int8")]
    ds = runtime.DeviceStore.upload(fact)
    joins = open_joins(dims, list(range(1, len(dims) + 1)))
    agg = GpuPreAgg(spec)
    try:
        agg.begin([(0, NG)])
        st = agg.collect(agg.submit_lookup_typed(joins, list(jts), ds, columns))[0]
        checked = agg.checked_folds()
        pr = agg.fetch()
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    assert st == 0 and checked >= 1
    p = [d.partner(k, kn) for d, (k, kn) in zip(dims, fk)]
    sel = np.flatnonzero(fold_rule(p, jts))
    assert np.count_nonzero(p[0][sel] < 0) > 0                          # partner-less rows in the NULL group
    gv, gn = served(dims[0], 0, p[0])
    uk, inv = model_groups([(gv[sel], gn[sel])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    assert np.array_equal(cols[0][0], np.bincount(inv, minlength=len(uk)))
    want = [0] * len(uk)
    for g, v in zip(inv, x[sel]):
        want[g] += int(v)
    assert all(-2**63 <= w < 2**63 for w in want)
    assert [int(v) for v in cols[1][0]] == want
