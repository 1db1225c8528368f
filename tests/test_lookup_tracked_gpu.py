"""
RIGHT and FULL joins in the fused lookup and star folds: ONE tracked relation of the mapping, matched flags
by slot that the session owns, and the unmatched pass after the last chunk
(strom_submit_gpupreagg_lookup_tracked / _lookup_unmatched; gpupreagg_dense_lookup / _packed_lookup with
GPUPREAGG_LOOKUP_TRACK, the _star kernels with GPUPREAGG_STAR_TRACK_REL, gpupreagg_dense_lookup_unmatched;
needs an MI355X: -m gpu).  The parent of this change has no such symbol: every test here fails there
(GpuPreAgg has no submit_lookup_tracked) -- test 9, tracked = 0, included, though what it pins is the
typed call's own behaviour.

The model is tests/tracked_fold_model.py (test_lookup_tracked_cpu.py holds it against the nested-loop
unmatched model): the per-chunk fold is the typed fold; a row of the tracked dimension is matched when a fact
row has it as its partner and survives every other relation, whatever the WHERE says of that row; the
unmatched pass emits every other row once, its own columns from the slot record, everything else NULL.

What the kernels can get wrong is, as ever, a row whose probe was masked: it reads slot 0 and flag 0.  So
the first data set leaves the slot-0 row of the tracked dimension without a partner while NULL and
out-of-range keys exist -- a masked row that stored would flag it, and it would be missing from the unmatched
pass -- and the second one matches it.  Every data set asserts the cases it is there for before the device runs.

Bars, the project's (test_lookup_join_types_gpu.py): keys, counts, integer sums and min / max bit-exact;
float8 sums rtol 1e-12 (a group sums at most ~1e3 values of [0, 1) here); the flag image byte for byte;
tracked = 0 against the typed call with float8 inputs that sum exactly (multiples of 2^-20), bit for bit.
"""
import numpy as np
import pytest

import tracked_fold_model as tm
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpupreagg import GpuPreAgg, lookup_tracked_defines, lookup_typed_defines, lookup_unmatched_defines
from test_lookup_join_types_gpu import AGG3, NG, Fact, one_dim, served
from test_star_lookup_gpu import (BAD_REQUEST, CPU_RECHECK, EXT, OVERFLOW_QUAL, QUAL, TILE_ROWS, Dim, open_joins,
                                  partial_rows, two_dims)

pytestmark = pytest.mark.gpu

N = 3 * TILE_ROWS + 5                           # rows of a fact chunk: three tiles and a ragged tail
ISNULL_QUAL = "(isnull (var 2 int4))"


def spec_of(qual=None, maxtype="int4", mintype=None):
    s = "(gpupreagg " + ("(qual " + qual + ") " if qual else "") + "(key (var 1 int4)) " + AGG3
    s += " (pmax (var 4 %s))" % maxtype if maxtype else ""
    s += " (pmin (var 5 %s))" % mintype if mintype else ""
    return s + ")"


QUAL_MODELS = {
    None: lambda r: np.ones(r.n, dtype=bool),
    QUAL: lambda r: (~r.cols["a"][1]) & (r.cols["a"][0] < EXT[0]) & (~r.cols["b"][1]) & (r.cols["b"][0] > EXT[1]),
    ISNULL_QUAL: lambda r: r.cols["a"][1].copy(),
    OVERFLOW_QUAL: lambda r: (~r.cols["a"][1]) & (r.cols["a"][0].astype(np.int64) + 2147483000 > 0),
}


# ---------------------------------------------------------------------------------------------
# data: a fact table whose keys leave some rows of the tracked dimension without a partner
# ---------------------------------------------------------------------------------------------
def holes_of(d):
    return np.setdiff1d(np.arange(d.key.min(), d.key.max() + 1), d.key)


def unreferenced(d, seed, slot0):
    """about 20 % of the dimension's rows, the slot-0 row (the smallest key) among them or not"""
    rng = np.random.default_rng(seed)
    u = rng.random(d.nd) < 0.2
    u[int(np.argmin(d.key))] = slot0
    return u


def reroute(fact, r, unref, seed):
    """the keys of relation r + 1 that name a row in `unref` go to a hole of the key range instead"""
    d = fact.dims[r]
    rng = np.random.default_rng(seed)
    k, kn = fact.fk[r]
    p = d.partner(k, kn)
    hit = (p >= 0) & unref[np.clip(p, 0, d.nd - 1)]
    holes = holes_of(d)
    k = k.copy()
    k[hit] = holes[rng.integers(0, len(holes), np.count_nonzero(hit))].astype(k.dtype)
    fact.fk[r] = (k, kn)


def one_fact(d, n, seed, slot0_matched, **kw):
    fact = Fact([d], n, seed, **kw)
    unref = unreferenced(d, seed + 1, not slot0_matched)
    reroute(fact, 0, unref, seed + 2)
    if slot0_matched and n >= 1:                # (a random key may never name it: one row does)
        k, kn = fact.fk[0]
        k[n // 2], kn[n // 2] = d.key.min(), False
    return fact


def assert_cases(d, facts, matched, slot0_matched):
    """the cases a data set is there for (the issue's list), before the device runs"""
    s0 = int(np.argmin(d.key))
    unmatched = tm.unmatched_rows(d, matched)
    assert len(matched) > 0 and len(unmatched) > 0 and len(holes_of(d)) > 0
    assert (s0 in matched) == slot0_matched
    k = np.concatenate([f.fk[0][0] for f in facts]).astype(np.int64)
    kn = np.concatenate([f.fk[0][1] for f in facts])
    assert kn.any() and (~kn & (k < d.key.min())).any() and (~kn & (k > d.key.max())).any()    # masked rows
    assert np.isin(k[~kn], holes_of(d)).any()                                                # a probed hole


def one_rows(fact, d, p, keep, third=False):
    """the virtual rows of one folded chunk: the dimension's columns by partner, the fact's own"""
    cols = {"key": served(d, 0, p), "a": (fact.a, fact.an), "b": (fact.b, np.zeros(fact.n, dtype=bool))}
    if len(d.cols) > 1:
        cols["mx"] = served(d, 1, p)
    if third:
        cols["mn"] = served(d, 2, p)
    return tm.Rows(**cols).take(np.flatnonzero(keep))


def one_unmatched_rows(d, rows, third=False):
    n = len(rows)
    cols = {"key": tm.served_rows(d, 0, rows), "a": tm.null_column(n), "b": tm.null_column(n, np.float64)}
    if len(d.cols) > 1:
        cols["mx"] = tm.served_rows(d, 1, rows)
    if third:
        cols["mn"] = tm.served_rows(d, 2, rows)
    return tm.Rows(**cols)


def want_of(rows, qual, d, third=False):
    rows = rows.take(np.flatnonzero(QUAL_MODELS[qual](rows)))
    return tm.aggregate(rows, mx="mx" if len(d.cols) > 1 else None, mn="mn" if third else None)


def one_columns(fact, d, third=False):
    cols = [(1, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]
    if len(d.cols) > 1:
        cols.append((1, 3, d.cols[1][0]))
    if third:
        cols.append((1, 4, d.cols[2][0]))
    return cols


class Query(object):
    """one session over open tables and uploaded chunks"""

    def __init__(self, dims, facts, spec, domain, ext=(), joins=None):
        runtime.init()
        self.stores = [runtime.DeviceStore.upload(f.chunk()) for f in facts]
        self.own_joins = joins is None
        self.joins = open_joins(dims, list(range(1, len(dims) + 1))) if joins is None else joins
        self.agg = GpuPreAgg(spec)
        self.agg.begin(domain, ext_params=list(ext))

    def fold(self, i, jts, tracked, columns):
        return self.agg.collect(self.agg.submit_lookup_tracked(self.joins, jts, tracked, self.stores[i], columns))[0]

    def unmatched(self, jts, tracked, columns):
        return self.agg.collect(self.agg.submit_lookup_unmatched(self.joins, jts, tracked, columns))[0]

    def rows(self):
        return partial_rows(self.agg.fetch(), 1)

    def close(self):
        self.agg.end()
        if self.own_joins:
            for j in self.joins:
                j.end()
        for s in self.stores:
            s.release()


def one_table_case(jt, form, slot0_matched, qual=None, seed=20001, n=N):
    d = one_dim(form)
    third = len(d.cols) > 2
    fact = one_fact(d, n, seed, slot0_matched)
    p = fact.partners()[0]
    matched, (keep,), unmatched = tm.tracked_model([[p]], [d], [jt], 1)
    if n > 1:
        assert_cases(d, [fact], matched, slot0_matched)
    spec = spec_of(qual, d.cols[1][0] if len(d.cols) > 1 else None, d.cols[2][0] if third else None)
    columns = one_columns(fact, d, third)
    q = Query([d], [fact], spec, [(0, NG + 1)], ext=EXT if qual == QUAL else ())
    try:
        assert q.fold(0, [jt], 1, columns) == 0
        folded = one_rows(fact, d, p, keep, third)
        tm.check_partial_rows(*q.rows(), want_of(folded, qual, d, third))
        img = q.agg.lookup_matches()
        assert img.dtype == np.uint8 and np.array_equal(img, tm.matches_image(d, matched))
        assert q.unmatched([jt], 1, columns) == 0
        both = tm.Rows.concat([folded, one_unmatched_rows(d, unmatched, third)])
        tm.check_partial_rows(*q.rows(), want_of(both, qual, d, third))
        assert np.array_equal(q.agg.lookup_matches(), img)      # the pass reads the flags, it sets none
        defines = q.agg.mapping_defines()
    finally:
        q.close()
    return d, fact, matched, unmatched, defines


# form -> (slot record length, narrow?, the virtual columns the dimension serves)
RECORD_FORMS = {"narrow2": (2, True, [0, 3]), "narrow4": (4, True, [0, 3]), "wide16": (16, False, [0, 3]),
                "wide32": (32, False, [0, 3, 4])}


# ---------------------------------------------------------------------------------------------
# test 1: one table, RIGHT and FULL, every record form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["narrow2", "narrow4", "wide16", "wide32"])
@pytest.mark.parametrize("jt", ["inner", "left"])
def test_one_table_right_and_full_with_every_record_form(jt, form, monkeypatch):
    """GROUP BY the dimension's column: nrows, psum(int8 fact.a), psum(fact.b), pmax of a dimension column
    (and pmin of a third one where the record has 32 bytes).  fetch() after the fold, the flag image, and
    fetch() after fold + unmatched, against the model.  The slot-0 row is unmatched here."""
    if form == "wide16":
        monkeypatch.setenv("STROM_HASHJOIN_NO_NARROW_RECS", "1")
    _, _, _, _, defines = one_table_case(jt, form, slot0_matched=False)
    rel = (4,) + RECORD_FORMS[form]
    assert sorted(defines) == sorted([lookup_tracked_defines([rel], [jt], 1), lookup_unmatched_defines(rel)]), defines


@pytest.mark.parametrize("jt", ["inner", "left"])
def test_the_slot_0_row_matched(jt):
    """the second data set: a fact row names the smallest key, so slot 0 is flagged and stays out of the pass"""
    one_table_case(jt, "narrow4", slot0_matched=True, seed=20101)


def test_a_chunk_of_one_row():
    """one row, one partner: exactly one flag, every other present slot comes out of the pass"""
    d = one_dim("narrow4")
    _, fact, matched, unmatched, _ = one_table_case("inner", "narrow4", slot0_matched=True, seed=20201, n=1)
    assert len(matched) == 1 and matched[0] == int(np.argmin(d.key)) and len(unmatched) == d.nd - 1


# ---------------------------------------------------------------------------------------------
# test 2: the WHERE does not decide a match
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qual", [QUAL, ISNULL_QUAL])
def test_a_row_the_where_rejects_still_matches_its_slot(qual):
    """a strict qual over fact columns (which an untracked program evaluates before the probe) and a
    non-strict one: fact RIGHT JOIN dim WHERE fact.a IS NULL, the anti-join from the right, which keeps the
    unmatched rows.  Row Q of the dimension has partner rows, and the qual rejects every one of them: Q is
    flagged and does not come out of the unmatched pass."""
    d = one_dim("narrow4")
    fact = one_fact(d, N, 20301, slot0_matched=False)
    p = fact.partners()[0]
    Q = int(p[p >= 0][7])
    mine = (p == Q)
    fact.a[mine], fact.an[mine] = 2**30 + 5, False          # not NULL, and not below the parameter
    matched, (keep,), unmatched = tm.tracked_model([[p]], [d], ["inner"], 1)
    assert_cases(d, [fact], matched, False)
    folded = one_rows(fact, d, p, keep)
    assert mine.any() and Q in matched and Q not in unmatched
    assert not QUAL_MODELS[qual](one_rows(fact, d, p, mine)).any()      # every partner row of Q is rejected
    assert 0 < np.count_nonzero(QUAL_MODELS[qual](folded)) < folded.n
    columns = one_columns(fact, d)
    q = Query([d], [fact], spec_of(qual), [(0, NG + 1)], ext=EXT if qual == QUAL else ())
    try:
        assert q.fold(0, ["inner"], 1, columns) == 0
        tm.check_partial_rows(*q.rows(), want_of(folded, qual, d))
        img = q.agg.lookup_matches()
        assert img[tm.slot_of(d, np.array([Q]))[0]] == 1
        assert np.array_equal(img, tm.matches_image(d, matched))
        assert q.unmatched(["inner"], 1, columns) == 0
        rest = one_unmatched_rows(d, unmatched)
        # the strict qual drops every unmatched row (its fact columns are NULL), the non-strict one keeps them
        assert QUAL_MODELS[qual](rest).all() == (qual == ISNULL_QUAL)
        tm.check_partial_rows(*q.rows(), want_of(tm.Rows.concat([folded, rest]), qual, d))
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------
# test 3: three chunks, a reset, a rescan
# ---------------------------------------------------------------------------------------------
def test_three_chunks_then_a_reset_and_a_rescan():
    d = one_dim("narrow4")
    facts = [one_fact(d, N, 20401 + 10 * i, slot0_matched=False) for i in range(3)]
    # row M is matched in the second chunk only
    p0 = facts[1].partners()[0]
    M = int(p0[p0 >= 0][11])
    for i in (0, 2):
        u = np.zeros(d.nd, dtype=bool)
        u[M] = True
        reroute(facts[i], 0, u, 20491 + i)
    ps = [f.partners()[0] for f in facts]
    assert not (ps[0] == M).any() and (ps[1] == M).any() and not (ps[2] == M).any()
    matched, keeps, unmatched = tm.tracked_model([[p] for p in ps], [d], ["left"], 1)
    assert_cases(d, facts, matched, False)
    assert M in matched
    columns = one_columns(facts[0], d)
    q = Query([d], facts, spec_of(), [(0, NG + 1)])
    try:
        for i in range(3):
            assert q.fold(i, ["left"], 1, columns) == 0
        assert np.array_equal(q.agg.lookup_matches(), tm.matches_image(d, matched))
        assert q.unmatched(["left"], 1, columns) == 0
        parts = [one_rows(f, d, p, k) for f, p, k in zip(facts, ps, keeps)]
        tm.check_partial_rows(*q.rows(), want_of(tm.Rows.concat(parts + [one_unmatched_rows(d, unmatched)]), None, d))
        # a rescan: the flags cleared, the pass re-armed (the partial rows are the session's: reset too)
        q.agg.reset_lookup_matches()
        q.agg.reset()
        assert not q.agg.lookup_matches().any()
        assert q.fold(0, ["left"], 1, columns) == 0
        m1, (k1,), u1 = tm.tracked_model([[ps[0]]], [d], ["left"], 1)
        assert M in u1
        assert np.array_equal(q.agg.lookup_matches(), tm.matches_image(d, m1))
        assert q.unmatched(["left"], 1, columns) == 0
        tm.check_partial_rows(*q.rows(), want_of(tm.Rows.concat([parts[0], one_unmatched_rows(d, u1)]), None, d))
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------
# test 4: no chunk at all
# ---------------------------------------------------------------------------------------------
def test_no_chunk_at_all_emits_every_present_slot():
    d = one_dim("narrow4")
    fact = one_fact(d, 1, 20501, slot0_matched=False)       # (never folded: it names the columns)
    columns = one_columns(fact, d)
    q = Query([d], [], spec_of(), [(0, NG + 1)])
    try:
        assert q.unmatched(["inner"], 1, columns) == 0
        keys, cols = q.rows()
        want = want_of(one_unmatched_rows(d, np.arange(d.nd)), None, d)
        tm.check_partial_rows(keys, cols, want)
        assert cols[0][0].sum() == d.nd                         # nrows counts every row of the dimension
        assert cols[1][1].all() and cols[2][1].all()            # the sums over fact columns are NULL
        assert not q.agg.lookup_matches().any()
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------
# test 5: stars
# ---------------------------------------------------------------------------------------------
_EXTRA = {}


def filter_dims():
    """two dimensions without columns, for the semi and the anti relation (computed once, left unchanged)"""
    if not _EXTRA:
        rng = np.random.default_rng(20601)
        _EXTRA["d"] = (Dim(rng, 3000, key_lo=40), Dim(rng, 3000, key_lo=-90, holes=2.5))
    return _EXTRA["d"]


def star_rows(fact, d1, p1, keep, d2=None, p2=None):
    cols = {"key": served(d1, 0, p1), "a": (fact.a, fact.an), "b": (fact.b, np.zeros(fact.n, dtype=bool))}
    if d2 is not None:
        cols["mx"] = served(d2, 0, p2)
    return tm.Rows(**cols).take(np.flatnonzero(keep))


def star_unmatched_rows(d1, rows, with_max):
    n = len(rows)
    cols = {"key": tm.served_rows(d1, 0, rows), "a": tm.null_column(n), "b": tm.null_column(n, np.float64)}
    if with_max:
        cols["mx"] = tm.null_column(n, np.float64)              # another relation's column: NULL
    return tm.Rows(**cols)


def test_star_semi_tracked_inner_anti():
    """(fact SEMI dS ANTI dA) RIGHT JOIN d1: row Z of d1 has partner rows, and the semi relation drops every
    one of them -- Z is unmatched; so is a row whose partner rows the anti relation drops"""
    d1, _ = two_dims()
    dS, dA = filter_dims()
    dims, jts, tracked = [dS, d1, dA], ["semi", "inner", "anti"], 2
    fact = Fact(dims, N, 20611)
    reroute(fact, 1, unreferenced(d1, 20613, True), 20615)
    p = fact.partners()
    Z, Y = int(p[1][p[1] >= 0][5]), int(p[1][p[1] >= 0][9])
    assert Z != Y
    kS, kSn = fact.fk[0]
    kSn[p[1] == Z] = True                                       # no semi partner: a NULL key
    kA, kAn = fact.fk[2]
    kA[p[1] == Y], kAn[p[1] == Y] = dA.key[3], False            # an anti partner
    p = fact.partners()
    matched, (keep,), unmatched = tm.tracked_model([p], dims, jts, tracked)
    assert (p[1] == Z).any() and (p[1] == Y).any() and Z in unmatched and Y in unmatched
    assert int(np.argmin(d1.key)) in unmatched and 0 < len(matched) < d1.nd
    assert 0 < np.count_nonzero(keep) < np.count_nonzero(p[1] >= 0)
    columns = [(2, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8")]
    q = Query(dims, [fact], spec_of(None, None), [(0, NG)])
    try:
        assert q.fold(0, jts, tracked, columns) == 0
        folded = star_rows(fact, d1, p[1], keep)
        tm.check_partial_rows(*q.rows(), tm.aggregate(folded))
        assert np.array_equal(q.agg.lookup_matches(), tm.matches_image(d1, matched))
        assert q.unmatched(jts, tracked, columns) == 0
        tm.check_partial_rows(*q.rows(), tm.aggregate(tm.Rows.concat([folded, star_unmatched_rows(d1, unmatched, False)])))
    finally:
        q.close()


def test_star_left_tracked_left():
    """(fact LEFT d2) FULL JOIN d1: every fact row is folded; d2's column is NULL in the unmatched rows"""
    d1, d2 = two_dims()
    dims, jts, tracked = [d2, d1], ["left", "left"], 2
    fact = Fact(dims, N, 20631)
    reroute(fact, 1, unreferenced(d1, 20633, True), 20635)
    p = fact.partners()
    matched, (keep,), unmatched = tm.tracked_model([p], dims, jts, tracked)
    assert keep.all() and int(np.argmin(d1.key)) in unmatched and 0 < len(matched) < d1.nd
    k1, k1n = fact.fk[1]
    assert k1n.any() and (~k1n & (k1 < d1.key.min())).any() and (~k1n & (k1 > d1.key.max())).any()
    columns = [(2, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8"), (1, 2, "float8")]
    q = Query(dims, [fact], spec_of(None, "float8"), [(0, NG)])
    try:
        assert q.fold(0, jts, tracked, columns) == 0
        folded = star_rows(fact, d1, p[1], keep, d2, p[0])
        tm.check_partial_rows(*q.rows(), tm.aggregate(folded, mx="mx"))
        assert np.array_equal(q.agg.lookup_matches(), tm.matches_image(d1, matched))
        assert q.unmatched(jts, tracked, columns) == 0
        both = tm.Rows.concat([folded, star_unmatched_rows(d1, unmatched, True)])
        tm.check_partial_rows(*q.rows(), tm.aggregate(both, mx="mx"))
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------
# test 6: one work-group walks many tiles of slots
# ---------------------------------------------------------------------------------------------
_BIG = {}


def big_dim():
    """three tiles of slots and a ragged tail; the 4-byte narrow record of one_dim("narrow4")"""
    if not _BIG:
        rng = np.random.default_rng(20701)
        nd = int((3 * TILE_ROWS + 400) / 1.25)
        d = Dim(rng, nd, key_lo=-700, holes=1.25)
        d.add("int4", (d.key % NG).astype(np.int32), rng.random(nd) < 0.04)
        d.add("int4", rng.integers(-1000, 1000, nd).astype(np.int32), rng.random(nd) < 0.05)
        _BIG["d"] = d
    return _BIG["d"]


@pytest.mark.parametrize("max_grid", ["1", "2"])
def test_a_work_group_walks_several_tiles_of_slots(max_grid, monkeypatch):
    monkeypatch.setenv("STROM_GPUPREAGG_UNMATCHED_MAX_GRID", max_grid)
    d = big_dim()
    nslots = int(d.key.max() - d.key.min()) + 1
    assert nslots > 3 * TILE_ROWS and nslots % TILE_ROWS != 0
    fact = one_fact(d, N, 20711, slot0_matched=False)
    p = fact.partners()[0]
    matched, (keep,), unmatched = tm.tracked_model([[p]], [d], ["inner"], 1)
    assert_cases(d, [fact], matched, False)
    slots = tm.slot_of(d, unmatched)
    assert all(((slots // TILE_ROWS) == t).any() for t in range(4))     # an unmatched row in every tile
    columns = one_columns(fact, d)
    q = Query([d], [fact], spec_of(), [(0, NG + 1)])
    try:
        assert q.fold(0, ["inner"], 1, columns) == 0
        assert q.unmatched(["inner"], 1, columns) == 0
        both = tm.Rows.concat([one_rows(fact, d, p, keep), one_unmatched_rows(d, unmatched)])
        tm.check_partial_rows(*q.rows(), want_of(both, None, d))
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------
# test 7: the seam -- two sessions fold the two halves of the rows
# ---------------------------------------------------------------------------------------------
def test_two_sessions_merge_their_flag_images():
    d = one_dim("narrow4")
    facts = [one_fact(d, N, 20801, slot0_matched=False), one_fact(d, N, 20811, slot0_matched=False)]
    reroute(facts[1], 0, unreferenced(d, 20802, True), 20821)      # (both leave the same rows alone)
    ps = [f.partners()[0] for f in facts]
    matched, keeps, unmatched = tm.tracked_model([[p] for p in ps], [d], ["inner"], 1)
    assert_cases(d, facts, matched, False)
    m0 = tm.matched_rows([[ps[0]]], ["inner"], 1)
    m1 = tm.matched_rows([[ps[1]]], ["inner"], 1)
    assert len(np.setdiff1d(m1, m0)) > 0 and len(np.setdiff1d(m0, m1)) > 0
    columns = one_columns(facts[0], d)
    joins = open_joins([d], [1])
    qs = [Query([d], fs, spec_of(), [(0, NG + 1)], joins=joins) for fs in ([facts[0]], [facts[1]], facts)]
    try:
        assert qs[0].fold(0, ["inner"], 1, columns) == 0 and qs[1].fold(0, ["inner"], 1, columns) == 0
        assert qs[2].fold(0, ["inner"], 1, columns) == 0 and qs[2].fold(1, ["inner"], 1, columns) == 0
        imgs = [q.agg.lookup_matches() for q in qs]
        assert np.array_equal(imgs[0], tm.matches_image(d, m0)) and np.array_equal(imgs[1], tm.matches_image(d, m1))
        assert np.array_equal(imgs[0] | imgs[1], imgs[2])
        # a wrong length and a byte of 2 are refused, and nothing is merged
        bad = imgs[1].copy()
        bad[int(np.flatnonzero(imgs[0] == 0)[0])] = 2
        for image in (imgs[1][:-1], np.concatenate([imgs[1], [0]]).astype(np.uint8), bad):
            with pytest.raises(runtime.StromError) as ei:
                qs[0].agg.merge_lookup_matches(image)
            assert ei.value.errcode == BAD_REQUEST
            assert np.array_equal(qs[0].agg.lookup_matches(), imgs[0])
        qs[0].agg.merge_lookup_matches(imgs[1])
        assert np.array_equal(qs[0].agg.lookup_matches(), imgs[2])
        assert qs[0].unmatched(["inner"], 1, columns) == 0
        # the first session: its own half folded, and the single session's unmatched rows
        first = tm.Rows.concat([one_rows(facts[0], d, ps[0], keeps[0]), one_unmatched_rows(d, unmatched)])
        tm.check_partial_rows(*qs[0].rows(), want_of(first, None, d))
        assert qs[2].unmatched(["inner"], 1, columns) == 0
        whole = tm.Rows.concat([one_rows(f, d, p, k) for f, p, k in zip(facts, ps, keeps)] +
                               [one_unmatched_rows(d, unmatched)])
        tm.check_partial_rows(*qs[2].rows(), want_of(whole, None, d))
    finally:
        for q in qs:
            q.close()
        joins[0].end()


# ---------------------------------------------------------------------------------------------
# test 8: a chunk that ends CpuReCheck has set its flags
# ---------------------------------------------------------------------------------------------
def test_a_chunk_that_ends_cpu_recheck_is_not_folded_and_its_flags_are_complete():
    d = one_dim("narrow4")
    fact = one_fact(d, N, 20901, slot0_matched=False, a_range=(-500, 500))
    p = fact.partners()[0]
    bad = int(np.flatnonzero((p >= 0) & ~fact.an)[len(fact.a) // 7])
    fact.a[bad] = 1000                          # 1000 + 2147483000 leaves int4, in a row that is folded
    matched, (keep,), _ = tm.tracked_model([[p]], [d], ["inner"], 1)
    assert_cases(d, [fact], matched, False)
    assert keep[bad] and bad < N - TILE_ROWS    # (rows behind the error still set their flags)
    columns = one_columns(fact, d)
    q = Query([d], [fact], spec_of(OVERFLOW_QUAL), [(0, NG + 1)])
    try:
        assert q.fold(0, ["inner"], 1, columns) == CPU_RECHECK
        assert len(q.agg.fetch()) == 0
        assert np.array_equal(q.agg.lookup_matches(), tm.matches_image(d, matched))
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------
# test 9: tracked = 0 is the typed call
# ---------------------------------------------------------------------------------------------
def test_nothing_tracked_is_the_typed_call_bit_for_bit():
    d = one_dim("narrow4")
    fact = one_fact(d, N, 21001, slot0_matched=False, exact_b=True)
    columns = one_columns(fact, d)
    spec = spec_of(QUAL)
    got = []
    for tracked_call in (False, True):
        q = Query([d], [fact], spec, [(0, NG + 1)], ext=EXT)
        try:
            if tracked_call:
                pending = q.agg.submit_lookup_tracked(q.joins, ["left"], 0, q.stores[0], columns)
            else:
                pending = q.agg.submit_lookup_typed(q.joins, ["left"], q.stores[0], columns)
            assert q.agg.collect(pending)[0] == 0
            got.append((q.rows(), q.agg.mapping_defines()))
            with pytest.raises(runtime.StromError):             # no flags were made
                q.agg.lookup_matches()
        finally:
            q.close()
    ((kt, ct), dt), ((kz, cz), dz) = got
    assert dt == dz == [lookup_typed_defines([(4, 4, True, [0, 3])], ["left"])]     # no new program
    assert len(kt) > 1 and np.array_equal(kt, kz) and len(ct) == len(cz) == 4
    for (vt, nt), (vz, nz) in zip(ct, cz):
        assert np.array_equal(nt, nz) and np.array_equal(vt[~nt], vz[~nz])


# ---------------------------------------------------------------------------------------------
# test 10: refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_session_usable():
    runtime.init()
    d1, d2 = two_dims()
    dims = [d2, d1]
    fact = Fact(dims, 5003, 21101)
    reroute(fact, 1, unreferenced(d1, 21103, True), 21105)
    p = fact.partners()
    columns = [(2, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8"), (1, 2, "float8")]
    spec = spec_of(None, "float8")
    # a dimension with a NULL key: that row has no slot
    nk = d1.key.astype(np.int32)
    nkn = np.zeros(d1.nd, dtype=bool)
    nkn[5] = True
    with_null = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", nk, nkn),
                                                            kds.Column("int4", d1.cols[0][1], d1.cols[0][2])]), [1])])
    j_null = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))").begin(with_null)
    j_tracked = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4) (jointype inner) (track_matches)))").begin(
        build_multihash([(d1.chunk(), [1])]))
    j_other = open_joins([d1], [2])[0]                          # the same dimension, another table
    q = Query(dims, [fact], spec, [(0, NG)])
    hashed = GpuPreAgg(spec).begin_hashed()
    ds, joins = q.stores[0], q.joins

    def refused(call, *args):
        with pytest.raises(runtime.StromError) as ei:
            call(*args)
        assert ei.value.errcode == BAD_REQUEST, ei.value

    try:
        refused(q.agg.lookup_matches)                                   # a session without flags
        refused(q.agg.merge_lookup_matches, np.zeros(8, dtype=np.uint8))
        refused(q.agg.reset_lookup_matches)
        t = q.agg.submit_lookup_tracked
        u = q.agg.submit_lookup_unmatched
        refused(t, joins, ["left", 4], 2, ds, columns)                  # what the typed call refuses
        refused(t, joins, ["semi", "left"], 2, ds, columns)             # ... a column under a semi relation
        refused(t, [joins[0], j_tracked], ["left", "left"], 2, ds, columns)     # ... a (track_matches) table
        refused(hashed.submit_lookup_tracked, joins, ["left", "left"], 2, ds, columns)
        refused(t, joins, ["left", "left"], -1, ds, columns)            # tracked outside 0 .. ntbls
        refused(t, joins, ["left", "left"], 3, ds, columns)
        refused(u, joins, ["left", "left"], 0, columns)                 # the pass needs a tracked relation
        refused(u, joins, ["left", "left"], 3, columns)
        semi_columns = [(2, 2, "int4"), (0, fact.A, "int4"), (0, fact.B, "float8"), (0, fact.B, "float8")]
        refused(t, joins, ["semi", "left"], 1, ds, semi_columns)        # a tracked semi relation
        refused(t, joins, ["anti", "left"], 1, ds, semi_columns)        # ... anti
        refused(u, joins, ["anti", "left"], 1, semi_columns)
        refused(t, [joins[0], j_null], ["left", "left"], 2, ds, columns)        # a NULL-key entry in the tracked table
        refused(u, [joins[0], j_null], ["left", "left"], 2, columns)
        assert lib_length(q.agg) == 0                                   # still no flags
        assert len(q.agg.fetch()) == 0                                  # and nothing was folded
        # the flags get bound by the first tracked fold
        assert q.fold(0, ["left", "left"], 2, columns) == 0
        refused(t, joins, ["left", "left"], 1, ds, columns)             # another position
        refused(t, [joins[0], j_other], ["left", "left"], 2, ds, columns)       # another table
        refused(u, [joins[0], j_other], ["left", "left"], 2, columns)
        before = q.agg.lookup_matches()
        assert q.unmatched(["left", "left"], 2, columns) == 0
        refused(u, joins, ["left", "left"], 2, columns)                 # a second pass without a reset
        refused(t, joins, ["left", "left"], 2, ds, columns)             # a fold after the pass without a reset
        assert np.array_equal(q.agg.lookup_matches(), before)
        keys, cols = q.rows()
    finally:
        q.close()
        hashed.end()
        for j in (j_null, j_tracked, j_other):
            j.end()
    # the counts: one fold and one pass, nothing else
    matched, (keep,), unmatched = tm.tracked_model([p], dims, ["left", "left"], 2)
    assert np.array_equal(before, tm.matches_image(d1, matched))
    both = tm.Rows.concat([star_rows(fact, d1, p[1], keep, d2, p[0]), star_unmatched_rows(d1, unmatched, True)])
    tm.check_partial_rows(keys, cols, tm.aggregate(both, mx="mx"))


def lib_length(agg):
    from pg_strom_amd._lib import lib
    return lib.strom_gpupreagg_lookup_matches_length(agg.session)


# ---------------------------------------------------------------------------------------------
# test 11: a coded text column -- RIGHT JOIN ... GROUP BY dim.name
# ---------------------------------------------------------------------------------------------
def test_group_by_the_dimensions_text_column_gives_every_name_a_group():
    import test_dim_text_lookup_gpu as tx
    from pg_strom_amd.textdict import TextDictionary
    runtime.init()
    d = tx.text_dim(21201, 400, tx.WORDS, null_ratio=0.1)
    rng = np.random.default_rng(21203)
    n = 5003
    k = (d.key_lo + rng.integers(-20, d.span + 20, n)).astype(np.int32)
    kn = rng.random(n) < 0.02
    # the rows that hold one chosen word are never referenced: that name has a group only through the pass
    lonely = d.words[int(np.flatnonzero(~d.tnull)[0])]
    unref = np.array([(w == lonely) for w in d.words]) | (rng.random(d.nd) < 0.2)
    p = d.partner(k, kn)
    hit = (p >= 0) & unref[np.clip(p, 0, d.nd - 1)]
    kn[hit] = True
    p = d.partner(k, kn)
    x = rng.integers(0, 1000, n).astype(np.int32)
    matched = tm.matched_rows([[p]], ["inner"], 1)
    unmatched = tm.unmatched_rows(d, matched)
    assert len(matched) > 0 and not any(d.words[i] == lonely for i in matched)
    dic = TextDictionary("text", nkeys_hint=64)
    join, coded = tx.encoded(d, dic)
    ds = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", k, kn), kds.Column("int4", x)]))
    agg = GpuPreAgg("(gpupreagg (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))))")
    columns = [(1, coded + 1, "int4"), (0, 2, "int4")]
    try:
        agg.begin([(0, max(dic.num_keys, 1))])
        assert agg.collect(agg.submit_lookup_tracked([join], ["inner"], 1, ds, columns))[0] == 0
        assert agg.collect(agg.submit_lookup_unmatched([join], ["inner"], 1, columns))[0] == 0
        pr = agg.fetch()
        names = dic.keys()
    finally:
        agg.end()
        join.end()
        dic.release()
        ds.release()
    (iv, inull), (cnt, _), (sx, sxn) = pr.column(0), pr.column(1), pr.column(2)
    got = {(None if nul else names[int(i)]): (int(c), None if sn else int(s))
           for i, nul, c, s, sn in zip(iv, inull, cnt, sx, sxn)}
    want = {}
    for i in p[p >= 0].tolist() + unmatched.tolist():
        want.setdefault(tx.key_of(d, i), [0, None])[0] += 1
    for i, v in zip(p[p >= 0].tolist(), x[p >= 0].tolist()):
        w = want[tx.key_of(d, i)]
        w[1] = v if w[1] is None else w[1] + v
    assert set(got) == set(want) == {tx.key_of(d, i) for i in range(d.nd)}      # every name of the dimension
    assert lonely in got and got[lonely][1] is None                             # ... also one without facts
    assert got == {name: tuple(v) for name, v in want.items()}
