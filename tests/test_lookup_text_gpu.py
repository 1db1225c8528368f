"""
Text / character(n) fact columns in the fused join-and-aggregate kernels (needs an MI355X: -m gpu):
strom_submit_gpupreagg_lookup (the per-mapping program and the run-time-mapping form),
strom_submit_gpupreagg_lookup_star and strom_submit_gpupreagg_joined, whose kernels turn a text
column's 8-byte offsets into datum addresses (strom_gpupreagg.h: strom_kvars_from_outer_column).

The parent of this change answers BadRequest to every accepted request below: a session whose
program has a text variable was refused by all three calls.

Dimensions and helpers are test_star_lookup_gpu.py's; the values are text_cases.WORDS; the model
is Python's own bytes comparison per distinct word (character(n) through text_cases.bpchar_key),
indexed by the row's word.  Bars: keys, counts and integer sums equal; float8 sums within rtol
1e-12 (check_count_and_sums) -- a group here sums at most ~1e5 values of [0, 1) in an order the
LDS atomics pick, a random-walk error of sqrt(1e5) * 2^-53 = 3.5e-14 relative, worst case
1e5 * 2^-53 = 1.1e-11 only if every rounding went one way.
"""
import numpy as np
import pytest

import text_cases
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash, STROM_RESULTS_ON_DEVICE
from pg_strom_amd.gpupreagg import GpuPreAgg
from test_star_lookup_gpu import (BAD_REQUEST, CPU_RECHECK, TILE_ROWS, Dim, check_count_and_sums, model_groups,
                                  open_joins, partial_rows)

pytestmark = pytest.mark.gpu

CORRUPTION = 300                                # StromError_DataStoreCorruption
WORDS = text_cases.WORDS
CHR10 = [(w[:10] + b" " * 10)[:10] for w in WORDS]     # character(10) as PostgreSQL stores it
NGROUPS = 53

# The program's variables, for the one-table calls and for the star alike:
#   1 the group column (dimension 1)   2 a int4   3 b float8   4 t text   5 c character(10)
#   6 an int4 column of a dimension (dimension 1's second column / dimension 2's column)
AGGS = "(key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"
# fact(k1, a, b, t, c) against one dimension; fact(k1, k2, a, b, t, c) against two
ONE_COLUMNS = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8"), (0, 4, "text"), (0, 5, "character"), (1, 3, "int4")]
STAR_COLUMNS = [(1, 2, "int4"), (0, 3, "int4"), (0, 4, "float8"), (0, 5, "text"), (0, 6, "character"), (2, 2, "int4")]


def words_where(fn, words=WORDS):
    return np.array([bool(fn(w)) for w in words])


# name -> (qual, external parameters, rows that pass: f(fact, var 6 values, var 6 isnull))
QUALS = {
    # outer columns only: evaluated BEFORE the probe (qual-first)
    "texteq": ("(texteq (var 4 text) (const text 'MAIL'))", (),
               lambda f, w, wn: ~f.tnull & words_where(lambda x: x == b"MAIL")[f.ti]),
    "text_lt_param": ("(text_lt (var 4 text) (param 0 text))", (b"b",),
                      lambda f, w, wn: ~f.tnull & words_where(lambda x: x < b"b")[f.ti]),
    # the blank rule: 'hello' against 'hello     ' ('hello', 'hello ' and 'hello  ' all store that)
    "bpchareq": ("(bpchareq (var 5 character) (const character 'hello'))", (),
                 lambda f, w, wn: words_where(lambda x: text_cases.bpchar_key(x) == b"hello", CHR10)[f.ci]),
    "isnull": ("(isnull (var 4 text))", (), lambda f, w, wn: f.tnull.copy()),
    # also reads a dimension column: evaluated AFTER the probes
    "text_and_inner": ("(and (text_ge (var 4 text) (const text 'a')) (int4gt (var 6 int4) (const int4 2)))", (),
                       lambda f, w, wn: ~f.tnull & words_where(lambda x: x >= b"a")[f.ti] & ~wn & (w > 2)),
}


def spec_of(qualname):
    return "(gpupreagg (qual " + QUALS[qualname][0] + ") " + AGGS + ")"


_DIMS = {}


def dims(ngroups=NGROUPS):
    """computed once, shared, left unchanged: dimension 1 serves the group column and an int4
    column, dimension 2 an int4 column; both have holes and NULLs"""
    if ngroups not in _DIMS:
        rng = np.random.default_rng(2203 + ngroups)
        nd = 3000 if ngroups == NGROUPS else 40000
        d1 = Dim(rng, nd, key_lo=-700)
        d1.add("int4", (d1.key % ngroups).astype(np.int32), rng.random(nd) < 0.04)
        d1.add("int4", rng.integers(-5, 6, nd).astype(np.int32), rng.random(nd) < 0.03)
        d2 = Dim(rng, 3000, key_lo=100)
        d2.add("int4", rng.integers(0, 10, 3000).astype(np.int32), rng.random(3000) < 0.03)
        _DIMS[ngroups] = (d1, d2)
    return _DIMS[ngroups]


def shared_column(sqltype, datums, pick, isnull=None):
    """a varlena column whose row i holds datums[pick[i]]: one datum buffer per distinct value (a
    Column of its own per row costs a ctypes buffer per row)"""
    col = kds.Column(sqltype, datums)
    col.values = np.ascontiguousarray(col.values[pick])
    if isnull is not None:
        col.isnull = np.ascontiguousarray(isnull, dtype=np.uint8)
    return col


class Fact(object):
    """fact(k1 [, k2], a int4, b float8, t text, c character(10)); t has NULLs with text_nulls"""

    def __init__(self, n, seed, fdims, key_nulls=True, text_nulls=True):
        rng = np.random.default_rng(seed)
        self.n, self.dims, self.key_nulls = n, fdims, key_nulls
        self.keys = [d.fact_keys(rng, n, key_nulls) for d in fdims]
        self.a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
        self.b = rng.random(n)
        self.ti = rng.integers(0, len(WORDS), n)
        self.ci = rng.integers(0, len(WORDS), n)
        self.tnull = (rng.random(n) < 0.07) if text_nulls else np.zeros(n, dtype=bool)
        if text_nulls and n > 1:
            self.tnull[1] = True                # (a chunk without a NULL has no bitmap)
        self.text_datums = WORDS                # (the unreadable-datum tests add raw datums)
        self.text_type = "text"

    def chunk(self):
        cols = [kds.Column(d.keytype, k, kn if self.key_nulls else None) for d, (k, kn) in zip(self.dims, self.keys)]
        cols += [kds.Column("int4", self.a), kds.Column("float8", self.b),
                 shared_column(self.text_type, self.text_datums, self.ti, self.tnull if self.tnull.any() else None),
                 shared_column("character", CHR10, self.ci)]
        return kds.build_kds("column", cols)

    def partners(self):
        return [d.partner(k, kn) for d, (k, kn) in zip(self.dims, self.keys)]

    def var6(self):
        """the dimension column the program reads as (var 6 int4), per fact row"""
        p = self.partners()
        if len(self.dims) == 1:
            _, v, isn = self.dims[0].cols[1]
            i = np.clip(p[0], 0, self.dims[0].nd - 1)
        else:
            _, v, isn = self.dims[1].cols[0]
            i = np.clip(p[1], 0, self.dims[1].nd - 1)
        return v[i], isn[i]


def selected(fact, passes):
    alive = np.logical_and.reduce([p >= 0 for p in fact.partners()])
    return np.flatnonzero(alive & passes)


def check_rows(fact, pr, passes, a_in=None, times=1):
    sel = selected(fact, passes)
    i1 = fact.partners()[0][sel]
    g = fact.dims[0].cols[0]
    uk, inv = model_groups([(g[1][i1], g[2][i1])])
    keys, cols = partial_rows(pr, 1)
    assert np.array_equal(keys, uk)
    check_count_and_sums(cols, inv, len(uk), (fact.a if a_in is None else a_in)[sel], fact.b[sel], times=times)
    return sel


def fold(fact, spec, ext=(), star=False, ngroups=NGROUPS, chunk=None):
    """one lookup request over the fact chunk: (status, partial rows or None, perfmon)"""
    runtime.init()
    ds = runtime.DeviceStore.upload(fact.chunk() if chunk is None else chunk)
    joins = open_joins(fact.dims, list(range(1, len(fact.dims) + 1)))
    agg = GpuPreAgg(spec)
    try:
        agg.begin([(0, ngroups)], ext_params=list(ext))
        pending = (agg.submit_lookup_star(joins, ds, STAR_COLUMNS) if star
                   else agg.submit_lookup(joins[0], ds, ONE_COLUMNS))
        st, pfm = agg.collect(pending)
        pr = agg.fetch() if st == 0 else None
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    return st, pr, pfm


def run_qual(fact, qualname, star=False):
    qual, ext, passes_fn = QUALS[qualname]
    st, pr, _ = fold(fact, spec_of(qualname), ext, star=star)
    assert st == 0
    passes = passes_fn(fact, *fact.var6())
    sel = check_rows(fact, pr, passes)
    return sel, passes


# ---------------------------------------------------------------------------------------------
# the one-table lookup, both mapping forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("qualname", ["texteq", "text_lt_param", "bpchareq", "isnull"])
def test_one_table_lookup_with_a_text_qual(qualname, generic, monkeypatch):
    """the program built FOR the mapping, and the run-time-mapping kernel of the session's own
    program (STROM_GPUPREAGG_LOOKUP_GENERIC): texteq, text_lt against a parameter, bpchareq under
    the blank rule, isnull(text); keys with NULLs, holes and values outside the table"""
    if generic:
        monkeypatch.setenv("STROM_GPUPREAGG_LOOKUP_GENERIC", "1")
    fact = Fact(9001, 31, dims()[:1])
    sel, passes = run_qual(fact, qualname)
    assert 0 < len(sel) < np.count_nonzero(fact.partners()[0] >= 0)
    assert np.count_nonzero(passes & (fact.partners()[0] < 0)) > 0      # the qual keeps rows the join drops


@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("nrows", [1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 3 * TILE_ROWS + 5])
def test_row_counts_around_one_tile(nrows, nulls):
    """one row, a tile less one (all ragged), one tile (the straight-line loaders; bitmap-free when
    no column has a NULL), a tile and one, three tiles and five"""
    fact = Fact(nrows, 100 + nrows, dims()[:1], key_nulls=nulls, text_nulls=nulls)
    run_qual(fact, "texteq" if nulls else "bpchareq")


def test_a_work_group_walks_several_tiles_and_ends_on_a_ragged_one(monkeypatch):
    """one work-group per CU and 2 x CUs x T + 5 rows (the environment of test_star_lookup_gpu's
    test of that name): every work-group folds at least two tiles -- the next tile's offsets are
    prefetched while this tile's datums are compared -- and the last tile has five rows"""
    monkeypatch.setenv("STROM_GPUPREAGG_BLOCKS_PER_CU", "1")
    runtime.init()
    W = runtime.device_info()["compute_units"]
    fact = Fact(2 * W * TILE_ROWS + 5, 41, dims()[:1])
    sel, _ = run_qual(fact, "texteq")
    assert len(sel) > 0


def test_a_text_qual_that_also_reads_a_dimension_column_runs_after_the_probe():
    fact = Fact(9001, 43, dims()[:1])
    sel, passes = run_qual(fact, "text_and_inner")
    assert 0 < len(sel) < np.count_nonzero(fact.partners()[0] >= 0)


def test_text_inside_an_aggregate_argument():
    """psum(case when t = 'MAIL' then a else 0 end): no qual, the text column is read by the
    aggregate's argument alone; a NULL t takes the else branch"""
    fact = Fact(9001, 47, dims()[:1])
    spec = ("(gpupreagg (key (var 1 int4)) (nrows)"
            " (psum (case (when (texteq (var 4 text) (const text 'MAIL')) (int8 (var 2 int4))) (else (const int8 0))))"
            " (psum (var 3 float8)))")
    st, pr, _ = fold(fact, spec)
    assert st == 0
    mail = ~fact.tnull & words_where(lambda x: x == b"MAIL")[fact.ti]
    assert mail.any()
    check_rows(fact, pr, np.ones(fact.n, dtype=bool), a_in=np.where(mail, fact.a, 0))


# ---------------------------------------------------------------------------------------------
# the star
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qualname,narrow", [("bpchareq", True), ("texteq", False), ("text_and_inner", True)])
def test_two_dimensions_with_a_text_qual_on_the_fact(qualname, narrow, monkeypatch):
    """narrow (2- / 4-byte) and standard (8- / 16-byte, STROM_HASHJOIN_NO_NARROW_RECS) slot
    records; a qual-first over fact columns, and one that reads relation 2's column"""
    if not narrow:
        monkeypatch.setenv("STROM_HASHJOIN_NO_NARROW_RECS", "1")
    fact = Fact(9001, 53, dims())
    sel, passes = run_qual(fact, qualname, star=True)
    p1, p2 = fact.partners()
    assert 0 < len(sel) < np.count_nonzero((p1 >= 0) & (p2 >= 0))
    assert np.count_nonzero(passes & (p1 >= 0) & (p2 < 0)) > 0 and np.count_nonzero(passes & (p1 < 0) & (p2 >= 0)) > 0


@pytest.mark.parametrize("text_nulls", [True, False])
def test_star_with_packed_accumulators(text_nulls):
    """1e4 groups, nrows and sums of OUTER columns without NULLs: gpupreagg_packed_lookup_star
    (num_kern_prep reports it); the text column is a qual input only -- never a packed field, no
    zone map -- and its NULL bitmap only picks the loader"""
    ngroups = 10000
    d1, d2 = dims(ngroups)
    fact = Fact(40009, 59, (d1, d2), key_nulls=False, text_nulls=text_nulls)
    qual, ext, passes_fn = QUALS["text_lt_param"]
    st, pr, pfm = fold(fact, spec_of("text_lt_param"), ext, star=True, ngroups=ngroups)
    assert st == 0
    assert pfm["num_kern_prep"] == 1                                    # the packed path was taken
    sel = check_rows(fact, pr, passes_fn(fact, *fact.var6()))
    assert len(sel) > 1000


# ---------------------------------------------------------------------------------------------
# the joined fold, and the plan that existed before
# ---------------------------------------------------------------------------------------------
def test_joined_fold_with_the_text_qual_in_the_aggregate_program():
    """strom_submit_gpupreagg_joined over a finished join with STROM_RESULTS_ON_DEVICE"""
    runtime.init()
    d1 = dims()[0]
    fact = Fact(9001, 61, (d1,))
    ds = runtime.DeviceStore.upload(fact.chunk())
    join = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(build_multihash([(d1.chunk(), [1])]))
    agg = GpuPreAgg(spec_of("texteq"))
    try:
        agg.begin([(0, NGROUPS)])
        jp = join.submit(ds, flags=STROM_RESULTS_ON_DEVICE)
        ap = agg.submit_joined(join, jp, ds, ONE_COLUMNS)
        assert agg.collect(ap)[0] == 0
        jr = join.collect(jp)
        pr = agg.fetch()
    finally:
        agg.end()
        join.end()
        ds.release()
    assert jr.nitems == np.count_nonzero(fact.partners()[0] >= 0)
    sel = check_rows(fact, pr, QUALS["texteq"][2](fact, *fact.var6()))
    assert len(sel) > 0


def test_same_answer_as_the_general_join_the_column_projection_and_a_plain_fold():
    """today's only plan for this query: the join, strom_hashjoin_project_column carrying the text
    and character(n) columns, then the plain fold of the joined chunk"""
    runtime.init()
    d1 = dims()[0]
    fact = Fact(20011, 67, (d1,))
    spec = spec_of("bpchareq")
    ds = runtime.DeviceStore.upload(fact.chunk())
    joins = open_joins([d1], [1])
    got = []
    try:
        for lookup in (True, False):
            agg = GpuPreAgg(spec)
            joined = None
            try:
                agg.begin([(0, NGROUPS)])
                if lookup:
                    assert agg.collect(agg.submit_lookup(joins[0], ds, ONE_COLUMNS))[0] == 0
                else:
                    joined, nitems = joins[0].join_to_column(ds, ONE_COLUMNS)
                    assert agg.fold(joined)[0] == 0
                got.append(partial_rows(agg.fetch(), 1))
            finally:
                agg.end()
                if joined is not None:
                    joined.release()
    finally:
        joins[0].end()
        ds.release()
    assert nitems == np.count_nonzero(fact.partners()[0] >= 0)
    (kl, cl), (kp, cp) = got
    assert len(kl) > 1 and np.array_equal(kl, kp)
    assert np.array_equal(cl[0][0], cp[0][0])                          # nrows
    assert np.array_equal(cl[1][0], cp[1][0])                          # integer sum
    assert np.allclose(cl[2][0], cp[2][0], rtol=1e-12, atol=0)         # float8 sum


# ---------------------------------------------------------------------------------------------
# datums the device cannot read, offsets that leave the chunk
# ---------------------------------------------------------------------------------------------
def unreadable_fact(n, seed, fdims, bad, partner):
    """text_raw datums as tests/test_text_gpu.py builds them: row 'bad' holds a compressed datum,
    row bad + 1 an external one; with partner=False both rows' dimension-1 keys fall into a hole"""
    fact = Fact(n, seed, fdims, key_nulls=False, text_nulls=False)
    d1 = fdims[0]
    k1 = d1.key[np.random.default_rng(seed).integers(0, d1.nd, n)].astype(np.int32)     # every row has a partner
    compressed = np.array([(20 << 2) | 2], dtype="<u4").tobytes() + b"\0" * 16
    external = bytes([0x01, 18]) + b"\0" * 16
    fact.text_type = "text_raw"
    fact.text_datums = [kds.varlena_datum(w) for w in WORDS] + [compressed, external]
    fact.ti[bad], fact.ti[bad + 1] = len(WORDS), len(WORDS) + 1
    if not partner:
        hole = np.setdiff1d(np.arange(d1.key_lo, d1.key_lo + d1.span), d1.key)[0]
        k1[bad] = k1[bad + 1] = hole
    fact.keys[0] = (k1, np.zeros(n, dtype=bool))
    return fact


@pytest.mark.parametrize("partner", [True, False])
@pytest.mark.parametrize("qualname", ["texteq", "text_and_inner"])
def test_an_unreadable_datum_needs_a_partner_to_send_the_chunk_back(qualname, partner):
    """a compressed and an external datum, met by the qual-first ("texteq") or by the row function
    behind the probe ("text_and_inner").  In rows with a partner: CpuReCheck, nothing folded, and the
    session folds the next clean chunk correctly.  In rows without one: status 0 and the right
    groups -- an error needs a partner, as in
    test_star_lookup_gpu.test_an_error_in_an_outer_only_qual_needs_a_partner_in_every_relation"""
    runtime.init()
    d1 = dims()[0]
    bad = 4321
    dirty = unreadable_fact(9001, 71, (d1,), bad, partner)
    clean = Fact(9001, 73, (d1,))
    qual, ext, passes_fn = QUALS[qualname]
    ds_dirty = runtime.DeviceStore.upload(dirty.chunk())
    ds_clean = runtime.DeviceStore.upload(clean.chunk())
    joins = open_joins([d1], [1])
    agg = GpuPreAgg(spec_of(qualname))
    try:
        agg.begin([(0, NGROUPS)])
        st = agg.collect(agg.submit_lookup(joins[0], ds_dirty, ONE_COLUMNS))[0]
        if partner:
            assert st == CPU_RECHECK
            assert agg.collect(agg.submit_lookup(joins[0], ds_clean, ONE_COLUMNS))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        joins[0].end()
        ds_dirty.release()
        ds_clean.release()
    if partner:
        check_rows(clean, pr, passes_fn(clean, *clean.var6()))          # the clean chunk's rows, and only they
        return
    assert st == 0
    p1 = dirty.partners()[0]
    assert p1[bad] < 0 and p1[bad + 1] < 0 and np.count_nonzero(p1 < 0) == 2
    dirty.ti[bad] = dirty.ti[bad + 1] = 0       # (the model never looks at rows without a partner)
    sel = check_rows(dirty, pr, passes_fn(dirty, *dirty.var6()))
    assert len(sel) > 0


def values_offset(buf, col):
    """where column 'col' of a COLUMN chunk image keeps its array (kern_coldir.values_off)"""
    head = kds.KdsHead(buf)
    coldir_off = kds.stromalign(kds.KDS_HEAD_FIXED + 8 * head.ncols)
    return int(np.frombuffer(buf[coldir_off + 32 * col:coldir_off + 32 * col + 4].tobytes(), dtype="<u4")[0])


@pytest.mark.parametrize("call", ["lookup", "star"])
def test_an_offset_beyond_the_chunk_is_corruption_and_never_followed(call):
    """the text column's offset of a row with a partner points 1 GB behind the chunk's end:
    DataStoreCorruption, no fault -- the offset is checked against kds->length before anything
    behind it is read"""
    star = (call == "star")
    fdims = dims() if star else dims()[:1]
    fact = Fact(9001, 79, fdims, key_nulls=False, text_nulls=False)
    for r, d in enumerate(fdims):               # every row has a partner in every relation
        fact.keys[r] = (d.key[np.random.default_rng(83 + r).integers(0, d.nd, fact.n)].astype(np.int32),
                        np.zeros(fact.n, dtype=bool))
    buf = fact.chunk()
    tcol = len(fdims) + 2                       # 0-based chunk column of t
    at = values_offset(buf, tcol) + 8 * 4321
    length = kds.KdsHead(buf).length
    assert 0 < int(buf[at:at + 8].view(np.uint64)[0]) < length
    buf[at:at + 8] = np.array([length + (1 << 30)], dtype="<u8").view(np.uint8)
    with pytest.raises(runtime.StromError) as ei:
        fold(fact, spec_of("texteq"), star=star, chunk=buf)
    assert ei.value.errcode == CORRUPTION


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_text_variables_a_mapping_cannot_serve_are_refused_and_nothing_is_launched():
    """(var 4 text) / (var 5 character) must be varlena columns of the fact chunk, mapped at depth 0
    under their own type: BadRequest otherwise, by all three calls, with nothing folded -- the
    accepted request at the end finds an empty table"""
    runtime.init()
    d1, d2 = dims()
    fact = Fact(9001, 89, (d1, d2))
    ds = runtime.DeviceStore.upload(fact.chunk())
    joins = open_joins([d1, d2], [1, 2])
    general = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(build_multihash([(d1.chunk(), [1])]))
    qual = "(and " + QUALS["texteq"][0] + " " + QUALS["bpchareq"][0] + ")"
    agg = GpuPreAgg("(gpupreagg (qual " + qual + ") " + AGGS + ")")

    def with_column(columns, i, entry):
        return columns[:i] + [entry] + columns[i + 1:]

    def refused(submit):
        with pytest.raises(runtime.StromError) as ei:
            submit()
        assert ei.value.errcode == BAD_REQUEST, ei.value

    # star: t is chunk column 5, c column 6, a (int4, by value) column 3; one table: t 5, c 6, a 3 too
    # (the one-table call probes with the chunk's column 1 and ignores k2)
    bad_mappings = [with_column(STAR_COLUMNS, 3, (1, 2, "text")),       # a text variable served by a dimension
                    with_column(STAR_COLUMNS, 4, (2, 2, "character")),
                    with_column(STAR_COLUMNS, 3, (0, 3, "text")),       # ... mapped onto a by-value column
                    with_column(STAR_COLUMNS, 3, (0, 5, "int8")),       # ... whose entry names another type
                    with_column(STAR_COLUMNS, 3, (0, 5, "character")),
                    with_column(STAR_COLUMNS, 4, (0, 6, "text")),
                    STAR_COLUMNS[:4]]                                   # ... or no entry at all
    try:
        agg.begin([(0, NGROUPS)])
        for columns in bad_mappings:
            refused(lambda: agg.submit_lookup_star(joins, ds, columns))
            one = [(d, a, t) if d < 2 else (1, 3, t) for d, a, t in columns]    # (relation 2's column: dimension 1's)
            refused(lambda: agg.submit_lookup(joins[0], ds, one))
        jp = general.submit(ds, flags=STROM_RESULTS_ON_DEVICE)
        one = [(d, a, t) if d < 2 else (1, 3, t) for d, a, t in bad_mappings[0]]
        refused(lambda: agg.submit_joined(general, jp, ds, one))
        general.collect(jp)
        # nothing was folded, and the session works
        assert agg.collect(agg.submit_lookup_star(joins, ds, STAR_COLUMNS))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        general.end()
        for j in joins:
            j.end()
        ds.release()
    passes = QUALS["texteq"][2](fact, None, None) & QUALS["bpchareq"][2](fact, None, None)
    check_rows(fact, pr, passes)
