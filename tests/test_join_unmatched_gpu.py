"""
RIGHT and FULL joins on the device (needs an MI355X: -m gpu): an INNER / LEFT program with
(track_matches) on its last relation, whose probe kernels flag the entries they accept, and the
unmatched pass after the last chunk.  The chunks' records are checked against the nested-loop model
of tests/join_model.py (and against the same program without tracking), the unmatched pass against
tests/outer_join_model.py: all row ids of the tracked relation minus those the model puts into its
slot over the chunks fed, compared as sets.

Shapes are the kernels' edges: one work-group over 1, T-1, T+1 and 3T+1 rows per one-pass family
(STROM_HASHJOIN_MAX_GRID=1), every case again through the general kernel (STROM_HASHJOIN_NO_FAST=1);
flags of 64 neighbouring entries set from many work-groups at once; the unmatched pass's stage at
exactly full and one beyond with one work-group (STROM_HASHJOIN_UNMATCHED_MAX_GRID=1).
"""
import ctypes

import numpy as np
import pytest

import join_model as jm
import outer_join_model as ojm
import text_cases
import zone_map_model as zm
from pg_strom_amd import kds, runtime
from pg_strom_amd._lib import lib
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash, entry_rowids, STROM_RESULTS_ON_DEVICE
from pg_strom_amd.gpupreagg import GpuPreAgg
from test_hashjoin_edges_gpu import FAMILIES, family_keys, outer_keys
from test_text_gpu import _walk_row_flat

pytestmark = pytest.mark.gpu

ERR_BAD_REQUEST = 101
ERR_NOSPACE = 301
HEAP_HASNULL = 0x0001
UNMATCHED_STAGE = 8192                          # offsets the unmatched pass stages before it must flush
KEY = "(hashkey (var 1 int4) 1 int4)"


def one_rel(jointype, tracked=True, sqltype="int4", qual=""):
    return "(gpuhashjoin (rel (hashkey (var 1 %s) 1 %s)%s (jointype %s)%s))" % (
        sqltype, sqltype, qual, jointype, " (track_matches)" if tracked else "")


def track_last(spec):
    assert spec.endswith("))")
    return spec[:-2] + " (track_matches)))"


class Session(object):
    """one tracked table, kept for every case that probes it"""

    def __init__(self, spec, inners, keys, ext=()):
        self.join = GpuHashJoin(spec)
        try:
            self.join.begin(build_multihash(list(zip(inners, keys))), ext_params=ext)
            self.dkm = self.join.device_kmhash()
            self.info = [self.join.table_info(d + 1) for d in range(len(inners))]
            self.nlast = self.info[-1]["nentries"]
        except Exception:
            self.join.end()
            raise

    def feed(self, outer, want, row_map=None, nrooms=None):
        """one chunk: its records == the model's"""
        res = self.join.collect(self.join.submit(outer, nrooms=len(want) + 8 if nrooms is None else nrooms,
                                                 row_map=row_map))
        assert res.errcode == 0 and res.nitems == len(want), (res.errcode, res.nitems, len(want))
        got = jm.records_to_rowids(self.dkm, res.records)
        assert np.array_equal(jm.sorted_records(got), jm.sorted_records(want))
        return res

    def unmatched_ids(self, **kw):
        res = self.join.unmatched(**kw)
        assert res.errcode == 0 and res.nitems == len(res.records)
        assert res.records.shape[1] == len(self.info) + 1
        return ojm.device_unmatched_rowids(self.dkm, res.records)

    def check_unmatched(self, want_records_fed):
        """the unmatched pass after chunks whose model records are given"""
        matched = np.unique(np.concatenate([np.zeros(0, dtype=np.int64)] +
                                           [ojm.unmatched_from_records(r) for r in want_records_fed]))
        want = np.setdiff1d(np.arange(self.nlast, dtype=np.int64), matched)
        got = self.unmatched_ids()
        assert np.array_equal(got, want), (len(got), len(want))
        return want

    def end(self):
        self.join.end()


class Sessions(object):
    def __init__(self):
        self.made = {}

    def get(self, name, make):
        if name not in self.made:
            self.made[name] = make()
        return self.made[name]

    def end(self):
        for s in self.made.values():
            s.end()
        self.made = {}


@pytest.fixture(scope="module")
def sessions():
    s = Sessions()
    yield s
    s.end()


# ---------------------------------------------------------------------------------------------
# 1. each one-pass family x {inner, left}
# ---------------------------------------------------------------------------------------------
MIXES = {"none": (0.0, False), "all": (1.0, False), "most": (0.8, True)}
ROWS = ["one_row", "tile_less_one", "tile_and_one", "three_tiles_and_one"]
_CASES = {}


def rows_of(family, where):
    T = FAMILIES[family][3]
    return {"one_row": 1, "tile_less_one": T - 1, "tile_and_one": T + 1, "three_tiles_and_one": 3 * T + 1}[where]


def family_session(sessions, family, jointype, tracked=True):
    def make():
        pk, pkn = family_keys(family)
        inner = kds.build_kds("row_flat", [kds.Column("int4", pk, pkn),
                                           kds.Column("int4", np.arange(len(pk), dtype=np.int32))])
        s = Session(one_rel(jointype, tracked), [inner], [[1]])
        s.pk, s.pkn = pk, pkn
        assert s.info[0]["mode"] == FAMILIES[family][4] and s.info[0]["unique"] and pkn.any()
        assert s.join.tracked_depth() == (1 if tracked else 0)
        return s
    return sessions.get((family, jointype, tracked), make)


def family_case(s, family, nrows, mix):
    key = (family, nrows, mix)
    if key not in _CASES:
        rate, nulls = MIXES[mix]
        fk, fkn = outer_keys(s, family, nrows, rate, nulls)
        _CASES[key] = dict(fk=fk, fkn=fkn, memo={}, outer=kds.build_kds("column", [kds.Column("int4", fk, fkn)]))
    return _CASES[key]


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("where", ROWS)
@pytest.mark.parametrize("jointype", ["inner", "left"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_one_pass_families_flag_what_they_join(sessions, family, jointype, where, mix, monkeypatch):
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = family_session(sessions, family, jointype)
    plain = family_session(sessions, family, jointype, tracked=False)
    nrows = rows_of(family, where)
    case = family_case(s, family, nrows, mix)
    rel = [jm.Rel(len(s.pk), [jm.Key(jm.outer_column(case["fk"], case["fkn"]), s.pk, s.pkn)], jointype)]
    want = jm.join_model(np.arange(nrows), rel, memo=case["memo"])
    nmatched = len(np.unique(want[want[:, 1] >= 0][:, 1]))
    if mix == "none":
        assert nmatched == 0
    if mix != "none" and nrows > 100:
        assert 0 < nmatched < len(s.pk)
    if mix == "most" and nrows > 100:
        assert case["fkn"].any() and (len(want) < nrows or jointype == "left")
    for no_fast in (False, True):
        if no_fast:
            monkeypatch.setenv("STROM_HASHJOIN_NO_FAST", "1")
        s.join.reset_matches()
        res = s.feed(case["outer"], want)
        assert res.perfmon["num_kern_prep"] == (1 if FAMILIES[family][5] and not no_fast else 0)
        # ... the records of the same program without tracking, entry offsets and all
        ref = plain.join.collect(plain.join.submit(case["outer"], nrooms=len(want) + 8))
        assert ref.errcode == 0
        assert np.array_equal(jm.sorted_records(res.records), jm.sorted_records(ref.records))
        got = s.unmatched_ids()
        assert len(got) == len(s.pk) - nmatched
        assert np.array_equal(got, np.setdiff1d(np.arange(len(s.pk)), ojm.unmatched_from_records(want)))
        # an entry with a NULL key can never be matched
        assert np.isin(np.flatnonzero(s.pkn), got).all()


# ---------------------------------------------------------------------------------------------
# 2. the general kernel
# ---------------------------------------------------------------------------------------------
def qual_case():
    """duplicate inner keys, NULL keys on both sides, and an ON qual (inner column 2 < outer column 2)
    that rejects some of the entries whose key is equal"""
    rng = np.random.default_rng(61)
    ninner, nouter = 400, 3001
    pk = rng.integers(0, 150, ninner).astype(np.int32)
    pkn = rng.random(ninner) < 0.05
    iv = rng.integers(0, 100, ninner).astype(np.int32)
    fk = rng.integers(-5, 160, nouter).astype(np.int32)
    fkn = rng.random(nouter) < 0.05
    ov = rng.integers(0, 100, nouter).astype(np.int32)
    return dict(pk=pk, pkn=pkn, iv=iv, fk=fk, fkn=fkn, ov=ov,
                inner=kds.build_kds("row_flat", [kds.Column("int4", pk, pkn), kds.Column("int4", iv)]),
                outer=kds.build_kds("column", [kds.Column("int4", fk, fkn), kds.Column("int4", ov)]))


@pytest.mark.parametrize("jointype", ["inner", "left"])
def test_duplicate_keys_and_a_qual_that_rejects_equal_keys(sessions, jointype):
    c = qual_case()
    s = sessions.get(("qual", jointype), lambda: Session(
        one_rel(jointype, qual=" (qual (int4lt (ivar 1 2 int4) (var 2 int4)))"), [c["inner"]], [[1]]))
    assert not s.info[0]["unique"]
    rels = [jm.Rel(len(c["pk"]), [jm.Key(jm.outer_column(c["fk"], c["fkn"]), c["pk"], c["pkn"])], jointype,
                   lambda orow, irows, e: c["iv"][e] < c["ov"][orow])]
    stats = []
    want = jm.join_model(np.arange(len(c["fk"])), rels, stats=stats)
    assert jm.prefix_kinds(stats[0])
    s.join.reset_matches()
    s.feed(c["outer"], want)
    unmatched = s.check_unmatched([want])
    matched = np.setdiff1d(np.arange(len(c["pk"])), unmatched)
    # every entry of a matched key that passes the qual for some row is flagged: duplicates among them
    keys, counts = np.unique(c["pk"][matched], return_counts=True)
    assert (counts > 1).any()
    # an entry whose key some outer row has, but which the qual rejects for every such row, stays unmatched
    has_equal_key = np.isin(c["pk"], c["fk"][~c["fkn"]]) & ~c["pkn"]
    assert has_equal_key[unmatched].any()
    assert np.isin(np.flatnonzero(c["pkn"]), unmatched).all() and c["pkn"].any()


@pytest.mark.parametrize("jointype", ["inner", "left"])
def test_every_inner_key_null_and_an_empty_outer_stream(sessions, jointype):
    n = 77
    inner = kds.build_kds("row_flat", [kds.Column("int4", np.zeros(n, dtype=np.int32), np.ones(n, dtype=bool)),
                                       kds.Column("int4", np.arange(n, dtype=np.int32))])
    s = Session(one_rel(jointype), [inner], [[1]])
    try:
        assert s.nlast == n
        # no chunk at all: everything is unmatched
        assert np.array_equal(s.unmatched_ids(), np.arange(n))
        fk = np.arange(50, dtype=np.int32) % 3
        want = jm.join_model(np.arange(50), [jm.Rel(n, [jm.Key(jm.outer_column(fk), np.zeros(n), np.ones(n, dtype=bool))], jointype)])
        assert len(want) == (0 if jointype == "inner" else 50)
        s.feed(kds.build_kds("column", [kds.Column("int4", fk)]), want)
        assert np.array_equal(s.unmatched_ids(), np.arange(n))
    finally:
        s.end()


def test_text_key_through_the_hash_index(sessions):
    iv = [b"a", b"L" * 200, b"b", b"b", None, b"zz", b"never"]
    ov = [[b"a ", b"a", None, b"L" * 200, b"absent", b"b", b""][(i * 3 + i // 7) % 7] for i in range(301)]
    inull = np.array([v is None for v in iv])
    onull = np.array([v is None for v in ov])
    inner = kds.build_kds("row_flat", [kds.Column("text", iv, inull), kds.Column("int4", np.arange(len(iv), dtype=np.int32))])
    s = Session(one_rel("left", sqltype="text"), [inner], [[1]])
    try:
        assert s.info[0]["mode"] == "hash"
        as_obj = lambda vals: np.array([b"" if v is None else bytes(v) for v in vals] + [None], dtype=object)[:-1]
        rels = [jm.Rel(len(iv), [jm.Key(jm.outer_column(as_obj(ov), onull), as_obj(iv), inull)], "left")]
        for fmt in ("row_flat", "column"):
            s.join.reset_matches()
            outer = kds.build_kds(fmt, [kds.Column("text", ov, onull), kds.Column("int4", np.arange(len(ov), dtype=np.int32))])
            want = jm.join_model(np.arange(len(ov)), rels)
            s.feed(outer, want)
            assert s.check_unmatched([want]).tolist() == [4, 5, 6]      # NULL, 'zz', 'never'
    finally:
        s.end()


_GENERAL = {}


def general_world():
    if not _GENERAL:
        d = jm.general_data()
        _GENERAL["d"] = d
        for fmt in ("row", "row_flat", "column"):
            _GENERAL[fmt], _GENERAL["inners"] = jm.general_chunks(d, fmt)
        n = len(d["fa"])
        _GENERAL["row_map"] = np.arange(n, dtype=np.int32)[::-1][::3].copy()
    return _GENERAL


def general_check(s, rels, fmt, mapped):
    w = general_world()
    rows = w["row_map"] if mapped else np.arange(len(w["d"]["fa"]))
    want = jm.join_model(rows, rels)
    assert len(want) > 0
    s.join.reset_matches()
    s.feed(w[fmt], want, row_map=w["row_map"] if mapped else None)
    unmatched = s.check_unmatched([want])
    assert 0 < len(unmatched) < s.nlast
    return want, unmatched


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("fmt", ["row", "row_flat", "column"])
@pytest.mark.parametrize("jointype", ["inner", "left"])
def test_two_key_relation_every_format_and_a_row_map(sessions, jointype, fmt, mapped):
    w = general_world()
    spec = ("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (hashkey (int8 (var 2 int2)) 2 int8)"
            " (qual (float8gt (ivar 1 3 float8) (var 3 float8))) (jointype %s) (track_matches)))" % jointype)
    s = sessions.get(("two_key", jointype), lambda: Session(spec, w["inners"][:1], [[1, 2]]))
    assert s.info[0]["mode"] == "hash"
    general_check(s, [jm._rel1(w["d"], jointype)], fmt, mapped)


PAIRS = [(t1, t2) for t1 in ("inner", "left", "semi", "anti") for t2 in ("inner", "left")]


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("fmt", ["row", "column"])
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_two_relations_the_last_one_tracked(sessions, pair, fmt, mapped):
    w = general_world()
    s = sessions.get(("two", pair), lambda: Session(track_last(jm.two_rel_spec(*pair)), w["inners"][:2], [[1, 2], [1]],
                                                    ext=[np.int16(jm.PARAM_V2)]))
    assert s.join.tracked_depth() == 2
    d = w["d"]
    want, unmatched = general_check(s, jm.two_rel_model(d, *pair), fmt, mapped)
    # an entry is flagged only when the prefix reaches it.  Behind a semi / anti relation the tracked
    # one is keyed by an outer column, so it can be joined alone: relation 1 in front of it lets
    # fewer rows through: it never matches an entry those rows alone would not have matched
    if pair[0] in ("semi", "anti"):
        rows = w["row_map"] if mapped else np.arange(len(d["fa"]))
        alone = jm.join_model(rows, jm.two_rel_model(d, *pair)[1:])
        alone = np.setdiff1d(np.unique(alone[:, -1]), [-1])
        assert np.isin(np.setdiff1d(np.arange(s.nlast), unmatched), alone).all()


@pytest.mark.parametrize("fmt", ["row_flat", "column"])
@pytest.mark.parametrize("jointype", ["inner", "left"])
def test_three_relations_left_semi_then_the_tracked_one(sessions, jointype, fmt):
    w = general_world()
    d = w["d"]
    spec = ("(gpuhashjoin (rel (jointype left) (hashkey (var 1 int4) 1 int4) (hashkey (int8 (var 2 int2)) 2 int8)"
            " (qual (float8gt (ivar 1 3 float8) (var 3 float8))))"
            " (rel (hashkey (ivar 1 4 int4) 1 int4) (jointype semi) (qual (int2lt (ivar 2 2 int2) (param 0 int2))))"
            " (rel (track_matches) (hashkey (var 4 int4) 1 int4) (qual (int2gt (ivar 3 2 int2) (var 2 int2))) (jointype %s)))"
            % jointype)
    rels = jm.three_rel_model(d)[:2] + [
        jm.Rel(len(d["pk3"]), [jm.Key(jm.outer_column(d["fd"], d["fdn"]), d["pk3"], d["pk3n"])], jointype,
               lambda orow, irows, e: d["v3"][e] > d["fb"][orow])]
    s = sessions.get(("three", jointype), lambda: Session(spec, w["inners"], [[1, 2], [1], [1]],
                                                          ext=[np.int16(jm.PARAM_V2)]))
    assert s.join.tracked_depth() == 3
    want, unmatched = general_check(s, rels, fmt, False)
    # relation 2 is a SEMI filter in front: without it more entries of relation 3 would be matched
    alone = jm.join_model(np.arange(len(d["fa"])), [rels[2]])
    assert len(np.setdiff1d(np.unique(alone[:, -1]), [-1])) > s.nlast - len(unmatched)


# ---------------------------------------------------------------------------------------------
# 3. lost updates: 64 entries whose flags are neighbours, set from many work-groups at once
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_fast", [True, False], ids=["general", "one_pass"])
@pytest.mark.parametrize("pattern", ["every_group_every_key", "group_w_key_w"])
def test_neighbouring_flags_from_many_work_groups(sessions, pattern, no_fast, monkeypatch):
    """The GENERAL variant is the one that meets the bar of 32 work-groups: its grid is not capped, 40192
    rows are 157 tiles of 256 rows, one per work-group, so under "group_w_key_w" work-group w probes key
    w mod 64 and nothing else -- different work-groups set different flags of the same word.  The
    one-pass variant runs the same two chunks for completeness, with looser coverage: its tiles are
    thousands of rows (about 10 work-groups here), so each of them sees 16 or more neighbouring keys."""
    if no_fast:
        monkeypatch.setenv("STROM_HASHJOIN_NO_FAST", "1")
    monkeypatch.delenv("STROM_HASHJOIN_MAX_GRID", raising=False)
    nkeys, nrows = 64, 40192                    # 157 tiles of 256 rows for the general kernel: > 32 work-groups
    def make():
        inner = kds.build_kds("row_flat", [kds.Column("int4", np.arange(nkeys + 8, dtype=np.int32))])
        return Session(one_rel("inner"), [inner], [[1]])
    s = sessions.get("neighbours", make)                # keys 64 .. 71 are never probed
    rng = np.random.default_rng(9)
    if pattern == "every_group_every_key":
        fk = rng.integers(0, nkeys, nrows).astype(np.int32)
    else:
        fk = ((np.arange(nrows) // 256) % nkeys).astype(np.int32)       # work-group w: key w mod 64 only
    s.join.reset_matches()
    res = s.join.join_chunk(kds.build_kds("column", [kds.Column("int4", fk)]))
    assert res.errcode == 0 and res.nitems == nrows
    assert s.unmatched_ids().tolist() == list(range(nkeys, nkeys + 8))


# ---------------------------------------------------------------------------------------------
# 4. chunks, 5. room
# ---------------------------------------------------------------------------------------------
def chunk_world(sessions, jointype="left"):
    s = family_session(sessions, "fast", jointype)
    rng = np.random.default_rng(404)
    chunks = []
    for i in range(3):
        # each chunk draws its partners from its own third of the inner keys
        part = s.pk[i::3][~s.pkn[i::3]]
        fk = np.where(rng.random(5000) < 0.7, part[rng.integers(0, len(part) // 2, 5000)], -7 - i).astype(np.int32)
        rel = [jm.Rel(len(s.pk), [jm.Key(jm.outer_column(fk), s.pk, s.pkn)], jointype)]
        chunks.append((kds.build_kds("column", [kds.Column("int4", fk)]), jm.join_model(np.arange(5000), rel)))
    return s, chunks


def test_three_chunks_two_in_flight_then_reset(sessions):
    s, chunks = chunk_world(sessions)
    s.join.reset_matches()
    p0 = s.join.submit(chunks[0][0])
    p1 = s.join.submit(chunks[1][0])             # both in flight
    p2 = s.join.submit(chunks[2][0])
    # the unmatched pass orders itself behind all three, waited for or not
    got = s.unmatched_ids()
    for p in (p0, p1, p2):
        assert s.join.collect(p).errcode == 0
    matched = np.unique(np.concatenate([ojm.unmatched_from_records(w) for _, w in chunks]))
    assert np.array_equal(got, np.setdiff1d(np.arange(s.nlast), matched)) and 0 < len(matched) < s.nlast
    # ... after one chunk fewer entries are matched
    s.join.reset_matches()
    assert np.array_equal(s.unmatched_ids(), np.arange(s.nlast))
    s.feed(*chunks[1])
    assert np.array_equal(s.unmatched_ids(), np.setdiff1d(np.arange(s.nlast), ojm.unmatched_from_records(chunks[1][1])))


@pytest.mark.parametrize("no_fast", [False, True], ids=["one_pass", "general"])
def test_a_chunk_short_of_room_retried_leaves_the_same_flags(sessions, no_fast, monkeypatch):
    if no_fast:
        monkeypatch.setenv("STROM_HASHJOIN_NO_FAST", "1")
    s, chunks = chunk_world(sessions)
    outer, want = chunks[0]
    s.join.reset_matches()
    s.feed(outer, want)
    full = s.join.matches_image()
    s.join.reset_matches()
    short = s.join.collect(s.join.submit(outer, nrooms=len(want) // 2))
    assert short.errcode == ERR_NOSPACE and short.nitems == len(want)
    # a chunk that ends with DataStoreNoSpace has flagged all of its candidates
    assert np.array_equal(s.join.matches_image(), full)
    res = s.join.join_chunk(outer, nrooms=len(want) // 2)
    assert res.retried and res.nitems == len(want)
    assert np.array_equal(s.join.matches_image(), full)
    # a byte per 32-byte granule: 0x80 "an entry starts here" + its position, 0x40 "matched"
    assert set(np.unique(full & 0xC0)) == {0, 0x80, 0xC0} and not (full[(full & 0x80) == 0]).any()


def test_unmatched_room(sessions):
    s, chunks = chunk_world(sessions)
    s.join.reset_matches()
    s.feed(*chunks[2])
    want = np.setdiff1d(np.arange(s.nlast), ojm.unmatched_from_records(chunks[2][1]))
    assert len(want) > 3
    res = s.join.collect(s.join.submit_unmatched(nrooms=len(want)))
    assert res.errcode == 0 and np.array_equal(ojm.device_unmatched_rowids(s.dkm, res.records), want)
    res = s.join.collect(s.join.submit_unmatched(nrooms=len(want) - 1))
    assert res.errcode == ERR_NOSPACE and res.nitems == len(want)
    res = s.join.unmatched(nrooms=len(want) - 1)
    assert res.errcode == 0 and res.retried
    assert np.array_equal(ojm.device_unmatched_rowids(s.dkm, res.records), want)


# ---------------------------------------------------------------------------------------------
# 6. the unmatched pass's stage and grid
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nentries", [1, UNMATCHED_STAGE - 1, UNMATCHED_STAGE, UNMATCHED_STAGE + 1, 2 * UNMATCHED_STAGE + 1])
def test_one_work_group_walks_the_flag_area(nentries, monkeypatch):
    """nothing is matched, so every entry is staged: with UNMATCHED_STAGE entries the stage ends
    exactly full and leaves in the last flush, one more forces a flush in the middle"""
    monkeypatch.setenv("STROM_HASHJOIN_UNMATCHED_MAX_GRID", "1")
    inner = kds.build_kds("row_flat", [kds.Column("int4", np.arange(nentries, dtype=np.int32))])
    s = Session(one_rel("inner"), [inner], [[1]])
    try:
        assert np.array_equal(s.unmatched_ids(nrooms=nentries), np.arange(nentries))
        # ... and with every entry matched the pass returns nothing
        res = s.join.join_chunk(kds.build_kds("column", [kds.Column("int4", np.arange(nentries, dtype=np.int32))]))
        assert res.nitems == nentries
        res = s.join.unmatched()
        assert res.errcode == 0 and res.nitems == 0 and len(res.records) == 0
    finally:
        s.end()


# ---------------------------------------------------------------------------------------------
# 7. projections of unmatched records, 8. FULL JOIN .. GROUP BY
# ---------------------------------------------------------------------------------------------
NGROUPS = 23


@pytest.fixture(scope="module")
def full_join():
    """a FULL join: inner (key, int4 v with NULLs, float8 f, text w with NULLs), outer (key, int8 id,
    int4 g, text t); about a third of the entries stay unmatched"""
    runtime.init()
    rng = np.random.default_rng(808)
    ni, no = 900, 4001
    pk = rng.permutation(2000)[:ni].astype(np.int32)
    pkn = rng.random(ni) < 0.03
    v = rng.integers(-1000, 1000, ni).astype(np.int32)
    vn = rng.random(ni) < 0.1
    f = rng.random(ni) * 100 - 50
    w = [text_cases.WORDS[i] for i in rng.integers(0, len(text_cases.WORDS), ni)]
    wn = rng.random(ni) < 0.1
    live = pk[~pkn]
    fk = np.where(rng.random(no) < 0.8, live[rng.integers(0, 2 * len(live) // 3, no)], 5000).astype(np.int32)
    fkn = rng.random(no) < 0.04
    g = rng.integers(0, NGROUPS, no).astype(np.int32)
    t = [text_cases.WORDS[i] for i in rng.integers(0, len(text_cases.WORDS), no)]
    inner = kds.build_kds("row_flat", [kds.Column("int4", pk, pkn), kds.Column("int4", v, vn),
                                       kds.Column("float8", f), kds.Column("text", w, wn)])
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn), kds.Column("int8", np.arange(no, dtype=np.int64)),
                                     kds.Column("int4", g), kds.Column("text", t)])
    s = Session(one_rel("left"), [inner], [[1]])
    want = jm.join_model(np.arange(no), [jm.Rel(ni, [jm.Key(jm.outer_column(fk, fkn), pk, pkn)], "left")])
    unmatched = np.setdiff1d(np.arange(ni), ojm.unmatched_from_records(want))
    assert 0.2 < len(unmatched) / ni < 0.6 and pkn.any()
    s.feed(outer, want)
    yield dict(s=s, outer=outer, want=want, unmatched=unmatched, v=v, vn=vn, f=f, w=w, wn=wn, g=g, pk=pk, pkn=pkn)
    s.end()


def test_unmatched_projection_tupslot(full_join):
    c = full_join
    nitems, cols = c["s"].join.unmatched_project([(0, 2, "int8"), (1, 2, "int4"), (1, 3, "float8"), (0, 1, "int4")])
    (o, on), (v, vn), (f, fn), (k, kn) = cols
    assert nitems == len(c["unmatched"])
    assert on.all() and kn.all() and not o.any() and not k.any()       # the outer columns: NULL, value 0
    assert not fn.any()
    # which entry a row is: float8 f is unique per entry
    order = np.argsort(f)
    u = c["unmatched"][np.argsort(c["f"][c["unmatched"]])]
    assert np.array_equal(f[order].view(np.int64), c["f"][u].view(np.int64))
    assert np.array_equal(vn[order], c["vn"][u]) and np.array_equal(v[order][~vn[order]], c["v"][u][~c["vn"][u]])


def test_unmatched_projection_row_flat(full_join):
    c = full_join
    dest_columns = [(0, 2, "int8"), (1, 2, "int4"), (1, 3, "float8"), (1, 4, "text"), (0, 4, "text")]
    nitems, dest, recs = c["s"].join.unmatched_project_rows(dest_columns)
    assert nitems == len(c["unmatched"]) and not recs[:, 0].any()
    ids = entry_rowids(c["s"].dkm, 1, recs[:, 1])
    assert np.array_equal(np.sort(ids), c["unmatched"])
    rows = _walk_row_flat(dest, nitems, len(dest_columns))
    offs = zm.tuple_offsets(dest)
    for i in range(nitems):
        e = int(ids[i])
        want = [None, None if c["vn"][e] else c["v"][e].tobytes(), c["f"][e].tobytes(),
                None if c["wn"][e] else c["w"][e], None]
        assert rows[i] == want, (i, e)
        infomask = int(np.frombuffer(dest[offs[i] + 20:offs[i] + 22].tobytes(), dtype="<u2")[0])
        assert infomask & HEAP_HASNULL, (i, e)


def align(n, a):
    return (n + a - 1) & ~(a - 1)


def test_unmatched_projection_column(full_join):
    c = full_join
    dest_columns = [(0, 2, "int8"), (1, 2, "int4"), (1, 3, "float8"), (1, 4, "text"), (0, 4, "text"), (0, 3, "int4")]
    joined, nitems = c["s"].join.unmatched_to_column(dest_columns)
    try:
        image = joined.download()
    finally:
        joined.release()
    assert nitems == len(c["unmatched"]) == kds.KdsHead(image).nitems
    cols = kds.decode_column_chunk(image)
    f = cols[2]["values"].view(np.float64)
    assert cols[2]["notnull"] is None or cols[2]["notnull"].all()
    order = np.argsort(c["f"])
    e = order[np.searchsorted(c["f"][order], f)]           # the entry of every row
    assert np.array_equal(np.sort(e), c["unmatched"])
    # the outer columns: all NULL, by-value and text alike; a NULL text has offset 0
    for col in (0, 4, 5):
        assert cols[col]["notnull"] is not None and not cols[col]["notnull"].any(), col
        assert not cols[col]["values"].view(np.uint8).any(), col
    nn = cols[1]["notnull"]
    assert np.array_equal(~nn, c["vn"][e]) and np.array_equal(cols[1]["values"].view(np.int32)[nn], c["v"][e][nn])
    # the inner text column: the datum's bytes are the entry's
    text = kds.decode_text_column(image, 3)
    offs = cols[3]["values"].view(np.uint64)
    heap = 0
    for i in range(nitems):
        want = None if c["wn"][e[i]] else c["w"][e[i]]
        assert text[i] == want and (int(offs[i]) == 0) == (want is None), i
        if want is not None:
            heap += align(len(kds.varlena_datum(want)), 4)
    assert kds.decode_text_column(image, 4) == [None] * nitems
    head = kds.KdsHead(image)
    assert head.usage - cols[3]["extra_off"] == heap > 0         # the outer text column took no heap bytes
    # zone maps: of the content, and of what the model says the content is
    for col, t, vals, isnull in ((0, "int8", np.zeros(nitems, dtype=np.int64), np.ones(nitems, dtype=bool)),
                                 (1, "int4", c["v"][e], c["vn"][e]), (2, "float8", c["f"][e], None),
                                 (5, "int4", np.zeros(nitems, dtype=np.int32), np.ones(nitems, dtype=bool))):
        got_vals, got_null = zm.content(cols[col], t)
        assert zm.same(zm.of_decoded(cols[col]), zm.expected(t, got_vals, got_null)), col
        assert zm.same(zm.of_decoded(cols[col]), zm.expected(t, vals, isnull)), col


def test_full_join_group_by(full_join):
    """SELECT g, count(*), count(v) FROM outer FULL JOIN inner .. GROUP BY g: one session folds the
    COLUMN projection of the chunk's join and then that of the unmatched pass, whose g is NULL"""
    c = full_join
    s = c["s"]
    dest_columns = [(0, 3, "int4"), (1, 2, "int4")]
    agg = GpuPreAgg("(gpupreagg (key (var 1 int4)) (nrows) (nrows (isnotnull (var 2 int4))))")
    ds = runtime.DeviceStore.upload(c["outer"])
    parts = []
    try:
        s.join.reset_matches()
        agg.begin([(0, NGROUPS)])
        joined, n1 = s.join.join_to_column(ds, dest_columns)
        parts.append(joined)
        assert agg.fold(joined)[0] == 0
        rest, n2 = s.join.unmatched_to_column(dest_columns)
        parts.append(rest)
        assert agg.fold(rest)[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        for p in parts:
            p.release()
        ds.release()
    assert n1 == len(c["want"]) and n2 == len(c["unmatched"])
    keys, knull = pr.column(0)
    assert knull.sum() == 1 and len(pr) == NGROUPS + 1
    irow = np.empty(len(c["g"]), dtype=np.int64)
    irow[c["want"][:, 0] - 1] = c["want"][:, 1]
    has_v = (irow >= 0) & ~c["vn"][np.where(irow < 0, 0, irow)]
    order = np.argsort(keys[~knull])
    assert np.array_equal(keys[~knull][order], np.arange(NGROUPS))
    assert np.array_equal(pr.column(1)[0][~knull][order], np.bincount(c["g"], minlength=NGROUPS))
    assert np.array_equal(pr.column(2)[0][~knull][order], np.bincount(c["g"][has_v], minlength=NGROUPS))
    # the NULL group: the unmatched entries
    assert pr.column(1)[0][knull][0] == len(c["unmatched"])
    assert pr.column(2)[0][knull][0] == int((~c["vn"][c["unmatched"]]).sum())


# ---------------------------------------------------------------------------------------------
# 9. ranks, 10. refusals
# ---------------------------------------------------------------------------------------------
def test_two_tables_stand_in_for_two_ranks(sessions):
    s, chunks = chunk_world(sessions)
    other = Session(one_rel("left"), [kds.build_kds("row_flat", [kds.Column("int4", s.pk, s.pkn),
                                                                  kds.Column("int4", np.arange(len(s.pk), dtype=np.int32))])], [[1]])
    try:
        s.join.reset_matches()
        s.feed(*chunks[0])
        other.feed(*chunks[1])
        other.feed(*chunks[2])
        alone = s.unmatched_ids()
        s.join.merge_matches(other.join.matches_image())
        matched = np.unique(np.concatenate([ojm.unmatched_from_records(w) for _, w in chunks]))
        merged = s.unmatched_ids()
        assert np.array_equal(merged, np.setdiff1d(np.arange(s.nlast), matched)) and len(merged) < len(alone)
        # ... which is what one table fed everything says
        for outer, want in chunks:
            other.join.collect(other.join.submit(outer))
        assert np.array_equal(other.unmatched_ids(), merged)
        # an image of another length is refused
        with pytest.raises(runtime.StromError) as ei:
            s.join.merge_matches(np.zeros(16, dtype=np.uint8))
        assert ei.value.errcode == ERR_BAD_REQUEST
        # ... and one of the right length that is not of this table: an entry start that is not ours, a
        # start of ours missing, another position inside the granule; nothing of it is merged
        before = s.join.matches_image()
        for what in ("extra", "missing", "moved"):
            wrong = other.join.matches_image()
            at = int(np.flatnonzero(wrong == 0)[0]) if what == "extra" else int(np.flatnonzero(wrong & 0x80)[-1])
            wrong[at] = {"extra": 0xC0, "missing": 0, "moved": wrong[at] ^ 0x01}[what]
            wrong[wrong != 0] |= 0x40
            with pytest.raises(runtime.StromError) as ei:
                s.join.merge_matches(wrong)
            assert ei.value.errcode == ERR_BAD_REQUEST, what
            assert np.array_equal(s.join.matches_image(), before), what
        assert np.array_equal(s.unmatched_ids(), merged)
    finally:
        other.end()


def expect_bad_request(call):
    with pytest.raises(runtime.StromError) as ei:
        call()
    assert ei.value.errcode == ERR_BAD_REQUEST, ei.value


def test_refusals_and_the_tables_still_work(monkeypatch):
    monkeypatch.setenv("STROM_GPUPREAGG_LOOKUP_GENERIC", "1")
    runtime.init()
    rng = np.random.default_rng(31)
    nd, n = 300, 2003
    dkey = rng.permutation(nd).astype(np.int32)
    dgrp = (dkey % NGROUPS).astype(np.int32)
    dim = kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)])
    fk = rng.integers(0, nd // 2, n).astype(np.int32)
    a = rng.integers(0, 1000, n).astype(np.int32)
    ds = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", fk), kds.Column("int4", a)]))
    plain = GpuHashJoin(jm.one_rel_spec()).begin(build_multihash([(dim, [1])]))
    tracked = GpuHashJoin(one_rel("inner")).begin(build_multihash([(dim, [1])]))
    # a dimension of the dimension: keyed by column 2 of `dim`, untracked and tracked
    sub = kds.build_kds("row_flat", [kds.Column("int4", np.arange(NGROUPS, dtype=np.int32)),
                                     kds.Column("int4", (np.arange(NGROUPS) % 5).astype(np.int32))])
    child = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))").begin(build_multihash([(sub, [1])]))
    tracked_child = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4) (track_matches)))").begin(
        build_multihash([(sub, [1])]))
    agg = GpuPreAgg("(gpupreagg (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))))").begin([(0, NGROUPS)])
    columns = [(1, 2, "int4"), (0, 2, "int4")]
    try:
        assert plain.tracked_depth() == 0 and tracked.tracked_depth() == 1
        info = tracked.table_info(1)
        assert info["mode"] == "direct" and info["unique"]
        # the new calls on a table without tracking
        expect_bad_request(lambda: plain.unmatched())
        expect_bad_request(lambda: plain.unmatched_project([(1, 2, "int4")]))
        expect_bad_request(lambda: plain.unmatched_to_column([(1, 2, "int4")]))
        expect_bad_request(lambda: plain.reset_matches())
        expect_bad_request(lambda: plain.matches_image())
        expect_bad_request(lambda: plain.merge_matches(np.zeros(16, dtype=np.uint8)))
        assert plain.join_chunk(ds).nitems == n
        # the lookup folds on a tracked table: they would leave every flag clear
        expect_bad_request(lambda: agg.submit_lookup(tracked, ds, columns))
        expect_bad_request(lambda: agg.submit_lookup_star([tracked], ds, columns))
        expect_bad_request(lambda: agg.submit_lookup_star([plain, tracked], ds, columns))
        # ... the snowflake with the tracked table as the root and as a child (keyed by the root's
        # column 2); the same trees of untracked tables are accepted
        snow_cols = [(2, 2, "int4"), (0, 2, "int4")]
        expect_bad_request(lambda: agg.submit_lookup_snowflake([tracked], [0], ds, columns))
        expect_bad_request(lambda: agg.submit_lookup_snowflake([tracked, child], [0, 1], ds, snow_cols, [None, "int4"]))
        expect_bad_request(lambda: agg.submit_lookup_snowflake([plain, tracked_child], [0, 1], ds, snow_cols, [None, "int4"]))
        control = GpuPreAgg(agg.spec).begin([(0, NGROUPS)])
        try:
            assert control.collect(control.submit_lookup_snowflake([plain], [0], ds, columns))[0] == 0
            assert control.collect(control.submit_lookup_snowflake([plain, child], [0, 1], ds, snow_cols, [None, "int4"]))[0] == 0
        finally:
            control.end()
        # the joined fold over the records of the unmatched pass: they name no outer row
        up = tracked.submit_unmatched(flags=STROM_RESULTS_ON_DEVICE)
        try:
            expect_bad_request(lambda: agg.submit_joined(tracked, up, ds, columns))
        finally:
            assert tracked.collect(up).errcode == 0
        # a join's records go with their outer chunk, the unmatched pass's without
        jp = tracked.submit(ds, flags=STROM_RESULTS_ON_DEVICE)
        try:
            err = ctypes.c_int(0)
            one = np.array([1], dtype=np.int32)
            int4 = np.array([23], dtype=np.int32)
            assert not lib.strom_hashjoin_project_column(jp[0], tracked.table, None, 1, one.ctypes.data, one.ctypes.data,
                                                         int4.ctypes.data, ctypes.byref(err))
            assert err.value == ERR_BAD_REQUEST
            # the joined fold stays allowed: the join ran and flagged
            assert agg.collect(agg.submit_joined(tracked, jp, ds, columns))[0] == 0
        finally:
            assert tracked.collect(jp).errcode == 0
        pr = agg.fetch()
        grp = dgrp[np.argsort(dkey)][fk]
        keys, _ = pr.column(0)
        order = np.argsort(keys)
        assert np.array_equal(keys[order], np.unique(grp))
        assert np.array_equal(pr.column(1)[0][order], np.bincount(grp, minlength=NGROUPS)[np.unique(grp)])
        # ... and the tracked table still works
        res = tracked.unmatched()
        ids = np.sort(entry_rowids(tracked.device_kmhash(), 1, res.records[:, 1]))
        assert np.array_equal(ids, np.flatnonzero(~np.isin(dkey, fk)))
    finally:
        agg.end()
        plain.end()
        tracked.end()
        child.end()
        tracked_child.end()
        ds.release()
