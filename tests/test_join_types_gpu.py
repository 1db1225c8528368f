"""
LEFT OUTER, SEMI and ANTI joins on the device (needs an MI355X: -m gpu), against the nested-loop
model of tests/join_model.py: the exact set of records, inner row ids in place of entry offsets, -1
where a record's slot is 0 ("no entry").

The shapes are the kernels' edges, not the workload.  The one-pass kernels (strom_hashjoin.h:
gpuhashjoin_main_fast_body, one body for four entry points) differ from the inner join in their
emit predicate only, and the one new way for them to be wrong is the ragged last tile: under ANTI
and LEFT a row emits BECAUSE it found nothing, and the rows beyond nitems find nothing either.  So
every family runs 1, T-1, T, T+1 and 3T+1 rows with one work-group (STROM_HASHJOIN_MAX_GRID=1), over
three key mixes, and every case runs a second time under STROM_HASHJOIN_NO_FAST=1, which selects the
general kernel: both paths are compared with the same model without asking the library which ran.
Tile sizes and the index rules are those test_hashjoin_edges_gpu.py states; its tables are used.
"""
import ctypes

import numpy as np
import pytest

import join_model as jm
import text_cases
import zone_map_model as zm
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash, STROM_RESULTS_ON_DEVICE
from pg_strom_amd.gpupreagg import GpuPreAgg
from test_hashjoin_edges_gpu import FAMILIES, T_FAST, family_keys, outer_keys
from test_text_gpu import _walk_row_flat

pytestmark = pytest.mark.gpu

ERR_BAD_REQUEST = 101
ERR_NOSPACE = 301
HEAP_HASNULL = 0x0001


class Session(object):
    """one table, kept for every case that probes it"""

    def __init__(self, spec, inners, keys, ext=(), ratio=1.0):
        self.inners = inners
        self.join = GpuHashJoin(spec, row_population_ratio=ratio)
        try:
            self.join.begin(build_multihash(list(zip(inners, keys))), ext_params=ext)
            self.dkm = self.join.device_kmhash()
            self.info = [self.join.table_info(d + 1) for d in range(len(inners))]
        except Exception:
            self.join.end()
            raise

    def run(self, outer, nrooms=None, row_map=None):
        return self.join.collect(self.join.submit(outer, nrooms=nrooms, row_map=row_map))

    def check(self, outer, want, nrooms=None, row_map=None):
        """the records of one launch == the model's, exactly"""
        res = self.run(outer, nrooms=len(want) + 8 if nrooms is None else nrooms, row_map=row_map)
        assert res.errcode == 0 and res.nitems == len(want), (res.errcode, res.nitems, len(want))
        got = jm.records_to_rowids(self.dkm, res.records)
        assert np.array_equal(jm.sorted_records(got), jm.sorted_records(want))
        return res

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
# one-pass, per family
# ---------------------------------------------------------------------------------------------
# (a) about half the keys have a partner, some lie below key_min, some at or above key_min + nslots,
#     some are NULL: the column has a bitmap (the checked loader)
# (b) no NULL column and every key has a partner: ANTI returns nothing, LEFT and SEMI emit every row,
#     every stage group ends exactly full
# (c) no key has a partner: SEMI returns nothing, ANTI and LEFT emit every row
MIXES = {"a": (0.5, True), "b": (1.0, False), "c": (0.0, False)}
ROWS = ["one_row", "tile_less_one", "tile", "tile_and_one", "three_tiles_and_one"]
_MODELS = {}


def rows_of(family, where):
    T = FAMILIES[family][3]
    return {"one_row": 1, "tile_less_one": T - 1, "tile": T, "tile_and_one": T + 1, "three_tiles_and_one": 3 * T + 1}[where]


def family_session(sessions, family, jointype):
    def make():
        pk, pkn = family_keys(family)
        inner = kds.build_kds("row_flat", [kds.Column("int4", pk, pkn),
                                           kds.Column("int4", np.arange(len(pk), dtype=np.int32))])
        s = Session(jm.one_rel_spec(jointype), [inner], [[1]])
        s.pk, s.pkn = pk, pkn
        span, mode = FAMILIES[family][1], FAMILIES[family][4]
        assert s.info[0]["mode"] == mode and s.info[0]["unique"]
        if span is not None:
            assert s.info[0]["nslots"] == span
        return s
    return sessions.get((family, jointype), make)


def family_case(s, family, nrows, mix):
    """(outer chunk, keys, the model's memo) of a family's case: computed once, shared by the join
    types (the candidates of depth 1 do not depend on them), left unchanged"""
    key = (family, nrows, mix)
    if key not in _MODELS:
        rate, nulls = MIXES[mix]
        fk, fkn = outer_keys(s, family, nrows, rate, nulls)
        _MODELS[key] = dict(fk=fk, fkn=fkn, memo={}, outer=kds.build_kds("column", [kds.Column("int4", fk, fkn)]))
    return _MODELS[key]


def family_want(s, case, jointype):
    rel = [jm.Rel(len(s.pk), [jm.Key(jm.outer_column(case["fk"], case["fkn"]), s.pk, s.pkn)], jointype)]
    return jm.join_model(np.arange(len(case["fk"])), rel, memo=case["memo"])


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("where", ROWS)
@pytest.mark.parametrize("jointype", ["semi", "anti", "left"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_one_pass_families_at_the_tile_edges(sessions, family, jointype, where, mix, monkeypatch):
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = family_session(sessions, family, jointype)
    nrows = rows_of(family, where)
    case = family_case(s, family, nrows, mix)
    want = family_want(s, case, jointype)
    if mix == "b":
        assert len(want) == (0 if jointype == "anti" else nrows)
    if mix == "c":
        assert len(want) == (0 if jointype == "semi" else nrows)
    if mix == "a" and nrows > 100:
        assert 0 < len(want) < nrows or jointype == "left"
    if jointype == "left":
        assert len(want) == nrows                  # unique keys: every outer row exactly once
    res = s.check(case["outer"], want)
    assert res.perfmon["num_kern_prep"] == (1 if FAMILIES[family][5] else 0)
    # ... and the general kernel
    monkeypatch.setenv("STROM_HASHJOIN_NO_FAST", "1")
    res = s.check(case["outer"], want)
    assert res.perfmon["num_kern_prep"] == 0


# ---------------------------------------------------------------------------------------------
# duplicates: SEMI and ANTI stay one-pass, LEFT takes the general kernel
# ---------------------------------------------------------------------------------------------
def duplicate_session(sessions, family, jointype):
    def make():
        pk, pkn = family_keys(family)
        rng = np.random.default_rng(len(pk))
        rep = rng.integers(1, 4, len(pk))
        pk, pkn = np.repeat(pk, rep), np.repeat(pkn, rep)
        order = rng.permutation(len(pk))
        pk, pkn = pk[order], pkn[order]
        inner = kds.build_kds("row_flat", [kds.Column("int4", pk, pkn),
                                           kds.Column("int4", np.arange(len(pk), dtype=np.int32))])
        s = Session(jm.one_rel_spec(jointype), [inner], [[1]])
        s.pk, s.pkn = pk, pkn
        assert s.info[0]["mode"] == "direct" and not s.info[0]["unique"] and pkn.any()
        assert s.info[0]["nslots"] == FAMILIES[family][1]
        return s
    return sessions.get(("dup", family, jointype), make)


@pytest.mark.parametrize("jointype", ["semi", "anti", "left"])
@pytest.mark.parametrize("family", ["fast", "fast_lds"])
def test_duplicate_inner_keys(sessions, family, jointype, monkeypatch):
    """every inner key 1 .. 3 times, NULL inner keys: "slot is not empty" answers SEMI and ANTI;
    LEFT is not unique and emits one record per partner"""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = duplicate_session(sessions, family, jointype)
    nrows = FAMILIES[family][3] + 1
    fk, fkn = outer_keys(s, family, nrows, 0.5, True)
    stats = []
    rel = [jm.Rel(len(s.pk), [jm.Key(jm.outer_column(fk, fkn), s.pk, s.pkn)], jointype)]
    want = jm.join_model(np.arange(nrows), rel, stats=stats)
    assert jm.prefix_kinds(stats[0])
    if jointype == "left":
        assert len(want) > nrows
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn)])
    res = s.check(outer, want)
    # the staged kernel alone reports itself: SEMI / ANTI over duplicates take it, LEFT cannot
    assert res.perfmon["num_kern_prep"] == (1 if FAMILIES[family][5] and jointype != "left" else 0)


# ---------------------------------------------------------------------------------------------
# room
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jointype", ["anti", "left"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_result_room(sessions, family, jointype, monkeypatch):
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = family_session(sessions, family, jointype)
    nrows = rows_of(family, "tile_and_one")
    case = family_case(s, family, nrows, "a")
    want = family_want(s, case, jointype)
    assert len(want) > 3
    s.check(case["outer"], want, nrooms=len(want))
    res = s.run(case["outer"], nrooms=len(want) - 1)
    assert res.errcode == ERR_NOSPACE and res.nitems == len(want)
    res = s.join.join_chunk(case["outer"], nrooms=len(want) - 1)
    assert res.errcode == 0 and res.retried and res.nitems == len(want)
    got = jm.records_to_rowids(s.dkm, res.records)
    assert np.array_equal(jm.sorted_records(got), jm.sorted_records(want))


# ---------------------------------------------------------------------------------------------
# the general kernel, several relations
# ---------------------------------------------------------------------------------------------
PAIRS = [("left", "inner"), ("inner", "left"), ("left", "left"), ("semi", "inner"), ("inner", "anti"), ("anti", "semi")]
_GENERAL = {}


def general_world():
    if not _GENERAL:
        d = jm.general_data()
        _GENERAL["d"] = d
        for fmt in ("row", "row_flat", "column"):
            _GENERAL[fmt], _GENERAL["inners"] = jm.general_chunks(d, fmt)
        n = len(d["fa"])
        # every third row, from the end: a tile edge moves, a row comes before a lower one
        _GENERAL["row_map"] = np.arange(n, dtype=np.int32)[::-1][::3].copy()
    return _GENERAL


def general_check(s, rels, fmt, mapped):
    w = general_world()
    rows = w["row_map"] if mapped else np.arange(len(w["d"]["fa"]))
    stats = []
    want = jm.join_model(rows, rels, stats=stats)
    # per depth a prefix of each kind: no candidate, exactly one, several
    for depth, cnt in enumerate(stats, 1):
        assert jm.prefix_kinds(cnt), (depth, np.bincount(np.minimum(cnt, 2)))
    assert len(want) > 0
    s.check(w[fmt], want, row_map=w["row_map"] if mapped else None)
    return want


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("fmt", ["row", "row_flat", "column"])
@pytest.mark.parametrize("pair", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_two_relations(sessions, pair, fmt, mapped):
    w = general_world()
    s = sessions.get(("two", pair), lambda: Session(jm.two_rel_spec(*pair), w["inners"][:2], [[1, 2], [1]],
                                                    ext=[np.int16(jm.PARAM_V2)]))
    want = general_check(s, jm.two_rel_model(w["d"], *pair), fmt, mapped)
    if pair[0] == "left":
        # NULL-extended prefixes reached relation 2, whose key reads relation 1
        ext = want[want[:, 1] < 0]
        assert len(ext) > 0 or pair[1] == "inner"
        assert np.all(ext[:, 2] < 0)


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("fmt", ["row", "row_flat", "column"])
def test_three_relations_left_semi_anti(sessions, fmt, mapped):
    w = general_world()
    s = sessions.get("three", lambda: Session(jm.THREE_REL_SPEC, w["inners"], [[1, 2], [1], [1]],
                                              ext=[np.int16(jm.PARAM_V2)]))
    want = general_check(s, jm.three_rel_model(w["d"]), fmt, mapped)
    assert np.all(want[:, 2] == -1) and np.all(want[:, 3] == -1)


# ---------------------------------------------------------------------------------------------
# text and character(n) keys
# ---------------------------------------------------------------------------------------------
LONG = b"L" * 200                                # a 4-byte header


def text_key_case(sqltype):
    outer_vals = [b"a ", b"a", None, LONG, b"absent", b"b", b""]
    inner_vals = [b"a", LONG, b"b", b"b", None, b"zz"]
    n = 301
    ov = [outer_vals[(i * 3 + i // 7) % len(outer_vals)] for i in range(n)]
    iv = list(inner_vals)
    if sqltype == "character":
        pad = lambda v: None if v is None else (v + b" " * 210)[:210]      # character(210)
        ov, iv = [pad(v) for v in ov], [pad(v) for v in iv]
    assert len(kds.varlena_datum(LONG)) >= 127 + 4
    return ov, iv


def text_model_column(vals, sqltype):
    isnull = np.array([v is None for v in vals])
    key = [b"" if v is None else (text_cases.bpchar_key(v) if sqltype == "character" else bytes(v)) for v in vals]
    arr = np.empty(len(key), dtype=object)
    arr[:] = key
    return arr, isnull


@pytest.mark.parametrize("fmt", ["row_flat", "column"])
@pytest.mark.parametrize("jointype", ["semi", "anti"])
@pytest.mark.parametrize("sqltype", ["text", "character"])
def test_text_keys(sessions, sqltype, jointype, fmt):
    ov, iv = text_key_case(sqltype)
    inull = np.array([v is None for v in iv])
    onull = np.array([v is None for v in ov])

    def make():
        inner = kds.build_kds("row_flat", [kds.Column(sqltype, iv, inull),
                                           kds.Column("int4", np.arange(len(iv), dtype=np.int32))])
        return Session(jm.one_rel_spec(jointype, sqltype), [inner], [[1]])
    s = sessions.get(("text", sqltype, jointype), make)
    outer = kds.build_kds(fmt, [kds.Column(sqltype, ov, onull), kds.Column("int4", np.arange(len(ov), dtype=np.int32))])
    okey, okn = text_model_column(ov, sqltype)
    ikey, ikn = text_model_column(iv, sqltype)
    stats = []
    want = jm.join_model(np.arange(len(ov)), [jm.Rel(len(iv), [jm.Key(jm.outer_column(okey, okn), ikey, ikn)], jointype)],
                         stats=stats)
    assert jm.prefix_kinds(stats[0])
    # 'a ' and 'a': two keys as text, one as character(n)
    a_blank = [i for i, v in enumerate(ov) if v is not None and v.rstrip(b" ") == b"a" and v[:2] == b"a "]
    assert a_blank and all((stats[0][i] > 0) == (sqltype == "character") for i in a_blank)
    assert 0 < len(want) < len(ov)
    s.check(outer, want)


# ---------------------------------------------------------------------------------------------
# projections of a LEFT join: "no entry" is NULL
# ---------------------------------------------------------------------------------------------
N_PROJ = 3 * T_FAST // 2
NGROUPS = 37


@pytest.fixture(scope="module")
def left_projection():
    """the _fast family's keys with an int4, a float8 and a text column behind them; about a third of
    the outer rows have no partner.  The model's records, once."""
    runtime.init()
    pk, pkn = family_keys("fast")
    rng = np.random.default_rng(77)
    n = len(pk)
    v = rng.integers(-1000, 1000, n).astype(np.int32)
    vn = rng.random(n) < 0.1
    f = rng.random(n) * 100 - 50
    w = [text_cases.WORDS[i] for i in rng.integers(0, len(text_cases.WORDS), n)]
    wn = rng.random(n) < 0.1
    inner = kds.build_kds("row_flat", [kds.Column("int4", pk, pkn), kds.Column("int4", v, vn),
                                       kds.Column("float8", f), kds.Column("text", w, wn)])
    s = Session(jm.one_rel_spec("left"), [inner], [[1]])
    s.pk, s.pkn = pk, pkn
    assert s.info[0]["mode"] == "direct" and s.info[0]["unique"]
    fk, fkn = outer_keys(s, "fast", N_PROJ, 0.67, True)
    g = rng.integers(0, NGROUPS, N_PROJ).astype(np.int32)
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn), kds.Column("int8", np.arange(N_PROJ, dtype=np.int64)),
                                     kds.Column("int4", g)])
    want = jm.join_model(np.arange(N_PROJ), [jm.Rel(n, [jm.Key(jm.outer_column(fk, fkn), pk, pkn)], "left")])
    assert len(want) == N_PROJ
    irow = np.empty(N_PROJ, dtype=np.int64)
    irow[want[:, 0] - 1] = want[:, 1]           # the partner of every outer row, or -1
    none = irow < 0
    assert 0.2 < none.mean() < 0.45
    at = np.where(none, 0, irow)
    case = dict(s=s, outer=outer, g=g, irow=irow, none=none,
                v=v[at], vn=vn[at] | none, f=f[at], fn=none.copy(),
                w=[None if (none[i] or wn[at[i]]) else w[at[i]] for i in range(N_PROJ)])
    yield case
    s.end()


def test_left_projection_tupslot(left_projection):
    c = left_projection
    nitems, cols = c["s"].join.join_chunk_project(c["outer"], [(0, 2, "int8"), (1, 2, "int4"), (1, 3, "float8"), (1, 1, "int4")])
    assert nitems == N_PROJ
    (o, on), (v, vn), (f, fn), (k, kn) = cols
    assert not on.any() and np.array_equal(np.sort(o), np.arange(N_PROJ))
    assert np.array_equal(vn, c["vn"][o]) and np.array_equal(v[~vn], c["v"][o][~vn])
    assert np.array_equal(fn, c["fn"][o]) and np.array_equal(f[~fn].view(np.int64), c["f"][o][~fn].view(np.int64))
    assert np.array_equal(kn, c["none"][o])
    assert not v[vn].any() and not f[fn].any()          # a NULL's value is 0, not the table head's bytes


def test_left_projection_row_flat(left_projection):
    c = left_projection
    dest_columns = [(0, 2, "int8"), (1, 2, "int4"), (1, 3, "float8"), (1, 4, "text")]
    nitems, dest, recs = c["s"].join.join_chunk_project_rows(c["outer"], dest_columns)
    assert nitems == N_PROJ
    rows = _walk_row_flat(dest, nitems, len(dest_columns))
    offs = zm.tuple_offsets(dest)
    seen = np.zeros(N_PROJ, dtype=bool)
    for i in range(nitems):
        o = int(recs[i, 0]) - 1
        seen[o] = True
        assert (recs[i, 1] == 0) == bool(c["none"][o])
        want = [np.int64(o).tobytes(), None if c["vn"][o] else c["v"][o].tobytes(),
                None if c["fn"][o] else c["f"][o].tobytes(), c["w"][o]]
        assert rows[i] == want, (i, o)
        infomask = int(np.frombuffer(dest[offs[i] + 20:offs[i] + 22].tobytes(), dtype="<u2")[0])
        if c["none"][o]:
            assert infomask & HEAP_HASNULL, (i, o)
        assert bool(infomask & HEAP_HASNULL) == any(x is None for x in want), (i, o)
    assert seen.all()


def align(n, a):
    return (n + a - 1) & ~(a - 1)


def test_left_projection_column_and_a_preagg_over_it(left_projection):
    c = left_projection
    ds = runtime.DeviceStore.upload(c["outer"])
    dest_columns = [(0, 2, "int8"), (1, 2, "int4"), (1, 3, "float8"), (1, 4, "text"), (0, 3, "int4")]
    agg = GpuPreAgg("(gpupreagg (key (var 5 int4)) (nrows) (nrows (isnotnull (var 2 int4))))")
    joined = None
    try:
        joined, nitems = c["s"].join.join_to_column(ds, dest_columns)
        image = joined.download()
        agg.begin([(0, NGROUPS)])
        assert agg.fold(joined)[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        if joined is not None:
            joined.release()
        ds.release()
    assert nitems == N_PROJ == kds.KdsHead(image).nitems
    cols = kds.decode_column_chunk(image)
    o = cols[0]["values"].astype(np.int64)
    assert cols[0]["notnull"] is None and np.array_equal(np.sort(o), np.arange(N_PROJ))
    # values and the nulls bitmaps
    for col, vals, isnull, view in ((1, c["v"], c["vn"], np.int32), (2, c["f"], c["fn"], np.int64)):
        nn = cols[col]["notnull"]
        assert nn is not None and np.array_equal(~nn, isnull[o])
        got = cols[col]["values"].view(view)
        assert np.array_equal(got[nn], vals[o][nn].view(view))
    # text: NULL has offset 0 and takes no heap bytes
    text = kds.decode_text_column(image, 3)
    offs = cols[3]["values"].view(np.uint64)
    heap = 0
    for i in range(N_PROJ):
        want = c["w"][o[i]]
        assert text[i] == want, i
        assert (int(offs[i]) == 0) == (want is None), i
        assert bool(cols[3]["notnull"][i]) == (want is not None), i
        if want is not None:
            heap += align(len(kds.varlena_datum(want)), 4)
    head = kds.KdsHead(image)
    assert head.usage - cols[3]["extra_off"] == heap > 0
    # zone maps: of the content, and of what the model says the content is
    for col, t, vals, isnull in ((0, "int8", o, None), (1, "int4", c["v"][o], c["vn"][o]),
                                 (2, "float8", c["f"][o], c["fn"][o]), (4, "int4", c["g"][o], None)):
        got_vals, got_null = zm.content(cols[col], t)
        assert zm.same(zm.of_decoded(cols[col]), zm.expected(t, got_vals, got_null)), col
        assert zm.same(zm.of_decoded(cols[col]), zm.expected(t, vals, isnull)), col
    # count(*), count(inner column) GROUP BY outer key: the NULLs arrive as NULLs
    keys, _ = pr.column(0)
    order = np.argsort(keys)
    assert np.array_equal(keys[order], np.arange(NGROUPS))
    assert np.array_equal(pr.column(1)[0][order], np.bincount(c["g"], minlength=NGROUPS))
    assert np.array_equal(pr.column(2)[0][order], np.bincount(c["g"][~c["vn"]], minlength=NGROUPS))
    assert c["vn"].sum() > c["none"].sum() > 0


# ---------------------------------------------------------------------------------------------
# semi / anti result as a row map
# ---------------------------------------------------------------------------------------------
def test_semi_and_anti_row_maps_feed_a_preagg_and_partition_the_chunk():
    """... FROM fact WHERE [NOT] EXISTS (...) GROUP BY g, without a host round trip"""
    runtime.init()
    case = jm.duplicates_case(nouter=T_FAST + 5, ninner=500, seed=19)
    fk, fkn = case["fk"], case["fkn"]
    n = len(fk)
    rng = np.random.default_rng(5)
    g = rng.integers(0, NGROUPS, n).astype(np.int32)
    x = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    ds = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", fk, fkn), kds.Column("int4", g),
                                                             kds.Column("int4", x)]))
    joins = {t: GpuHashJoin(jm.one_rel_spec(t)).begin(build_multihash([(case["inner"], [1])]))
             for t in ("semi", "anti", "inner", "left")}
    nvalids = {}
    try:
        assert not joins["semi"].table_info(1)["unique"]
        for t in ("semi", "anti"):
            want = jm.join_model(np.arange(n), jm.one_rel_model(case, t))
            rows = np.sort(want[:, 0] - 1)
            assert 0 < len(rows) < n
            pending = joins[t].submit(ds, flags=STROM_RESULTS_ON_DEVICE)
            rmap = joins[t].row_map(pending)
            agg = GpuPreAgg("(gpupreagg (key (var 2 int4)) (nrows) (psum (int8 (var 3 int4))))").begin([(0, NGROUPS)])
            try:
                res = joins[t].collect(pending)
                assert res.errcode == 0 and res.nitems == len(rows) == rmap.nvalids
                nvalids[t] = rmap.nvalids
                assert agg.collect(agg.submit(ds, row_map=rmap))[0] == 0
                pr = agg.fetch()
            finally:
                agg.end()
                rmap.release()
            keys, _ = pr.column(0)
            order = np.argsort(keys)
            ug = np.unique(g[rows])
            assert np.array_equal(keys[order], ug)
            assert np.array_equal(pr.column(1)[0][order], np.bincount(g[rows], minlength=NGROUPS)[ug])
            sums = np.zeros(NGROUPS, dtype=np.int64)
            np.add.at(sums, g[rows], x[rows].astype(np.int64))
            assert np.array_equal(pr.column(2)[0][order], sums[ug])
        # a row with a NULL key is in the ANTI map and in no other: the two maps partition the chunk
        assert fkn.any() and nvalids["semi"] + nvalids["anti"] == n
        for t in ("inner", "left"):
            pending = joins[t].submit(ds, nrooms=4 * n, flags=STROM_RESULTS_ON_DEVICE)
            try:
                with pytest.raises(runtime.StromError) as ei:
                    joins[t].row_map(pending)
                assert ei.value.errcode == ERR_BAD_REQUEST
            finally:
                assert joins[t].collect(pending).errcode == 0
        # ... and a SEMI join whose results went to the host has nothing on the device to map
        pending = joins["semi"].submit(ds)
        try:
            with pytest.raises(runtime.StromError) as ei:
                joins["semi"].row_map(pending)
            assert ei.value.errcode == ERR_BAD_REQUEST
        finally:
            joins["semi"].collect(pending)
    finally:
        for j in joins.values():
            j.end()
        ds.release()


# ---------------------------------------------------------------------------------------------
# refusals: the fused folds are an inner join's
# ---------------------------------------------------------------------------------------------
def test_fused_folds_refuse_a_left_table_and_fold_nothing(monkeypatch):
    """a table that would otherwise qualify (DIRECT, unique, a plain outer key) built from a
    (jointype left) program: BadRequest, nothing launched -- the one good request afterwards has
    the counts of exactly one fold -- and join_to_column still serves it"""
    monkeypatch.setenv("STROM_GPUPREAGG_LOOKUP_GENERIC", "1")
    runtime.init()
    rng = np.random.default_rng(2917)
    nd, n = 500, 5003
    dkey = rng.permutation(nd).astype(np.int32)
    dgrp = (dkey % NGROUPS).astype(np.int32)
    dim = kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)])
    fk = rng.integers(-20, nd + 100, n).astype(np.int32)
    fkn = rng.random(n) < 0.03
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    ds = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", fk, fkn), kds.Column("int4", a)]))
    left = GpuHashJoin(jm.one_rel_spec("left")).begin(build_multihash([(dim, [1])]))
    inner = GpuHashJoin(jm.one_rel_spec()).begin(build_multihash([(dim, [1])]))
    agg = GpuPreAgg("(gpupreagg (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))))").begin([(0, NGROUPS)])
    columns = [(1, 2, "int4"), (0, 2, "int4")]
    joined = None

    def expect_bad_request(call):
        with pytest.raises(runtime.StromError) as ei:
            call()
        assert ei.value.errcode == ERR_BAD_REQUEST, ei.value

    try:
        info = left.table_info(1)
        assert info["mode"] == "direct" and info["unique"]
        expect_bad_request(lambda: agg.submit_lookup(left, ds, columns))
        expect_bad_request(lambda: agg.submit_lookup_star([left], ds, columns))
        # (relation 2 serves no column: an existence filter, which a LEFT join is not)
        expect_bad_request(lambda: agg.submit_lookup_star([inner, left], ds, columns))
        jp = left.submit(ds, flags=STROM_RESULTS_ON_DEVICE)
        try:
            expect_bad_request(lambda: agg.submit_joined(left, jp, ds, columns))
        finally:
            assert left.collect(jp).errcode == 0    # (a refused request leaves the join's task to its owner)
        # nothing was folded, and the session still works
        assert agg.collect(agg.submit_lookup(inner, ds, columns))[0] == 0
        pr = agg.fetch()
        joined, nitems = left.join_to_column(ds, [(0, 2, "int4"), (1, 2, "int4")])
        image = joined.download()
    finally:
        if joined is not None:
            joined.release()
        agg.end()
        left.end()
        inner.end()
        ds.release()
    pos = np.full(nd + 200, -1, dtype=np.int64)
    pos[dkey] = np.arange(nd)
    partner = np.where(fkn | (fk < 0), -1, pos[np.clip(fk, 0, nd + 199)])
    have = partner >= 0
    grp = dgrp[partner[have]]
    keys, _ = pr.column(0)
    order = np.argsort(keys)
    assert np.array_equal(keys[order], np.unique(grp))
    assert np.array_equal(pr.column(1)[0][order], np.bincount(grp, minlength=NGROUPS)[np.unique(grp)])
    sums = np.zeros(NGROUPS, dtype=np.int64)
    np.add.at(sums, grp, a[have].astype(np.int64))
    assert np.array_equal(pr.column(2)[0][order], sums[np.unique(grp)])
    # the general projection of the LEFT join: every outer row once, NULL where it has no partner
    assert nitems == n
    cols = kds.decode_column_chunk(image)
    got_a = cols[0]["values"].astype(np.int64)
    nn = cols[1]["notnull"]
    assert nn is not None and int((~nn).sum()) == int((~have).sum()) > 0
    pairs = np.stack([got_a, np.where(nn, cols[1]["values"].astype(np.int64), -1)], axis=1)
    want = np.stack([a.astype(np.int64), np.where(have, dgrp[np.where(have, partner, 0)], -1).astype(np.int64)], axis=1)
    assert np.array_equal(jm.sorted_records(pairs), jm.sorted_records(want))
