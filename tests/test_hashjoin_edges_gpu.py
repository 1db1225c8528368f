"""
The main join kernels at the edges of their own geometry (needs an MI355X: -m gpu).

gpuhashjoin_main_fast / _fast_narrow / _fast_lds / _fast_keyed are ONE body (strom_hashjoin.h:
gpuhashjoin_main_fast_body): a tile is 256 x 4 x quads rows, a full tile takes the straight-line
loaders (without the bitmap words when no column has a NULL bitmap), the ragged last one checks every
row; matches are compacted into a 4096-record LDS stage that is flushed with one reservation, and the
fill of the stage carries over from tile to tile.  gpuhashjoin_main (any format, row map, duplicate
keys, several relations) gives a thread ceil(rows / (work-groups x 256)) rows, up to 64, in four
slices of 16; it counts a whole tile, reserves once, and emits slice by slice through a 32 KB stage, or
directly when a slice's records do not fit it.  What either can get wrong shows at small shapes, once
STROM_HASHJOIN_MAX_GRID lets one work-group walk many tiles: one row, a tile less one, exactly a tile,
a tile and one; a stage that ends exactly full; result room of exactly the needed size and one less; a
slice boundary, a tile boundary; the stage's capacity at equality and one above.

Reference: a plain numpy join (sorted inner keys, searchsorted left / right, the matches expanded, NULL
keys dropped on both sides): the exact set of (outer row + 1, inner row id) records.  The device's entry
offsets are translated with entry_rowids and both sides compared after lexsort.  Every comparison is
exact.  One case per family is also compared with the CPU oracle, which ties the two references.
"""
import os

import numpy as np
import pytest

import oracle_binding as oracle
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash, entry_rowids

pytestmark = pytest.mark.gpu

C3_SPEC = "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))"
INT8_SPEC = "(gpuhashjoin (rel (hashkey (var 1 int8) 1 int8)))"
# the spec of test_outer_only_qual_pulled_up_into_the_join (HASHJOIN_FAST_OUTER_QUAL)
QUAL_SPEC = ("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)"
             " (qual (and (int4lt (var 2 int4) (param 0 int4)) (float8gt (var 3 float8) (param 1 float8))))))")
QUAL_EXT = [np.int32(2**30), 0.25]
# the spec of test_two_relations_multi_key_quals_and_row_map
TWO_REL_SPEC = ("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (hashkey (int8 (var 2 int2)) 2 int8)"
                " (qual (float8gt (ivar 1 3 float8) (var 3 float8))))"
                " (rel (hashkey (ivar 1 4 int4) 1 int4) (qual (int2lt (ivar 2 2 int2) (param 0 int2)))))")

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
ERR_NOSPACE = 301
ERR_BUILD = -11

# Nothing hands a launch's kernel or tile size to Python, so this file repeats the host's rules
# (gpuhashjoin.cpp: strom_hashjoin_table_create and gpuhashjoin_launch); a change there has to be
# repeated here, or the row counts stop sitting on the tile edges:
#   * one integer key whose range is <= 2^27 and <= max(8 x entries, 65536): a DIRECT slot array of
#     `range` 4-byte slots; any other single integer key: a KEYED index
#   * one relation, DIRECT or KEYED, unique keys, a COLUMN outer chunk, no row map: a one-pass kernel;
#     KEYED -> _fast_keyed; DIRECT with more than 262144 slots (a 4-byte array beyond 1 MB) -> the
#     3-byte slots of _fast_narrow; DIRECT with align256(4 x slots) <= 32 KB -> _fast_lds, which
#     alone reports itself (num_kern_prep == 1); every other DIRECT table -> _fast
#   * everything else (here: a row map) -> gpuhashjoin_main
#   * tile rows = 256 x 4 x quads: HASHJOIN_LDS_QUADS (8) for _fast_lds, HASHJOIN_FAST_QUADS (4) for
#     _fast and _fast_narrow, HASHJOIN_QUADS (2) for _fast_keyed; the stage takes HASHJOIN_STAGE (4096)
#     records
#   * work-groups = min(tiles, CUs x blocks per CU, STROM_HASHJOIN_MAX_GRID)
BLOCK = 256
T_LDS = BLOCK * 4 * int(os.environ.get("STROM_HASHJOIN_LDS_QUADS", "8"))
T_FAST = BLOCK * 4 * int(os.environ.get("STROM_HASHJOIN_FAST_QUADS", "4"))
T_KEYED = BLOCK * 4 * int(os.environ.get("STROM_HASHJOIN_QUADS", "2"))

# family: (inner keys, key span or None for "anywhere in int4", key_min, tile rows, mode, staged in LDS)
# fast_lds: 6001 slots, no multiple of 4 (the 16-byte LDS copy); fast_narrow: 300001 slots <= 8 x 40000,
# and 300001 mod 4 == 1: the last packed quad of hashjoin_narrow_slots_kernel is partial
FAMILIES = {
    "fast_lds": (5000, 6001, -1234, T_LDS, "direct", True),
    "fast": (20000, 25000, 0, T_FAST, "direct", False),
    "fast_narrow": (40000, 300001, 100000, T_FAST, "direct", False),
    "fast_keyed": (3000, None, 0, T_KEYED, "keyed", False),
}


def numpy_join(fk, fkn, pk, pkn):
    """(outer row + 1, inner row id) of every pair with equal, non-NULL keys"""
    rid = np.arange(len(pk)) if pkn is None else np.flatnonzero(~np.asarray(pkn, dtype=bool))
    order = np.argsort(pk[rid], kind="stable")
    rid = rid[order]
    sk = pk[rid]
    lo = np.searchsorted(sk, fk, side="left")
    cnt = np.searchsorted(sk, fk, side="right") - lo
    if fkn is not None:
        cnt[np.asarray(fkn, dtype=bool)] = 0
    orow = np.repeat(np.arange(len(fk)), cnt)
    within = np.arange(len(orow)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    irow = rid[np.repeat(lo, cnt) + within]
    return orow, irow


def sorted_records(recs):
    return recs[np.lexsort(recs.T[::-1])]


def records_of(*cols):
    return np.stack([np.asarray(c).astype(np.int32) for c in cols], axis=1).reshape(-1, len(cols))


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
        """the records of one launch == want, exactly"""
        res = self.run(outer, nrooms=nrooms, row_map=row_map)
        assert res.errcode == 0 and res.nitems == len(want)
        got = np.empty_like(res.records)
        got[:, 0] = res.records[:, 0]
        for d in range(len(self.inners)):
            got[:, d + 1] = entry_rowids(self.dkm, d + 1, res.records[:, d + 1])
        assert np.array_equal(sorted_records(got), sorted_records(want))
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


def family_keys(family):
    """inner keys of a family: unique, a NULL on one row in a hundred; the DIRECT ones sit on slot 0
    and on the last slot of their array"""
    nkeys, span, key_min = FAMILIES[family][:3]
    rng = np.random.default_rng(sum(family.encode()))
    if span is None:
        pk = np.unique(rng.integers(INT32_MIN + 1, INT32_MAX, nkeys + 100, dtype=np.int64))
        pk = pk[(pk != -1) & (pk != 8192)]      # (outer_keys: key_min - 1 and key_min + nslots of this index)
        pk = rng.permutation(pk)[:nkeys].astype(np.int32)
    else:
        pk = (1 + rng.permutation(span - 2)[:nkeys]).astype(np.int64) + key_min
        pk[0], pk[1] = key_min, key_min + span - 1
        pk = pk.astype(np.int32)
    pkn = rng.random(nkeys) < 0.01
    pkn[:2] = False
    return pk, pkn


def family_session(sessions, family, spec=C3_SPEC, ext=()):
    def make():
        pk, pkn = family_keys(family)
        inner = kds.build_kds("row_flat", [kds.Column("int4", pk, pkn),
                                           kds.Column("int4", np.arange(len(pk), dtype=np.int32))])
        s = Session(spec, [inner], [[1]], ext=ext)
        s.pk, s.pkn = pk, pkn
        span, mode = FAMILIES[family][1], FAMILIES[family][4]
        info = s.info[0]
        assert info["mode"] == mode and info["unique"]
        if span is not None:
            assert info["nslots"] == span
        assert (info["nslots"] > 262144) == (family == "fast_narrow")
        return s
    return sessions.get((family, spec), make)


def outer_keys(s, family, nrows, rate, nulls):
    """an outer key column that matches at about `rate`: partners are drawn from the inner keys (those
    of NULL inner rows among them: no partner), the others from values no inner row has -- holes of
    the slot array, both neighbours of the array, both ends of int4.  With a bitmap the very first
    and the very last row are NULL, over keys that would match."""
    nkeys, span, key_min = FAMILIES[family][:3]
    rng = np.random.default_rng(7919 * nrows)
    valid = s.pk[~s.pkn]
    nslots = s.info[0]["nslots"]
    specials = np.array([key_min - 1, key_min + nslots, INT32_MIN, INT32_MAX], dtype=np.int64)
    if span is None:
        miss = rng.integers(INT32_MIN, INT32_MAX, 4096, dtype=np.int64)
    else:
        miss = key_min + np.arange(span, dtype=np.int64)
    miss = np.concatenate([np.setdiff1d(miss, s.pk[~s.pkn]), specials])
    if rate >= 1.0:
        fk = valid[rng.integers(0, len(valid), nrows)].astype(np.int64)
    elif rate <= 0.0:
        fk = miss[rng.integers(0, len(miss), nrows)]
    else:
        fk = np.where(rng.random(nrows) < rate, s.pk[rng.integers(0, nkeys, nrows)].astype(np.int64),
                      miss[rng.integers(0, len(miss), nrows)])
        fk[0] = s.pk[0]                         # slot 0
        fk[-1] = s.pk[1]                        # the last slot
        k = max(0, min(len(specials), nrows - 2))
        fk[1:1 + k] = specials[:k]
    fkn = None
    if nulls:
        fkn = rng.random(nrows) < 0.05
        fkn[0] = fkn[-1] = True
    return fk.astype(np.int32), fkn


def probe_family(s, family, nrows, rate, nulls):
    fk, fkn = outer_keys(s, family, nrows, rate, nulls)
    orow, irow = numpy_join(fk, fkn, s.pk, s.pkn)
    want = records_of(orow + 1, irow)
    if rate >= 1.0 and not nulls:
        assert len(want) == nrows
    if rate <= 0.0:
        assert len(want) == 0
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn)])
    res = s.check(outer, want)
    assert res.perfmon["num_kern_prep"] == (1 if FAMILIES[family][5] else 0)
    return outer, want


# ---------------------------------------------------------------------------------------------
# the one-pass kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("where", ["one_row", "three_rows", "tile_less_one", "tile", "tile_and_one",
                                   "two_tiles_and_three"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_row_counts_around_one_tile(sessions, family, where, nulls):
    """the three loaders of a tile (full without bitmaps, full with bitmaps, ragged), fewer rows than
    a quad, and the row bound of the ragged tile; about half the rows match"""
    T = FAMILIES[family][3]
    nrows = {"one_row": 1, "three_rows": 3, "tile_less_one": T - 1, "tile": T, "tile_and_one": T + 1,
             "two_tiles_and_three": 2 * T + 3}[where]
    probe_family(family_session(sessions, family), family, nrows, 0.5, nulls)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_numpy_model_and_oracle_agree(sessions, family):
    """the oracle's records for one of the cases above are the numpy model's, and the device's"""
    s = family_session(sessions, family)
    outer, want = probe_family(s, family, FAMILIES[family][3] + 1, 0.5, True)
    rc, n, recs = oracle.gpuhashjoin(C3_SPEC, outer, s.inners)
    assert rc == 0 and n == len(want)
    assert np.array_equal(sorted_records(recs), sorted_records(want))


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("rate", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("max_grid,tiles,extra", [(1, 5, 5), (3, 7, 1)])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_work_group_walks_many_tiles(sessions, family, max_grid, tiles, extra, rate, nulls, monkeypatch):
    """the stage's fill carries over from tile to tile and is flushed when the next group of quads may
    not fit: never filled at 0 %, flushed half full at 50 %, and at 100 % without NULLs the keyed
    kernel's 2048-row tiles leave it exactly full (fill == HASHJOIN_STAGE_ENTRIES) every second tile,
    while the others flush a full group each time; the last tile is ragged"""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", str(max_grid))
    T = FAMILIES[family][3]
    probe_family(family_session(sessions, family), family, tiles * T + extra, rate, nulls)


@pytest.mark.parametrize("room", ["exact", "one_short", "half"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_result_room(sessions, family, room, monkeypatch):
    """room for exactly the records there are: success; one record less: DataStoreNoSpace and nitems
    is the room a retry needs.  With one work-group the flushes come one after the other, so one
    record short fails the last of them; half the room fails an earlier one, and the flushes after
    it have to go on counting."""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = family_session(sessions, family)
    nrows = 3 * FAMILIES[family][3] + 1
    fk, fkn = outer_keys(s, family, nrows, 0.5, False)
    orow, irow = numpy_join(fk, fkn, s.pk, s.pkn)
    want = records_of(orow + 1, irow)
    assert len(want) > 3
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn)])
    if room == "exact":
        s.check(outer, want, nrooms=len(want))
    else:
        res = s.run(outer, nrooms=len(want) - 1 if room == "one_short" else len(want) // 2)
        assert res.errcode == ERR_NOSPACE and res.nitems == len(want)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_pulled_up_outer_qual(sessions, family):
    """HASHJOIN_FAST_OUTER_QUAL at a tile and one row: the qual is evaluated on the tile's registers
    before the probe; a NULL in its column rejects the row"""
    s = family_session(sessions, family, spec=QUAL_SPEC, ext=QUAL_EXT)
    nrows = FAMILIES[family][3] + 1
    fk, fkn = outer_keys(s, family, nrows, 0.5, True)
    rng = np.random.default_rng(23)
    a = rng.integers(0, 2**31, nrows, dtype=np.int64).astype(np.int32)
    an = rng.random(nrows) < 0.03
    an[1] = an[-2] = True
    b = rng.random(nrows)
    orow, irow = numpy_join(fk, fkn, s.pk, s.pkn)
    keep = ~an[orow] & (a[orow] < 2**30) & (b[orow] > 0.25)
    want = records_of(orow[keep] + 1, irow[keep])
    assert 0 < len(want) < len(orow)
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn), kds.Column("int4", a, an),
                                     kds.Column("float8", b)])
    res = s.check(outer, want)
    assert res.perfmon["num_kern_prep"] == (1 if FAMILIES[family][5] else 0)


@pytest.mark.parametrize("nslots,staged", [(8192, True), (8193, False)])
def test_the_lds_line(sessions, nslots, staged):
    """a slot array of exactly 32 KB is staged in LDS, one slot more is read through the caches"""
    def make():
        rng = np.random.default_rng(nslots)
        pk = (1 + rng.permutation(nslots - 2)[:5000]).astype(np.int32)
        pk[0], pk[1] = 0, nslots - 1
        inner = kds.build_kds("row_flat", [kds.Column("int4", pk), kds.Column("int4", pk)])
        s = Session(C3_SPEC, [inner], [[1]])
        s.pk = pk
        assert s.info[0]["mode"] == "direct" and s.info[0]["unique"] and s.info[0]["nslots"] == nslots
        return s
    s = sessions.get(("lds_line", nslots), make)
    rng = np.random.default_rng(5)
    nrows = T_LDS + 3
    fk = rng.integers(-2, nslots + 2, nrows).astype(np.int32)
    fk[:4] = [0, nslots - 1, nslots, -1]
    fkn = rng.random(nrows) < 0.03
    fkn[:4] = False
    orow, irow = numpy_join(fk, fkn, s.pk, None)
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn)])
    res = s.check(outer, records_of(orow + 1, irow))
    assert res.perfmon["num_kern_prep"] == (1 if staged else 0)


@pytest.mark.parametrize("key_min", [-3000, 2**40])
def test_int8_direct_key_far_keys_do_not_wrap_into_the_table(sessions, key_min):
    """key - key_min is taken in 64 bits and compared unsigned with the slot count: keys at both ends
    of int8 and next to the table must not turn into a slot"""
    nkeys = 6001
    pk = key_min + np.random.default_rng(8).permutation(nkeys).astype(np.int64)        # dense
    s = sessions.get(("int8", key_min), lambda: Session(INT8_SPEC, [kds.build_kds(
        "row_flat", [kds.Column("int8", pk), kds.Column("int4", np.arange(nkeys, dtype=np.int32))])], [[1]]))
    assert s.info[0]["mode"] == "direct" and s.info[0]["unique"] and s.info[0]["nslots"] == nkeys
    rng = np.random.default_rng(9)
    nrows = T_LDS + 1
    fk = key_min + rng.integers(-nkeys, 2 * nkeys, nrows)
    far = [INT64_MIN, INT64_MAX, key_min - 1, key_min + nkeys, key_min, key_min + nkeys - 1,
           key_min + 2**32, key_min - 2**32,            # (equal to a key in the low 32 bits)
           key_min + 2**63 if key_min < 0 else key_min - 2**63]
    fk[:len(far)] = far
    fk[-1] = INT64_MAX
    fkn = rng.random(nrows) < 0.02
    fkn[:len(far)] = False
    fkn[-1] = False
    orow, irow = numpy_join(fk, fkn, pk, None)
    assert 0 < len(orow) < nrows
    outer = kds.build_kds("column", [kds.Column("int8", fk, fkn)])
    s.check(outer, records_of(orow + 1, irow))


# ---------------------------------------------------------------------------------------------
# the general kernel (a row map forces it), one work-group: rows per thread = ceil(rows / 256) <= 64
# ---------------------------------------------------------------------------------------------
GENERAL_KEYS = 300


def general_session(sessions, fanout):
    def make():
        pk = np.repeat(np.arange(GENERAL_KEYS, dtype=np.int32), fanout)
        np.random.default_rng(fanout).shuffle(pk)
        inner = kds.build_kds("row_flat", [kds.Column("int4", pk),
                                           kds.Column("int4", np.arange(len(pk), dtype=np.int32))])
        s = Session(C3_SPEC, [inner], [[1]], ratio=float(fanout))
        s.pk = pk
        assert s.info[0]["unique"] == (fanout == 1)
        return s
    return sessions.get(("general", fanout), make)


def general_case(nfact, fanout):
    """keys of which three in four have partners, a NULL on one row in a hundred; the row map takes
    every row, in reverse"""
    rng = np.random.default_rng(1000 + nfact + fanout)
    fk = rng.integers(0, int(GENERAL_KEYS * 1.3), nfact).astype(np.int32)
    fkn = rng.random(nfact) < 0.01
    # row 0 comes last through the reversed map: at 4097 and 16385 rows it is alone in the second
    # slice and the second tile, so it has partners
    fk[0], fkn[0] = 7, False
    outer = kds.build_kds("column", [kds.Column("int4", fk, fkn), kds.Column("float8", np.zeros(nfact))])
    return fk, fkn, outer, np.arange(nfact, dtype=np.int32)[::-1].copy()


# 257: two rows per thread; 4096: exactly one slice of 16 rows per thread; 4097: 17, a second slice;
# 16384: one tile of 64 rows per thread; 16385: a second tile of one row; 40001: three tiles
GENERAL_ROWS = [1, 255, 256, 257, 4096, 4097, 16383, 16384, 16385, 40001]


def general_check(sessions, fanout, nfact):
    s = general_session(sessions, fanout)
    fk, fkn, outer, row_map = general_case(nfact, fanout)
    orow, irow = numpy_join(fk, fkn, s.pk, None)
    assert len(orow) == int(np.count_nonzero((fk < GENERAL_KEYS) & ~fkn)) * fanout
    s.check(outer, records_of(orow + 1, irow), row_map=row_map)


@pytest.mark.parametrize("nfact", GENERAL_ROWS)
@pytest.mark.parametrize("fanout", [1, 40])
def test_general_kernel_slices_and_tiles(sessions, fanout, nfact, monkeypatch):
    """fan-out 1 is staged (a slice of 4096 rows has at most 4096 records), fan-out 40 takes the direct
    path from 257 rows on; the emit base moves on by every slice's total, in the second to fourth slice
    and the second and third tile; single_mask / emit_mask bits up to 63"""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    general_check(sessions, fanout, nfact)


@pytest.mark.parametrize("nfact", [4097, 16385, 40001])
@pytest.mark.parametrize("fanout", [1, 40])
def test_general_kernel_without_the_first_match_scratch(sessions, fanout, nfact, monkeypatch):
    """first_buf == NULL, the path a failed or oversized scratch allocation takes: the emit pass
    probes again, also for rows with one match -- the same records, with a second slice, a second
    tile and three tiles"""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    monkeypatch.setenv("STROM_HASHJOIN_NO_FIRST_MATCH", "1")
    general_check(sessions, fanout, nfact)


@pytest.mark.parametrize("doubled", [False, True])
def test_general_kernel_stage_capacity_at_equality_and_one_above(sessions, doubled, monkeypatch):
    """two relations in a record: the stage takes 32768 / 4 / 2 = 4096 records.  4096 rows that all
    match unique keys make the one slice's total exactly that (staged); with one inner key doubled
    and met once the total is 4097 (direct)"""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    nfact = 4096

    def make():
        pk = np.random.default_rng(77).permutation(5000).astype(np.int32)
        if doubled:
            pk[-1] = pk[0]
        inner = kds.build_kds("row_flat", [kds.Column("int4", pk), kds.Column("int4", pk)])
        s = Session(C3_SPEC, [inner], [[1]], ratio=1.1)
        s.pk = pk
        assert s.info[0]["mode"] == "direct" and s.info[0]["unique"] == (not doubled)
        return s
    s = sessions.get(("stage_cap", doubled), make)
    fk = s.pk[:nfact].copy()                    # distinct keys, the doubled one (pk[0]) once
    outer = kds.build_kds("column", [kds.Column("int4", fk)])
    orow, irow = numpy_join(fk, None, s.pk, None)
    assert len(orow) == nfact + (1 if doubled else 0)
    s.check(outer, records_of(orow + 1, irow), row_map=np.arange(nfact, dtype=np.int32)[::-1].copy())


@pytest.mark.parametrize("room", ["one_short", "half"])
@pytest.mark.parametrize("fanout", [1, 40])
def test_general_kernel_goes_on_counting_without_room(sessions, fanout, room, monkeypatch):
    """40001 rows are three tiles of one work-group: one record short fails the last tile's
    reservation, half the room the second tile's, after which the third goes on counting -- nitems is
    the full count either way"""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = general_session(sessions, fanout)
    fk, fkn, outer, row_map = general_case(40001, fanout)
    orow, irow = numpy_join(fk, fkn, s.pk, None)
    res = s.run(outer, nrooms=len(orow) - 1 if room == "one_short" else len(orow) // 2, row_map=row_map)
    assert res.errcode == ERR_NOSPACE and res.nitems == len(orow)


def test_general_kernel_two_relations_across_a_tile_boundary(sessions, monkeypatch):
    """three words per record: the stage takes 8192 / 3 = 2730 records.  16385 rows are a tile of four
    4096-row slices and a tile of one row; the first half of the chunk has partners for most rows
    (slices beyond the stage: direct), the second half for few (staged)"""
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    rng = np.random.default_rng(31)
    n1, n2, nf = 3000, 500, 16385
    a = rng.integers(0, 60, n1).astype(np.int32)
    b = rng.integers(0, 5, n1).astype(np.int64)
    c = rng.random(n1)
    link = rng.integers(0, 700, n1).astype(np.int32)
    linkn = rng.random(n1) < 0.05
    pk2 = rng.permutation(700)[:n2].astype(np.int32)
    v2 = rng.integers(0, 9, n2).astype(np.int16)
    fa = np.where(np.arange(nf) < nf // 2, rng.integers(0, 70, nf), rng.integers(0, 700, nf)).astype(np.int32)
    fan = rng.random(nf) < 0.02
    fb = rng.integers(0, 6, nf).astype(np.int16)
    fc = rng.random(nf)

    def make():
        t1 = kds.build_kds("row", [kds.Column("int4", a), kds.Column("int8", b), kds.Column("float8", c),
                                   kds.Column("int4", link, linkn)])
        t2 = kds.build_kds("row_flat", [kds.Column("int4", pk2), kds.Column("int2", v2)])
        return Session(TWO_REL_SPEC, [t1, t2], [[1, 2], [1]], ext=[np.int16(6)], ratio=30.0)
    s = sessions.get("two_rel", make)
    outer = kds.build_kds("column", [kds.Column("int4", fa, fan), kds.Column("int2", fb), kds.Column("float8", fc)])
    # the numpy model: both keys of the first relation as one number, then its qual; the second
    # relation on the first one's link column, then its qual
    o1, i1 = numpy_join(fa.astype(np.int64) * 16 + fb, fan, a.astype(np.int64) * 16 + b, None)
    keep = c[i1] > fc[o1]
    o1, i1 = o1[keep], i1[keep]
    j, i2 = numpy_join(link[i1], linkn[i1], pk2, None)
    keep = v2[i2] < 6
    j, i2 = j[keep], i2[keep]
    want = records_of(o1[j] + 1, i1[j], i2)
    per_slice = np.bincount((nf - 1 - o1[j]) // 4096, minlength=5)     # (row map: every row, reversed)
    assert per_slice[:4].max() > 2730 and 0 < per_slice[:4].min() <= 2730
    row_map = np.arange(nf, dtype=np.int32)[::-1].copy()
    s.check(outer, want, row_map=row_map)
    rc, n, recs = oracle.gpuhashjoin(TWO_REL_SPEC, outer, s.inners, [np.int16(6)], row_map=row_map)
    assert rc == 0 and np.array_equal(sorted_records(recs), sorted_records(want))


def test_numpy_model_and_oracle_agree_on_the_general_kernel(sessions, monkeypatch):
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = general_session(sessions, 40)
    fk, fkn, outer, row_map = general_case(4097, 40)
    orow, irow = numpy_join(fk, fkn, s.pk, None)
    rc, n, recs = oracle.gpuhashjoin(C3_SPEC, outer, s.inners, row_map=row_map)
    assert rc == 0 and np.array_equal(sorted_records(recs), sorted_records(records_of(orow + 1, irow)))


# ---------------------------------------------------------------------------------------------
# geometry: a program of its own per setting (the knobs are -D options and part of the program's key)
# ---------------------------------------------------------------------------------------------
def geometry_session(family):
    pk, pkn = family_keys(family)
    inner = kds.build_kds("row_flat", [kds.Column("int4", pk, pkn),
                                       kds.Column("int4", np.arange(len(pk), dtype=np.int32))])
    s = Session(C3_SPEC, [inner], [[1]])
    s.pk, s.pkn = pk, pkn
    return s


@pytest.mark.parametrize("family", ["fast", "fast_narrow"])
def test_geometry_one_quad_tiles_fill_the_stage_exactly(family, monkeypatch):
    """HASHJOIN_FAST_QUADS=1: 1024-row tiles, four of which fill the 4096-record stage when every
    row matches: the flush at fill == HASHJOIN_STAGE_ENTRIES, in one work-group over nine tiles and
    a ragged tenth"""
    monkeypatch.setenv("STROM_HASHJOIN_FAST_QUADS", "1")
    monkeypatch.setenv("STROM_HASHJOIN_MAX_GRID", "1")
    s = geometry_session(family)
    try:
        assert s.info[0]["mode"] == "direct" and s.info[0]["unique"]
        probe_family(s, family, 9 * 1024 + 5, 1.0, False)
    finally:
        s.end()


def test_geometry_fewer_lds_quads_than_fast_quads(monkeypatch):
    """HASHJOIN_LDS_QUADS=2 used to size the stage's wave totals for two quads, which the _fast
    kernel indexes with four: HASHJOIN_MAX_QUADS covers every kernel's quads now"""
    monkeypatch.setenv("STROM_HASHJOIN_LDS_QUADS", "2")
    s = geometry_session("fast")
    try:
        probe_family(s, "fast", 2 * T_FAST + 3, 0.5, True)
    finally:
        s.end()


def test_geometry_the_header_cannot_serve_is_a_build_error(monkeypatch):
    """HASHJOIN_FAST_QUADS=16 is beyond what strom_hashjoin.h takes (static_assert): the program does
    not build, so begin() fails and nothing is launched"""
    monkeypatch.setenv("STROM_HASHJOIN_FAST_QUADS", "16")
    with pytest.raises(runtime.StromError) as ei:
        geometry_session("fast").end()
    assert ei.value.errcode == ERR_BUILD
    assert "HASHJOIN_FAST_QUADS" in str(ei.value)
