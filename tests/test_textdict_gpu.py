"""
GROUP BY text / character(n) through the key dictionary (needs an MI355X: -m gpu).

Expected values come from Python alone: per row the key is the payload for text and
payload.rstrip(b" ") for character(n).  An encoding is right when keys()[id[row]] is the row's
key, ids are equal iff keys are equal, ids lie in [0, num_keys), num_keys is the number of
distinct non-NULL keys and a NULL row is NULL.  The oracle has no text-key GROUP BY; the
end-to-end cases are checked against a Python dict.
"""
import ctypes

import numpy as np
import pytest

import text_cases
from pg_strom_amd import kds, runtime, textdict
from pg_strom_amd._lib import lib
from pg_strom_amd.gpupreagg import GpuPreAgg
from pg_strom_amd.gpuscan import GpuScan
from pg_strom_amd.textdict import TextDictionary, group_by_text

pytestmark = pytest.mark.gpu

W = text_cases.WORDS
BLOCK = 256                      # TEXTDICT_BLOCK's default
CPU_RECHECK, BAD_REQUEST, CORRUPTION = 2, 101, 300


@pytest.fixture(autouse=True)
def _runtime():
    runtime.init()


def row_key(payload, kind):
    return payload.rstrip(b" ") if kind == "character" else payload


def upload_keys(kind, payloads, isnull=None, extra=()):
    buf = kds.build_kds("column", [kds.Column(kind, payloads, isnull)] + list(extra))
    return runtime.DeviceStore.upload(buf), buf


def decode_ids(enc, col=0):
    c = kds.decode_column_chunk(enc.download())[col]
    ids = c["values"].astype(np.int64)
    notnull = c["notnull"] if c["notnull"] is not None else np.ones(len(ids), dtype=bool)
    return ids, notnull, c


def check_encoding(d, enc, kind, payloads, isnull=None, col=0, known=None):
    """every property of the module docstring; 'known': key -> id of earlier calls, updated"""
    n = len(payloads)
    ids, notnull, c = decode_ids(enc, col)
    isnull = np.zeros(n, dtype=bool) if isnull is None else np.asarray(isnull, dtype=bool)
    keys = d.keys()
    nk = d.num_keys
    assert len(keys) == nk and len(ids) == n
    assert np.array_equal(notnull, ~isnull)
    by_key = {} if known is None else known
    for i in range(n):
        if isnull[i]:
            continue
        want = row_key(payloads[i], kind)
        assert 0 <= ids[i] < nk, (i, ids[i], nk)
        assert keys[ids[i]] == want, (i, ids[i])
        assert by_key.setdefault(want, int(ids[i])) == ids[i], (i, want)
    assert len(set(by_key.values())) == len(by_key) == nk        # equal ids <=> equal keys; no id unused
    if nk and not isnull.all():
        assert c["stat_flags"] & 1 and (c["minval"], c["maxval"]) == (0, nk - 1)
    return ids, by_key


# ---- 1. sizes that cross a wave, a block and a grid stride ------------------------------------
@pytest.mark.parametrize("kind", ["text", "character"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK + 1, 2 * (2 * BLOCK) + 3])
def test_sizes_across_wave_block_and_grid_stride(kind, n, monkeypatch):
    monkeypatch.setenv("STROM_TEXTDICT_MAX_GRID", "2")           # two work-groups: the last size strides
    rng = np.random.default_rng(n)
    order = rng.permutation(len(W))
    payloads = [W[order[i % len(W)]] for i in range(n)]
    isnull = (np.arange(n) % 11 == 5)
    src, _ = upload_keys(kind, payloads, isnull)
    d = TextDictionary(kind)
    try:
        enc = d.encode(src, [0])
        _, by_key = check_encoding(d, enc, kind, payloads, isnull)
        enc.release()
        if n >= 64:
            # 'hello', 'hello ' and 'hello  ': three text keys, one character key
            hello = {by_key[row_key(w, kind)] for w in (b"hello", b"hello ", b"hello  ")}
            assert len(hello) == (3 if kind == "text" else 1)
            assert d.num_keys == len({row_key(w, kind) for w in W})
    finally:
        d.release()
        src.release()


# ---- 2. every lane at one slot; growth inside one call ------------------------------------------
def test_one_key_in_4096_rows():
    payloads = [b"the same key"] * 4096
    src, _ = upload_keys("text", payloads)
    d = TextDictionary("text")
    try:
        enc = d.encode(src, [0])
        ids, _ = check_encoding(d, enc, "text", payloads)
        assert d.num_keys == 1 and not ids.any()
        enc.release()
    finally:
        d.release()
        src.release()


def test_all_distinct_3000_rows_from_a_hint_of_4():
    payloads = [(b"key-%05d" % i) * (1 + i % 23) for i in range(3000)]      # 1- and 4-byte headers
    src, _ = upload_keys("text", payloads)
    d = TextDictionary("text", nkeys_hint=4)
    try:
        enc = d.encode(src, [0])
        ids, _ = check_encoding(d, enc, "text", payloads)
        assert d.num_keys == 3000 and np.array_equal(np.sort(ids), np.arange(3000))
        enc.release()
    finally:
        d.release()
        src.release()


# ---- 3. tags and home slots collide: byte compare and probe walk decide ---------------------------
def test_four_bit_hashes(monkeypatch):
    monkeypatch.setenv("STROM_TEXTDICT_HASH_BITS", "4")
    rng = np.random.default_rng(4)
    distinct = [b"%08d" % (7919 * i) for i in range(500)]
    pick = np.concatenate([np.arange(500), rng.integers(0, 500, 1500)])
    rng.shuffle(pick)
    payloads = [distinct[i] for i in pick]
    src, _ = upload_keys("text", payloads)
    d = TextDictionary("text")
    plain = TextDictionary("text")
    try:
        enc = d.encode(src, [0])
        # the program that ran is the one whose text cuts the hash to four bits, not the default
        source = textdict.program_source()
        assert source.startswith("#define TEXTDICT_HASH_BITS 4\n")
        prog = runtime.DevProgram(source, 0)
        assert d.program_key() == prog.key
        assert lib.strom_get_devprog_source(prog.key).decode() == source
        prog.release()
        monkeypatch.delenv("STROM_TEXTDICT_HASH_BITS")
        plain.encode(src, [0]).release()
        assert plain.program_key() not in (0, d.program_key())
        monkeypatch.setenv("STROM_TEXTDICT_HASH_BITS", "4")
        check_encoding(d, enc, "text", payloads)
        assert d.num_keys == 500
        enc.release()
        enc = d.encode(src, [0])                                 # steady state over the same chains
        check_encoding(d, enc, "text", payloads)
        assert d.num_keys == 500
        enc.release()
    finally:
        d.release()
        plain.release()
        src.release()


# ---- 4. across calls ------------------------------------------------------------------------------
def test_ids_across_calls_reset_and_a_failed_call():
    one = [W[i % 10] for i in range(700)]
    two = [W[5 + i % 15] for i in range(900)]                    # W[5..9] known, W[10..19] new
    src1, _ = upload_keys("text", one)
    src2, _ = upload_keys("text", two)
    plain = kds.varlena_datum(b"abc")
    compressed = np.array([(20 << 2) | 2], dtype="<u4").tobytes() + b"\0" * 16
    external = bytes([0x01, 18]) + b"\0" * 16
    bad = runtime.DeviceStore.upload(kds.build_kds(
        "column", [kds.Column("text_raw", [plain, compressed, external, kds.varlena_datum(b"new key")] * 100)]))
    d = TextDictionary("text")
    try:
        enc = d.encode(src1, [0])
        ids1, known = check_encoding(d, enc, "text", one)
        enc.release()
        assert d.num_keys == 10
        enc = d.encode(src2, [0])
        _, known = check_encoding(d, enc, "text", two, known=known)          # old keys keep their ids
        enc.release()
        assert d.num_keys == 20
        assert sorted(known[w] for w in W[10:20]) == list(range(10, 20))     # new ones from num_keys on
        # a chunk with a compressed and an external datum is the CPU's; nothing of it stays
        with pytest.raises(runtime.StromError) as ei:
            d.encode(bad, [0])
        assert ei.value.errcode == CPU_RECHECK
        assert d.num_keys == 20
        enc = d.encode(src1, [0])
        again, _ = check_encoding(d, enc, "text", one, known=known)
        enc.release()
        assert np.array_equal(again, ids1) and d.num_keys == 20
        d.reset()
        assert d.num_keys == 0 and d.keys() == []
        enc = d.encode(src2, [0])
        check_encoding(d, enc, "text", two)
        enc.release()
        assert d.num_keys == 15
    finally:
        d.release()
        for s in (src1, src2, bad):
            s.release()


# ---- 5. errors and refusals -------------------------------------------------------------------------
def test_an_offset_beyond_the_chunk_is_corruption():
    payloads = [W[i % len(W)] for i in range(500)]
    buf = kds.build_kds("column", [kds.Column("text", payloads)])
    voff = int(np.frombuffer(buf[64:68].tobytes(), dtype="<u4")[0])          # coldir[0].values_off
    offs = buf[voff:voff + 8 * 500].view(np.uint64)
    offs[321] = len(buf) + 4096
    src = runtime.DeviceStore.upload(buf)
    d = TextDictionary("text")
    try:
        with pytest.raises(runtime.StromError) as ei:
            d.encode(src, [0])
        assert ei.value.errcode == CORRUPTION
        assert d.num_keys == 0
    finally:
        d.release()
        src.release()


def test_bad_requests_are_refused_before_any_launch():
    n = 300
    txt = [W[i % len(W)] for i in range(n)]
    cols = [kds.Column("text", txt), kds.Column("int4", np.arange(n, dtype=np.int32))]
    column = runtime.DeviceStore.upload(kds.build_kds("column", cols))
    rows = runtime.DeviceStore.upload(kds.build_kds("row", cols))
    d = TextDictionary("text")

    def refused(dicts, key_cols, store, carry):
        handles = (ctypes.c_void_p * 9)(*[h for h in dicts] + [None] * (9 - len(dicts)))
        keys = (ctypes.c_int32 * 9)(*(list(key_cols) + [0] * (9 - len(key_cols))))
        carr = (ctypes.c_int32 * 4)(*(list(carry) + [0] * (4 - len(carry))))
        err = ctypes.c_int(0)
        h = lib.strom_textdict_encode(handles, keys, len(key_cols), store, carr, len(carry), ctypes.byref(err))
        assert not h
        return err.value

    try:
        assert refused([None], [0], column.handle, []) == BAD_REQUEST            # NULL handle
        assert refused([d.handle], [0], rows.handle, []) == BAD_REQUEST          # not a COLUMN chunk
        assert refused([d.handle], [0], None, []) == BAD_REQUEST                 # not resident
        assert refused([d.handle], [1], column.handle, []) == BAD_REQUEST        # key column by value
        assert refused([d.handle], [0], column.handle, [0]) == BAD_REQUEST       # varlena carry column
        assert refused([d.handle], [2], column.handle, []) == BAD_REQUEST        # no such column
        assert refused([], [], column.handle, []) == BAD_REQUEST                 # no key
        assert refused([d.handle] * 9, [0] * 9, column.handle, []) == BAD_REQUEST
        assert d.num_keys == 0
        enc = d.encode(column, [0], [1])                                         # and the good one
        check_encoding(d, enc, "text", txt)
        enc.release()
    finally:
        d.release()
        column.release()
        rows.release()


# ---- 6. the encoded chunk ---------------------------------------------------------------------------
def test_carried_columns_come_back_bit_equal():
    n = 1237
    rng = np.random.default_rng(6)
    txt = [W[i] for i in rng.integers(0, len(W), n)]
    a = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    b = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    f = rng.standard_normal(n)
    an, fn = rng.random(n) < 0.1, rng.random(n) < 0.2
    cols = [kds.Column("int4", a, an), kds.Column("text", txt, np.arange(n) % 7 == 0),
            kds.Column("int8", b), kds.Column("float8", f, fn)]
    buf = kds.build_kds("column", cols)
    src = runtime.DeviceStore.upload(buf)
    d = TextDictionary("text")
    try:
        enc = d.encode(src, [1], [3, 0, 2])
        check_encoding(d, enc, "text", txt, np.arange(n) % 7 == 0)
        got = kds.decode_column_chunk(enc.download())
        want = kds.decode_column_chunk(buf)
        head = kds.KdsHead(enc.download())
        assert head.ncols == 4 and head.nitems == n and list(head.colmeta["attlen"]) == [4, 8, 4, 8]
        for g, w in zip(got[1:], [want[3], want[0], want[2]]):
            assert np.array_equal(g["values"], w["values"])
            assert (g["notnull"] is None) == (w["notnull"] is None)
            if w["notnull"] is not None:
                assert np.array_equal(g["notnull"], w["notnull"])
            assert (g["stat_flags"], g["minval"], g["maxval"]) == (w["stat_flags"], w["minval"], w["maxval"])
        assert got[0]["stat_flags"] == 1 and (got[0]["minval"], got[0]["maxval"]) == (0, d.num_keys - 1)
        enc.release()
    finally:
        d.release()
        src.release()


# ---- 7. GROUP BY end to end ---------------------------------------------------------------------------
N = 4001
SPEC1 = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)) (pmin (var 3 int4)))"
SPEC2 = "(gpupreagg (key (var 1 int4)) (key (var 2 int4)) (nrows) (psum (var 3 int8)) (pmin (var 4 int4)))"
TYPES = ("text", "character", "int4", "int8", "int4")


@pytest.fixture(scope="module")
def table():
    """one table for all end-to-end cases: (text t, character(12) c, int4 g, int8 v, int4 x)"""
    rng = np.random.default_rng(70)
    pool = W + [(b"k%04d" % i) * (1 + i % 30) for i in range(150)]
    t = [pool[i] for i in rng.integers(0, len(pool), N)]
    c = [(W[i][:12] + b" " * 12)[:12] for i in rng.integers(0, len(W), N)]
    tnull = rng.random(N) < 0.05
    g = rng.integers(-3, 4, N).astype(np.int32)
    v = rng.integers(-10**12, 10**12, N)
    x = rng.integers(-1000, 1000, N).astype(np.int32)
    return dict(t=t, c=c, tnull=tnull, g=g, v=v, x=x)


def build_chunk(tb, lo, hi, fmt="column"):
    return kds.build_kds(fmt, [kds.Column("text", tb["t"][lo:hi], tb["tnull"][lo:hi]),
                               kds.Column("character", tb["c"][lo:hi]),
                               kds.Column("int4", tb["g"][lo:hi]), kds.Column("int8", tb["v"][lo:hi]),
                               kds.Column("int4", tb["x"][lo:hi])])


def expected_groups(tb, key_fn, rows=None):
    want = {}
    for i in (range(N) if rows is None else rows):
        k = key_fn(i)
        cnt, sm, mn = want.get(k, (0, 0, None))
        want[k] = (cnt + 1, sm + int(tb["v"][i]), int(tb["x"][i]) if mn is None else min(mn, int(tb["x"][i])))
    return want


def groups_of(pr, keycols, nkeys):
    """partial rows -> {key or key tuple: (count, sum, min)}; key column i of keycols replaces id column i"""
    cnt, sm, mn = (pr.column(nkeys + j)[0] for j in range(3))
    got = {}
    for r in range(len(pr)):
        key = []
        for k in range(nkeys):
            if k < len(keycols):
                key.append(keycols[k][r])
            else:
                val, nul = pr.column(k)
                key.append(None if nul[r] else int(val[r]))
        key = key[0] if nkeys == 1 else tuple(key)
        assert key not in got
        got[key] = (int(cnt[r]), int(sm[r]), int(mn[r]))
    return got


def text_key(tb):
    return lambda i: None if tb["tnull"][i] else tb["t"][i]


@pytest.mark.parametrize("hashed", [False, True])
def test_group_by_text_key_with_a_null_group(table, hashed):
    src = runtime.DeviceStore.upload(build_chunk(table, 0, N))
    try:
        pr, keycols = group_by_text([src], [(0, "text")], SPEC1, [3, 4], hashed=hashed)
        want = expected_groups(table, text_key(table))
        assert None in want                                          # the NULL key group is there
        assert groups_of(pr, keycols, 1) == want
    finally:
        src.release()


def test_group_by_character_key(table):
    src = runtime.DeviceStore.upload(build_chunk(table, 0, N))
    try:
        pr, keycols = group_by_text([src], [(1, "character")], SPEC1, [3, 4])
        assert groups_of(pr, keycols, 1) == expected_groups(table, lambda i: table["c"][i].rstrip(b" "))
    finally:
        src.release()


def test_group_by_text_and_int4(table):
    src = runtime.DeviceStore.upload(build_chunk(table, 0, N))
    try:
        pr, keycols = group_by_text([src], [(0, "text")], SPEC2, [2, 3, 4], int_keys=[1])
        tk = text_key(table)
        assert groups_of(pr, keycols, 2) == expected_groups(table, lambda i: (tk(i), int(table["g"][i])))
    finally:
        src.release()


def test_group_by_two_text_keys_with_two_dictionaries(table):
    src = runtime.DeviceStore.upload(build_chunk(table, 0, N))
    try:
        pr, keycols = group_by_text([src], [(0, "text"), (1, "character")], SPEC2, [3, 4])
        tk = text_key(table)
        assert groups_of(pr, keycols, 2) == expected_groups(
            table, lambda i: (tk(i), table["c"][i].rstrip(b" ")))
    finally:
        src.release()


def test_group_by_over_three_chunks_transposed_on_the_device(table):
    """the source arrives as ROW_FLAT heap tuples and is transposed by strom_dstore_to_column"""
    bounds = [(0, 1500), (1500, 1501), (1501, N)]
    oids = [kds.column_type_oid(t) for t in TYPES]
    rows, cols = [], []
    try:
        for lo, hi in bounds:
            rows.append(runtime.DeviceStore.upload(build_chunk(table, lo, hi, "row_flat")))
            cols.append(rows[-1].to_column(oids)[0])
        pr, keycols = group_by_text(cols, [(0, "text")], SPEC1, [3, 4])
        assert groups_of(pr, keycols, 1) == expected_groups(table, text_key(table))
    finally:
        for s in rows + cols:
            s.release()


def test_group_by_behind_the_row_map_of_a_text_qual(table):
    """WHERE t >= 'b' is evaluated where text lives -- a GpuScan over the source chunk -- and its
    device row map applies unchanged to the encoded chunk"""
    src = runtime.DeviceStore.upload(build_chunk(table, 0, N))
    scan = GpuScan("(text_ge (var 1 text) (const text 'b'))").begin()
    rm = None
    try:
        rm, res = scan.scan_to_rowmap(src)
        keep = [i for i in range(N) if not table["tnull"][i] and table["t"][i] >= b"b"]
        assert res.nitems == len(keep) > 0
        pr, keycols = group_by_text([src], [(0, "text")], SPEC1, [3, 4], row_maps=[rm])
        assert groups_of(pr, keycols, 1) == expected_groups(table, text_key(table), keep)
    finally:
        if rm is not None:
            rm.release()
        scan.end()
        src.release()


def test_an_encoded_chunk_through_the_chunk_message(table):
    """strom_submit_gpupreagg_chunk takes an encoded chunk as it is"""
    src = runtime.DeviceStore.upload(build_chunk(table, 0, N))
    d = TextDictionary("text")
    enc = None
    try:
        enc = d.encode(src, [0], [3, 4])
        agg = GpuPreAgg(SPEC1)
        status, pr = agg.collect_chunk(agg.submit_chunk(enc))
        agg.end()
        assert status == 0
        assert groups_of(pr, textdict.ids_to_keys(pr, [d]), 1) == expected_groups(table, text_key(table))
    finally:
        if enc is not None:
            enc.release()
        d.release()
        src.release()
