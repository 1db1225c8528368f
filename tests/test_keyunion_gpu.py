"""
The union of key dictionaries (strom_keyunion_*, strom_keymap_*) and GROUP BY text over shards
(needs an MI355X: -m gpu).

The id rule is Python's own:  for k in image: ids.setdefault(k, len(ids))  with 'ids' starting as
the keys the absorbing dictionary holds (the key of a datum: its payload for text, its payload
without trailing blanks for character(n)).  A map is right when it EQUALS that model element for
element -- not merely when it is consistent -- because ranks that never talk to each other again
rely on getting the same numbers.  The end-to-end cases are checked against a Python dict over all
rows and against group_by_text over the same chunks under one dictionary.
"""
import ctypes

import numpy as np
import pytest

import text_cases
from pg_strom_amd import kds, runtime, textdict
from pg_strom_amd._lib import lib
from pg_strom_amd.textdict import TextDictionary, group_by_text, group_by_text_sharded, recode, unify

pytestmark = pytest.mark.gpu

W = text_cases.WORDS
BLOCK = 256                      # TEXTDICT_BLOCK's default
BAD_REQUEST, CORRUPTION = 101, 300


@pytest.fixture(autouse=True)
def _runtime():
    runtime.init()


def row_key(payload, kind):
    return payload.rstrip(b" ") if kind == "character" else payload


def image_of(payloads):
    """a key image as strom_textdict_fetch lays it out: complete datums, each on a 4-byte boundary"""
    heap, offs = b"", []
    for p in payloads:
        offs.append(len(heap))
        d = kds.varlena_datum(p)
        heap += d + b"\0" * (-len(d) % 4)
    return heap, np.array(offs, dtype=np.uint64)


def model_absorb(ids, payloads, kind):
    """the contract: ids {key: id} is updated, the map is returned"""
    return [ids.setdefault(row_key(p, kind), len(ids)) for p in payloads]


def ids_of(d):
    return {k: i for i, k in enumerate(d.keys())}


def upload_keys(kind, payloads, isnull=None, extra=()):
    return runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column(kind, payloads, isnull)] + list(extra)))


def absorb_and_check(d, payloads, kind, ids):
    """absorb the image of 'payloads' into d; the map, keys() and num_keys are the model's"""
    want = model_absorb(ids, payloads, kind)
    m = d.absorb(image_of(payloads))
    try:
        assert len(m) == len(payloads)
        assert m.ids().tolist() == want
    finally:
        m.release()
    assert d.keys() == list(ids) and d.num_keys == len(ids)


# ---- 1. ordered ids; sizes that cross a wave, a block (= a tile of the ranks) and a grid stride ------
@pytest.mark.parametrize("start", ["empty", "half"])
@pytest.mark.parametrize("kind", ["text", "character"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK + 1, 2 * (2 * BLOCK) + 3])
def test_ids_in_image_order(kind, n, start, monkeypatch):
    monkeypatch.setenv("STROM_TEXTDICT_MAX_GRID", "2")
    rng = np.random.default_rng(1000 + n)
    order = rng.permutation(len(W))
    payloads = [W[order[i % len(W)]] for i in range(n)]
    d = TextDictionary(kind)
    src = None
    try:
        if start == "half":
            half = [W[i] for i in rng.permutation(len(W))[:len(W) // 2]]
            src = upload_keys(kind, half * 3)
            d.encode(src, [0]).release()
            assert d.num_keys == len({row_key(w, kind) for w in half})
        ids = ids_of(d)                                          # an encode's ids are what they are
        absorb_and_check(d, payloads, kind, ids)
        if n >= 64:
            hello = {ids[row_key(w, kind)] for w in (b"hello", b"hello ", b"hello  ")}
            assert len(hello) == (3 if kind == "text" else 1)
            assert d.num_keys == len({row_key(w, kind) for w in W})
        # absorbing the same image again changes nothing and maps to the same ids
        absorb_and_check(d, payloads, kind, ids)
    finally:
        d.release()
        if src is not None:
            src.release()


# ---- 2. every lane at a few slots: the timing of the claims decides nothing ---------------------------
def test_contention_decides_nothing(monkeypatch):
    monkeypatch.setenv("STROM_TEXTDICT_HASH_BITS", "4")
    pattern = [b"b", b"a", b"b", b"c", b"a"]
    payloads = [pattern[i % 5] for i in range(4096)]
    d = TextDictionary("text")
    try:
        ids = {}
        absorb_and_check(d, payloads, "text", ids)
        assert ids == {b"b": 0, b"a": 1, b"c": 2}
        prog = runtime.DevProgram(textdict.program_source(), 0)  # the program with 4-bit hashes ran
        assert textdict.program_source().startswith("#define TEXTDICT_HASH_BITS 4\n") and d.program_key() == prog.key
        prog.release()
        # 300 distinct keys under 16 hash values, 1- and 4-byte headers mixed, some already known
        more = [(b"key-%05d" % (7919 * i)) * (1 + (i % 3) * 8) for i in range(300)]
        assert any(len(p) > 126 for p in more) and any(len(p) < 126 for p in more)
        absorb_and_check(d, more[:7] + [b"a", b"c"] + more[7:] + more[:50], "text", ids)
        assert d.num_keys == 303
    finally:
        d.release()


# ---- 3. growth inside one absorb -------------------------------------------------------------------
def test_3000_distinct_keys_into_a_hint_of_4():
    payloads = [(b"key-%05d" % i) * (1 + i % 23) for i in range(3000)]
    d = TextDictionary("text", nkeys_hint=4)
    try:
        m = d.absorb(image_of(payloads))
        assert np.array_equal(m.ids(), np.arange(3000))
        m.release()
        assert d.num_keys == 3000 and d.keys() == payloads
    finally:
        d.release()


# ---- 4. a dictionary absorbed where it lies ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["text", "character"])
def test_absorb_dict_equals_absorb_of_its_image(kind):
    rng = np.random.default_rng(44)
    payloads = [W[i] for i in rng.integers(0, len(W), 700)] + [b"only here %d" % i for i in range(40)]
    chunk = upload_keys(kind, payloads)
    seed = image_of([b"abc", b"only here 7", b"~", b"abc "])    # both unions hold some of the keys already
    src, empty = TextDictionary(kind), TextDictionary(kind)
    g1, g2 = TextDictionary(kind), TextDictionary(kind)
    maps = []
    try:
        src.encode(chunk, [0]).release()
        for g in (g1, g2):
            g.absorb(seed).release()
        heap, offs = src.image()
        assert len(offs) == src.num_keys
        maps = [g1.absorb_dict(src), g2.absorb((heap, offs)), g1.absorb_dict(empty), g2.absorb(empty.image())]
        assert len(maps[0]) == src.num_keys
        assert np.array_equal(maps[0].ids(), maps[1].ids())
        assert g1.keys() == g2.keys() and g1.num_keys == g2.num_keys
        assert [g1.keys()[i] for i in maps[0].ids()] == src.keys()
        assert len(maps[2]) == 0 and len(maps[3]) == 0 and len(maps[2].ids()) == 0
    finally:
        for m in maps:
            m.release()
        for x in (src, empty, g1, g2, chunk):
            x.release()


# ---- 5. a failed absorb changes nothing -----------------------------------------------------------
def test_a_failed_absorb_changes_nothing():
    from test_textdict_gpu import check_encoding
    one = [W[i % 10] for i in range(700)]
    src = upload_keys("text", one)
    d = TextDictionary("text")
    try:
        enc = d.encode(src, [0])
        _, known = check_encoding(d, enc, "text", one)
        enc.release()
        before = d.keys()
        good = [b"new key %d" % i for i in range(100)]
        heap, offs = image_of(good)
        beyond = offs.copy()
        beyond[57] = len(heap) + 4096
        external = heap + bytes([0x01, 18]) + b"\0" * 18
        with_external = np.concatenate([offs, np.array([len(heap)], dtype=np.uint64)])
        short = offs.copy()
        short[99] = len(heap) - 2                                 # inside the heap, but the length found there runs past its end
        for image in ((heap, beyond), (external, with_external), (heap, short)):
            with pytest.raises(runtime.StromError) as ei:
                d.absorb(image)
            assert ei.value.errcode == CORRUPTION
            assert d.num_keys == 10 and d.keys() == before
        enc = d.encode(src, [0])
        check_encoding(d, enc, "text", one, known=known)
        enc.release()
        # ... and the good image is taken afterwards
        ids = ids_of(d)
        absorb_and_check(d, good, "text", ids)
        assert d.num_keys == 110
    finally:
        d.release()
        src.release()


# ---- 6. recode ---------------------------------------------------------------------------------
def decode(enc):
    return kds.decode_column_chunk(enc.download())


def same_column(g, w):
    assert np.array_equal(g["values"], w["values"])
    assert (g["notnull"] is None) == (w["notnull"] is None)
    if w["notnull"] is not None:
        assert np.array_equal(g["notnull"], w["notnull"])
    assert (g["stat_flags"], g["minval"], g["maxval"]) == (w["stat_flags"], w["minval"], w["maxval"])


@pytest.mark.parametrize("kind", ["text", "character"])
@pytest.mark.parametrize("n", [1, 63, 65, 4 * BLOCK + 3])
def test_recode_into_the_union(kind, n, monkeypatch):
    monkeypatch.setenv("STROM_TEXTDICT_MAX_GRID", "2")
    rng = np.random.default_rng(600 + n)
    parts = []
    for lo, hi in ((0, 18), (9, len(W))):                        # the two dictionaries overlap in W[9:18]
        txt = [W[i] for i in rng.integers(lo, hi, n)]
        isnull = (np.arange(n) % 5 == 2)
        a = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        f = rng.standard_normal(n)
        fnull = rng.random(n) < 0.2
        chunk = upload_keys(kind, txt, isnull, [kds.Column("int4", a), kds.Column("float8", f, fnull)])
        parts.append((txt, isnull, chunk))
    dicts = [TextDictionary(kind), TextDictionary(kind)]
    encs, maps, g = [], [], None
    try:
        for d, (_, _, chunk) in zip(dicts, parts):
            encs.append(d.encode(chunk, [0], [1, 2]))
        before = [decode(e) for e in encs]
        g, maps = unify(dicts)
        model = {}
        for d, m in zip(dicts, maps):
            assert m.ids().tolist() == [model.setdefault(k, len(model)) for k in d.keys()]
        assert g.keys() == list(model)
        for e, m in zip(encs, maps):
            recode(e, [0], [m])
        keys = g.keys()
        for e, was, (txt, isnull, _) in zip(encs, before, parts):
            now = decode(e)
            notnull = now[0]["notnull"] if now[0]["notnull"] is not None else np.ones(n, dtype=bool)
            assert np.array_equal(notnull, ~isnull)
            assert (was[0]["notnull"] is None) == (now[0]["notnull"] is None)
            for row in range(n):
                if isnull[row]:
                    assert now[0]["values"][row] == 0
                else:
                    assert keys[now[0]["values"][row]] == row_key(txt[row], kind), row
            assert now[0]["stat_flags"] & 1 and (now[0]["minval"], now[0]["maxval"]) == (0, g.num_keys - 1)
            same_column(now[1], was[1])
            same_column(now[2], was[2])
    finally:
        for x in maps + encs + dicts + [c for _, _, c in parts] + ([g] if g else []):
            x.release()


def test_recode_of_an_all_null_chunk_and_of_ids_the_map_does_not_have():
    n = 300
    nulls = upload_keys("text", [b""] * n, np.ones(n, dtype=bool))
    ten = upload_keys("text", [W[i % 10] for i in range(n)])
    three = upload_keys("text", [W[i % 3] for i in range(n)])
    d0, d10, d3, g = (TextDictionary("text") for _ in range(4))
    held = [nulls, ten, three, d0, d10, d3, g]
    try:
        e0 = d0.encode(nulls, [0])
        held.append(e0)
        assert d0.num_keys == 0
        g.encode(three, [0]).release()
        m0 = g.absorb_dict(d0)
        held.append(m0)
        assert len(m0) == 0
        recode(e0, [0], [m0])
        c = decode(e0)[0]
        assert not c["notnull"].any() and not c["values"].any()
        # ids 0..9 through a map of 3 entries
        e10 = d10.encode(ten, [0])
        held.append(e10)
        d3.encode(three, [0]).release()
        m3 = g.absorb_dict(d3)
        held.append(m3)
        assert len(m3) == 3 and d10.num_keys == 10
        with pytest.raises(runtime.StromError) as ei:
            recode(e10, [0], [m3])
        assert ei.value.errcode == CORRUPTION
    finally:
        for x in reversed(held):
            x.release()


# ---- 7. GROUP BY over three shards -----------------------------------------------------------------
SPEC1 = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)) (pmin (var 3 int4)))"
SPEC2 = "(gpupreagg (key (var 1 int4)) (key (var 2 int4)) (nrows) (psum (var 3 int8)) (pmin (var 4 int4)))"
# rows of the chunks: shard 0 has one chunk, shard 1 two, shard 2 one with NULL keys only
BOUNDS = [[(0, 900)], [(900, 1700), (1700, 2300)], [(2300, 2600)]]
NROWS = 2600


@pytest.fixture(scope="module")
def sharded_table():
    """(text t, character(12) c, int4 g, int8 v, int4 x).  Keys: shard 0 draws from W[:18] and
    k0000..k0059, the first chunk of shard 1 from W[9:] and k0040..k0099 (overlap), its second chunk
    from keys no other chunk has (disjoint), shard 2 has none"""
    rng = np.random.default_rng(77)
    ks = [(b"k%04d" % i) * (1 + i % 30) for i in range(100)]
    pools = [W[:18] + ks[:60], W[9:] + ks[40:], [b"apart %d" % i for i in range(70)], [b""]]
    t, c = [], []
    for pool, (lo, hi) in zip(pools, [b for s in BOUNDS for b in s]):
        t += [pool[i] for i in rng.integers(0, len(pool), hi - lo)]
        c += [(pool[i][:12] + b" " * 12)[:12] for i in rng.integers(0, len(pool), hi - lo)]
    tnull = rng.random(NROWS) < 0.05
    tnull[2300:] = True
    cnull = np.zeros(NROWS, dtype=bool)
    cnull[2300:] = True
    tb = dict(t=t, c=c, tnull=tnull, cnull=cnull, g=rng.integers(-3, 4, NROWS).astype(np.int32),
              v=rng.integers(-10**12, 10**12, NROWS), x=rng.integers(-1000, 1000, NROWS).astype(np.int32))
    shards = [[runtime.DeviceStore.upload(kds.build_kds("column", [
        kds.Column("text", t[lo:hi], tnull[lo:hi]), kds.Column("character", c[lo:hi], cnull[lo:hi]),
        kds.Column("int4", tb["g"][lo:hi]), kds.Column("int8", tb["v"][lo:hi]),
        kds.Column("int4", tb["x"][lo:hi])])) for lo, hi in bounds] for bounds in BOUNDS]
    yield tb, shards
    for s in shards:
        for chunk in s:
            chunk.release()


def expected_groups(tb, key_fn):
    want = {}
    for i in range(NROWS):
        k = key_fn(i)
        cnt, sm, mn = want.get(k, (0, 0, None))
        want[k] = (cnt + 1, sm + int(tb["v"][i]), int(tb["x"][i]) if mn is None else min(mn, int(tb["x"][i])))
    return want


def groups_of(pr, keycols, nkeys):
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


CASES = {
    "text": ([(0, "text")], SPEC1, [3, 4], (), 1),
    "character": ([(1, "character")], SPEC1, [3, 4], (), 1),
    "text_int4": ([(0, "text")], SPEC2, [2, 3, 4], (1,), 2),
}


@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_group_by_over_three_shards(sharded_table, case, hashed):
    tb, shards = sharded_table
    text_keys, spec, carry, int_keys, nkeys = CASES[case]
    tkey = lambda i: None if tb["tnull"][i] else tb["t"][i]
    ckey = lambda i: None if tb["cnull"][i] else tb["c"][i].rstrip(b" ")
    key_fn = {"text": tkey, "character": ckey, "text_int4": lambda i: (tkey(i), int(tb["g"][i]))}[case]
    pr, keycols = group_by_text_sharded(shards, text_keys, spec, carry, hashed=hashed, int_keys=int_keys)
    got = groups_of(pr, keycols, nkeys)
    want = expected_groups(tb, key_fn)
    assert (None in want) if nkeys == 1 else any(k[0] is None for k in want)     # the NULL key group is there
    assert got == want
    # one dictionary over the same chunks: the same groups by key bytes, the same partials
    pr1, keycols1 = group_by_text([c for s in shards for c in s], text_keys, spec, carry, hashed=hashed,
                                  int_keys=list(int_keys))
    assert groups_of(pr1, keycols1, nkeys) == got


# ---- 8. refusals -----------------------------------------------------------------------------------
def test_bad_requests_are_refused_before_any_launch():
    n = 300
    txt = [W[i % len(W)] for i in range(n)]
    cols = [kds.Column("text", txt), kds.Column("int8", np.arange(n, dtype=np.int64))]
    column = runtime.DeviceStore.upload(kds.build_kds("column", cols))
    rows = runtime.DeviceStore.upload(kds.build_kds("row", [kds.Column("int4", np.arange(n, dtype=np.int32))]))
    d, other, chars = TextDictionary("text"), TextDictionary("text"), TextDictionary("character")
    heap, offs = image_of(txt[:5])
    hbuf = np.frombuffer(heap, dtype=np.uint8)
    enc = m = None

    def absorb(dst, heap_p, offs_p, nkeys):
        err = ctypes.c_int(0)
        assert not lib.strom_keyunion_absorb(dst, heap_p, len(heap), offs_p, nkeys, ctypes.byref(err))
        return err.value

    def absorb_dict(dst, src):
        err = ctypes.c_int(0)
        assert not lib.strom_keyunion_absorb_dict(dst, src, ctypes.byref(err))
        return err.value

    def recode_rc(store, cols_, maps_):
        colidx = (ctypes.c_int32 * 9)(*(list(cols_) + [0] * (9 - len(cols_))))
        handles = (ctypes.c_void_p * 9)(*(list(maps_) + [None] * (9 - len(maps_))))
        return lib.strom_keyunion_recode(store, colidx, handles, len(cols_))

    try:
        assert absorb(None, hbuf.ctypes.data, offs.ctypes.data, 5) == BAD_REQUEST
        assert absorb(d.handle, None, offs.ctypes.data, 5) == BAD_REQUEST         # keys without a heap
        assert absorb(d.handle, hbuf.ctypes.data, None, 5) == BAD_REQUEST         # ... without offsets
        assert absorb_dict(None, d.handle) == BAD_REQUEST
        assert absorb_dict(d.handle, None) == BAD_REQUEST
        assert absorb_dict(d.handle, d.handle) == BAD_REQUEST                     # dst == src
        assert absorb_dict(d.handle, chars.handle) == BAD_REQUEST                 # text <- character(n)
        assert absorb_dict(chars.handle, d.handle) == BAD_REQUEST
        assert d.num_keys == 0 and chars.num_keys == 0
        enc = other.encode(column, [0], [1])                                      # (int4 ids, int8)
        m = d.absorb_dict(other)
        assert recode_rc(None, [0], [m.handle]) == BAD_REQUEST                    # not resident
        assert recode_rc(rows.handle, [0], [m.handle]) == BAD_REQUEST             # not a COLUMN chunk
        assert recode_rc(enc.handle, [1], [m.handle]) == BAD_REQUEST              # int8: not an id column
        assert recode_rc(column.handle, [0], [m.handle]) == BAD_REQUEST           # text offsets: attlen -1
        assert recode_rc(enc.handle, [2], [m.handle]) == BAD_REQUEST              # no such column
        assert recode_rc(enc.handle, [0], [None]) == BAD_REQUEST                  # NULL map
        assert recode_rc(enc.handle, [], []) == BAD_REQUEST                       # ncols 0
        assert recode_rc(enc.handle, [0] * 9, [m.handle] * 9) == BAD_REQUEST      # ncols 9
        assert recode_rc(enc.handle, [0, 0], [m.handle, m.handle]) == BAD_REQUEST  # a column twice
        assert lib.strom_keyunion_recode(enc.handle, None, None, 1) == BAD_REQUEST
        # nothing was rewritten by the refused calls; the good one goes through
        ids = decode(enc)[0]["values"].copy()
        recode(enc, [0], [m])
        assert [d.keys()[i] for i in decode(enc)[0]["values"]] == [other.keys()[i] for i in ids] == txt
    finally:
        for x in (m, enc, d, other, chars, column, rows):
            if x is not None:
                x.release()
