"""
text / character(n) columns in GpuHashJoin's COLUMN projection (needs an MI355X: -m gpu):
strom_hashjoin_project_column() sizes the heap area with a counting kernel, then the projection
copies every joined row's datum there and leaves its offset in the column array
(include/strom_kds.h).  Every case projects an outer int8 row number and the inner key next to
the text columns, so each joined row names its own source rows and no check depends on the
join's result order.  Two readers: Python's bytes from the source tables (tests/text_cases.py),
and the oracle's / the HIP scan over the downloaded chunk (check() of test_gpuscan_gpu.py).
"""
import contextlib

import numpy as np
import pytest

import text_cases
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpupreagg import GpuPreAgg
from pg_strom_amd.gpuscan import GpuScan
from test_gpuscan_gpu import check

pytestmark = pytest.mark.gpu

ERR_BAD_REQUEST = 101
ERR_CORRUPTION = 300
KEY_JOIN = "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))"


def align(n, a):
    return (n + a - 1) & ~(a - 1)


def room(payload):
    """bytes a datum takes in the heap area: the whole varlena, rounded to the 4-byte boundary"""
    return align(len(kds.varlena_datum(payload)), 4)


@contextlib.contextmanager
def joined_chunk(outer, inners, keys, dest_columns, spec=KEY_JOIN, ratio=1.0, rowmap_qual=None):
    """join the resident 'outer' and leave the rows as a COLUMN chunk: yields (DeviceStore, its
    download, nitems).  rowmap_qual: a GpuScan in front whose row map the join reads."""
    runtime.init()
    ds = runtime.DeviceStore.upload(outer)
    join = GpuHashJoin(spec, row_population_ratio=ratio).begin(build_multihash(list(zip(inners, keys))))
    scan = GpuScan(rowmap_qual).begin() if rowmap_qual else None
    joined = rowmap = None
    try:
        if scan:
            rowmap, _ = scan.scan_to_rowmap(ds)
        joined, nitems = join.join_to_column(ds, dest_columns, row_map=rowmap)
        yield joined, joined.download(), nitems
    finally:
        if joined is not None:
            joined.release()
        if rowmap is not None:
            rowmap.release()
        if scan:
            scan.end()
        join.end()
        ds.release()


def int_column(image, col):
    """(values as int64, isnull) of a fixed-width column of the download"""
    c = kds.decode_column_chunk(image)[col]
    isnull = np.zeros(len(c["values"]), dtype=bool) if c["notnull"] is None else ~c["notnull"]
    return c["values"].astype(np.int64), isnull


def scanned_rows(res):
    return np.sort(np.asarray(res.results[:res.nitems], dtype=np.int64)) - 1


def heap_invariants(image, text_cols, want_heap_bytes):
    """what include/strom_kds.h promises of the heap area, and that the sizing pass was exact"""
    head = kds.KdsHead(image)
    cols = kds.decode_column_chunk(image)
    heap_off = cols[text_cols[0]]["extra_off"]
    assert heap_off != 0 and heap_off % 256 == 0
    spans = []
    for c in text_cols:
        assert cols[c]["extra_off"] == heap_off and cols[c]["stat_flags"] == 0
        m = head.colmeta[c]
        assert (int(m["attlen"]), int(m["attbyval"]), int(m["attalign"])) == (-1, 0, 4)
        offs = cols[c]["values"].view(np.uint64)
        nn = cols[c]["notnull"]
        for i in range(head.nitems):
            at = int(offs[i])
            if nn is not None and not nn[i]:
                assert at == 0, (c, i)                       # NULL: offset 0 and a clear bit
                continue
            assert at != 0 and heap_off <= at < head.usage and at % 4 == 0, (c, i, at)
            b0 = int(image[at])
            size = (2 + (16 if int(image[at + 1]) == 18 else 8)) if b0 == 1 else ((b0 >> 1) & 0x7f) if b0 & 1 \
                else int(np.frombuffer(image[at:at + 4].tobytes(), dtype="<u4")[0]) >> 2
            spans.append((at, align(size, 4)))
    spans.sort()
    for (a, la), (b, _) in zip(spans, spans[1:]):
        assert a + la <= b, (a, la, b)                       # no two datums overlap
    if spans:
        assert spans[-1][0] + spans[-1][1] <= head.usage
    assert head.usage - heap_off == sum(l for _, l in spans) == want_heap_bytes
    assert head.length == align(head.usage, 256) and len(image) >= head.length


# ---------------------------------------------------------------------------------------------
# 1 + 2: every outer format; five whole projection tiles (256 threads x 4 records) and a ragged one
# ---------------------------------------------------------------------------------------------
N_FORMATS = 6000
FORMATS_QUAL = ("(or (texteq (var 1 text) (const text 'hello')) (or (bpchareq (var 2 character) (const character 'SHIP'))"
                " (text_lt (var 3 text) (const text 'b'))))")


def dimension_with_text(seed=8):
    rng = np.random.default_rng(seed)
    pk = np.arange(-50, 50, dtype=np.int32)
    words = [text_cases.WORDS[i] for i in rng.integers(0, len(text_cases.WORDS), 100)]
    wnull = np.arange(100) % 7 == 2
    pay = rng.integers(0, 1000, 100).astype(np.int32)
    payn = np.arange(100) % 5 == 1
    inner = kds.build_kds("row", [kds.Column("int4", pk), kds.Column("text", words, wnull), kds.Column("int4", pay, payn)])
    return inner, words, wnull, pay, payn


@pytest.fixture(scope="module", params=["row", "row_flat", "column"])
def formats_case(request):
    outer, txt, chr10, num, tnull = text_cases.text_table(N_FORMATS, 31, request.param)
    inner, words, wnull, pay, payn = dimension_with_text()
    dest = [(0, 2, "text"), (0, 3, "character"), (1, 2, "text"), (1, 3, "int4"), (0, 4, "int8"), (1, 1, "int4")]
    with joined_chunk(outer, [inner], [[1]], dest) as (joined, image, nitems):
        scan = GpuScan(FORMATS_QUAL).begin()
        try:
            resident = scan.scan_chunk(joined)
        finally:
            scan.end()
    return dict(image=image, nitems=nitems, resident=resident, txt=txt, chr10=chr10, num=num, tnull=tnull,
                words=words, wnull=wnull, pay=pay, payn=payn)


def test_every_datum_of_every_joined_row_equals_its_source(formats_case):
    c = formats_case
    image = c["image"]
    assert c["nitems"] == N_FORMATS == kds.KdsHead(image).nitems
    o, onull = int_column(image, 4)
    key, knull = int_column(image, 5)
    pay, payn = int_column(image, 3)
    assert not onull.any() and not knull.any()
    assert np.array_equal(np.sort(o), np.arange(N_FORMATS))            # every outer row, once
    d = key + 50
    assert np.array_equal(key, c["num"][o])
    assert np.array_equal(payn, c["payn"][d]) and np.array_equal(pay[~payn], c["pay"][d][~payn])
    otext = kds.decode_text_column(image, 0)
    ochr = kds.decode_text_column(image, 1)
    itext = kds.decode_text_column(image, 2)
    for i in range(N_FORMATS):
        assert otext[i] == (None if c["tnull"][o[i]] else c["txt"][o[i]]), i
        assert ochr[i] == c["chr10"][o[i]], i
        assert itext[i] == (None if c["wnull"][d[i]] else c["words"][d[i]]), i
    # a text qual over the result, resident and downloaded: the oracle's scan, the HIP scan, Python
    want = np.array([i for i in range(N_FORMATS)
                     if otext[i] == b"hello" or text_cases.bpchar_key(ochr[i]) == b"SHIP"
                     or (itext[i] is not None and itext[i] < b"b")], dtype=np.int64)
    assert 0 < len(want) < N_FORMATS
    assert c["resident"].errcode == 0 and np.array_equal(scanned_rows(c["resident"]), want)
    res = check(FORMATS_QUAL, image)
    assert res.errcode == 0 and np.array_equal(scanned_rows(res), want)


def test_heap_area_invariants_and_exact_sizing(formats_case):
    c = formats_case
    image = c["image"]
    o, _ = int_column(image, 4)
    d = int_column(image, 5)[0] + 50
    want = sum(0 if c["tnull"][a] else room(c["txt"][a]) for a in o)
    want += sum(room(c["chr10"][a]) for a in o)
    want += sum(0 if c["wnull"][b] else room(c["words"][b]) for b in d)
    heap_invariants(image, [0, 1, 2], want)
    cols = kds.decode_column_chunk(image)
    assert cols[1]["notnull"] is None                      # character(10) has no NULL: nulls_off == 0
    assert cols[0]["notnull"] is not None and cols[2]["notnull"] is not None
    # fixed-width columns next to them keep their zone maps
    assert cols[5]["stat_flags"] & 1 and (cols[5]["minval"], cols[5]["maxval"]) == (-50, 49)


# ---------------------------------------------------------------------------------------------
# 3: datum forms, on both sides of the join; fewer rows than a wave, one record into a second tile
# ---------------------------------------------------------------------------------------------
def pattern(n, salt):
    return bytes((salt + 131 * k) % 256 for k in range(n))


# payloads: the 1-byte datum; 1-byte headers of 2, 3, 4 and 127 bytes in all; 4-byte headers over 128, 129, 1000
FORMS = [b"", b"\x80", b"\xff\xfe", b"a\xc3\xa9", pattern(126, 200), pattern(128, 90), pattern(129, 250), pattern(1000, 128)]


@pytest.mark.parametrize("n", [37, 1025])
@pytest.mark.parametrize("fmt", ["row", "column"])
def test_datum_forms_on_both_sides(fmt, n):
    assert [len(kds.varlena_datum(f)) for f in FORMS] == [1, 2, 3, 4, 127, 132, 133, 1004]
    nf = len(FORMS)
    otxt = [FORMS[(i // nf + i) % nf] for i in range(n)]
    fk = (np.arange(n) % nf).astype(np.int32)
    outer = kds.build_kds(fmt, [kds.Column("int4", fk), kds.Column("text", otxt), kds.Column("int8", np.arange(n, dtype=np.int64))])
    itxt = [FORMS[(j + 3) % nf] for j in range(nf)]
    inner = kds.build_kds("row_flat", [kds.Column("int4", np.arange(nf, dtype=np.int32)), kds.Column("text", itxt)])
    dest = [(0, 3, "int8"), (1, 1, "int4"), (0, 2, "text"), (1, 2, "text")]
    with joined_chunk(outer, [inner], [[1]], dest) as (_, image, nitems):
        pass
    assert nitems == n
    o = int_column(image, 0)[0]
    d = int_column(image, 1)[0]
    assert np.array_equal(np.sort(o), np.arange(n)) and np.array_equal(d, fk[o])
    got_o = kds.decode_text_column(image, 2)
    got_i = kds.decode_text_column(image, 3)
    for i in range(n):
        assert got_o[i] == otxt[o[i]] and got_i[i] == itxt[d[i]], i
    heap_invariants(image, [2, 3], sum(room(otxt[a]) for a in o) + sum(room(itxt[b]) for b in d))
    cols = kds.decode_column_chunk(image)
    assert cols[2]["notnull"] is None and cols[3]["notnull"] is None
    # an independent reader over the bytes >= 0x80 and the long datums
    res = check("(or (texteq (var 3 text) (param 0 text)) (text_gt (var 4 text) (param 1 text)))", image,
                (FORMS[7], FORMS[4]))
    want = [i for i in range(n) if got_o[i] == FORMS[7] or got_i[i] > FORMS[4]]
    assert res.errcode == 0 and np.array_equal(scanned_rows(res), np.array(want, dtype=np.int64))


# ---------------------------------------------------------------------------------------------
# 4: empty totals
# ---------------------------------------------------------------------------------------------
def test_text_columns_that_are_null_in_every_joined_row():
    """no wave reserves anything: the heap area is empty, usage / length / extra_off agree"""
    n = 1500
    fk = (np.arange(n) % 100).astype(np.int32)
    outer = kds.build_kds("column", [kds.Column("int4", fk), kds.Column("text", [b"x"] * n, np.ones(n, dtype=bool)),
                                     kds.Column("int8", np.arange(n, dtype=np.int64))])
    inner = kds.build_kds("row", [kds.Column("int4", np.arange(100, dtype=np.int32)),
                                  kds.Column("text", [b"never read"] * 100, np.ones(100, dtype=bool))])
    dest = [(0, 3, "int8"), (1, 1, "int4"), (0, 2, "text"), (1, 2, "text")]
    with joined_chunk(outer, [inner], [[1]], dest) as (_, image, nitems):
        pass
    assert nitems == n
    head = kds.KdsHead(image)
    cols = kds.decode_column_chunk(image)
    for c in (2, 3):
        assert not cols[c]["values"].any() and cols[c]["notnull"] is not None and not cols[c]["notnull"].any()
        assert cols[c]["extra_off"] == head.usage
        assert kds.decode_text_column(image, c) == [None] * n
    assert head.usage % 256 == 0 and head.length == head.usage == len(image)
    res = check("(isnull (var 3 text))", image)
    assert res.nitems == n
    assert check("(texteq (var 4 text) (const text 'never read'))", image).nitems == 0


def test_a_join_without_matches_gives_a_valid_empty_chunk():
    n = 3000
    outer = kds.build_kds("column", [kds.Column("int4", np.full(n, 1000, dtype=np.int32)), kds.Column("text", [b"abc"] * n),
                                     kds.Column("int8", np.arange(n, dtype=np.int64))])
    inner, *_ = dimension_with_text()
    dest = [(0, 3, "int8"), (1, 1, "int4"), (0, 2, "text"), (1, 2, "text")]
    with joined_chunk(outer, [inner], [[1]], dest) as (_, image, nitems):
        pass
    assert nitems == 0
    head = kds.KdsHead(image)
    assert head.nitems == 0 and head.format == kds.KDS_FORMAT_COLUMN and head.ncols == 4
    assert head.length == align(head.usage, 256) == len(image)
    cols = kds.decode_column_chunk(image)
    assert all(len(c["values"]) == 0 for c in cols)
    assert int(head.colmeta[2]["attlen"]) == -1 and int(head.colmeta[0]["attlen"]) == 8
    assert kds.decode_text_column(image, 2) == [] and check("(isnull (var 4 text))", image).nitems == 0


# ---------------------------------------------------------------------------------------------
# 5: one inner datum copied into several rows: duplicate keys, a row map in front
# ---------------------------------------------------------------------------------------------
def test_duplicate_inner_keys_behind_a_row_map():
    n = 4000
    outer, txt, chr10, num, tnull = text_cases.text_table(n, 52, "column")
    W = text_cases.WORDS
    nd = 300                                                 # key = j // 3 - 50, three rows per key
    ikey = (np.arange(nd) // 3 - 50).astype(np.int32)
    disc = (np.arange(nd) % 3).astype(np.int16)
    words = [W[(7 * j) % len(W)] + b"#%d" % j for j in range(nd)]
    wnull = np.arange(nd) % 11 == 5
    inner = kds.build_kds("row", [kds.Column("int4", ikey), kds.Column("int2", disc), kds.Column("text", words, wnull)])
    dest = [(0, 4, "int8"), (1, 1, "int4"), (1, 2, "int2"), (1, 3, "text"), (0, 2, "text")]
    with joined_chunk(outer, [inner], [[1]], dest, ratio=3.3,
                      rowmap_qual="(int4gt (var 1 int4) (const int4 -30))") as (_, image, nitems):
        pass
    sel = np.flatnonzero(num > -30)
    assert nitems == 3 * len(sel)
    o = int_column(image, 0)[0]
    key = int_column(image, 1)[0]
    dsc = int_column(image, 2)[0]
    want_pairs = np.stack([np.repeat(sel, 3), np.tile(np.arange(3), len(sel))], axis=1)
    got_pairs = np.stack([o, dsc], axis=1)
    assert np.array_equal(got_pairs[np.lexsort(got_pairs.T[::-1])], want_pairs)       # each (outer row, inner row) once
    assert np.array_equal(key, num[o])
    d = (key + 50) * 3 + dsc
    itext = kds.decode_text_column(image, 3)
    otext = kds.decode_text_column(image, 4)
    for i in range(nitems):
        assert itext[i] == (None if wnull[d[i]] else words[d[i]]), i
        assert otext[i] == (None if tnull[o[i]] else txt[o[i]]), i
    heap_invariants(image, [3, 4], sum(0 if wnull[b] else room(words[b]) for b in d)
                    + sum(0 if tnull[a] else room(txt[a]) for a in o))


# ---------------------------------------------------------------------------------------------
# 6: text columns from depth 1 and depth 2 of a two-level join
# ---------------------------------------------------------------------------------------------
def test_text_columns_from_both_relations_of_a_two_level_join():
    rng = np.random.default_rng(17)
    n, n1 = 5000, 500
    names = [b"region-%03d" % (i % 37) for i in range(n1)]
    nnull = np.arange(n1) % 29 == 3
    dim1 = kds.build_kds("row", [kds.Column("int4", np.arange(n1, dtype=np.int32)), kds.Column("text", names, nnull)])
    words = [b"region-%03d" % i for i in range(0, 40, 2)] + [b"region-%03d" % 4]      # even regions, one twice
    dim2 = kds.build_kds("row_flat", [kds.Column("text", words), kds.Column("int4", np.arange(len(words), dtype=np.int32))])
    fk = rng.integers(-5, n1 + 20, n).astype(np.int32)
    outer = kds.build_kds("column", [kds.Column("int4", fk), kds.Column("int8", np.arange(n, dtype=np.int64))])
    spec = "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)) (rel (hashkey (ivar 1 2 text) 1 text)))"
    dest = [(0, 2, "int8"), (1, 1, "int4"), (1, 2, "text"), (2, 1, "text"), (2, 2, "int4")]
    with joined_chunk(outer, [dim1, dim2], [[1], [1]], dest, spec=spec, ratio=1.2) as (_, image, nitems):
        pass
    cnt = {}
    for w in words:
        cnt[w] = cnt.get(w, 0) + 1
    assert nitems == sum(cnt.get(names[k], 0) for k in fk if 0 <= k < n1 and not nnull[k]) > 0
    o = int_column(image, 0)[0]
    k1 = int_column(image, 1)[0]
    e = int_column(image, 4)[0]
    name = kds.decode_text_column(image, 2)
    word = kds.decode_text_column(image, 3)
    assert np.array_equal(k1, fk[o])
    pairs = set()
    for i in range(nitems):
        assert name[i] == names[k1[i]] == words[e[i]] == word[i], i
        pairs.add((int(o[i]), int(e[i])))
    assert len(pairs) == nitems                               # no pair twice
    heap_invariants(image, [2, 3], 2 * sum(room(w) for w in word))


# ---------------------------------------------------------------------------------------------
# 7: compressed and external datums are carried, not interpreted
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["row", "column"])
def test_unreadable_datums_are_copied_whole_and_still_go_back_to_the_cpu(fmt):
    plain = kds.varlena_datum(b"abc")
    compressed = np.array([(20 << 2) | 2], dtype="<u4").tobytes() + b"\0" * 16
    external = bytes([0x01, 18]) + b"\0" * 16
    datums = [plain, compressed, external, plain] * 500
    n = len(datums)
    fk = (np.arange(n) % 123).astype(np.int32)
    outer = kds.build_kds(fmt, [kds.Column("int4", fk), kds.Column("text_raw", datums), kds.Column("int8", np.arange(n, dtype=np.int64))])
    inner = kds.build_kds("row", [kds.Column("int4", np.arange(100, dtype=np.int32))])
    with joined_chunk(outer, [inner], [[1]], [(0, 3, "int8"), (1, 1, "int4"), (0, 2, "text")]) as (_, image, nitems):
        pass
    src = np.flatnonzero(fk < 100)
    assert nitems == len(src)
    o = int_column(image, 0)[0]
    assert np.array_equal(np.sort(o), src)
    got = kds.decode_text_column(image, 2)
    for i in range(nitems):
        want = datums[o[i]]
        assert got[i] == (b"abc" if want is plain else bytearray(want)), i
    res = check("(texteq (var 3 text) (const text 'abc'))", image)
    assert len(res.passed_rows()) == sum(1 for a in src if datums[a] is plain) > 0
    assert len(res.recheck_rows()) == sum(1 for a in src if datums[a] is not plain) > 0


# ---------------------------------------------------------------------------------------------
# 8: Scan -> Join -> PreAgg stays in HBM with a text column
# ---------------------------------------------------------------------------------------------
def test_scan_join_preagg_chain_with_a_text_column():
    n, nd = 50021, 4000
    rng = np.random.default_rng(61)
    fk = rng.integers(0, int(nd * 1.25), n).astype(np.int32)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    b = rng.random(n)
    fact = kds.build_kds("column", [kds.Column("int4", fk), kds.Column("int4", a), kds.Column("float8", b)])
    dkey = rng.permutation(nd).astype(np.int32)
    dgrp = (dkey % 37).astype(np.int32)
    W = text_cases.WORDS
    dname = [W[i] for i in rng.integers(0, len(W), nd)]
    dnull = rng.random(nd) < 0.05
    inner = kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp), kds.Column("text", dname, dnull)])
    spec = "(gpupreagg (qual (text_ge (var 3 text) (const text 'b'))) (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))))"
    agg = GpuPreAgg(spec)
    qual = "(and (int4lt (var 2 int4) (const int4 1073741824)) (float8gt (var 3 float8) (const float8 0.25)))"
    try:
        with joined_chunk(fact, [inner], [[1]], [(1, 2, "int4"), (0, 2, "int4"), (1, 3, "text")],
                          rowmap_qual=qual) as (joined, image, nitems):
            agg.begin([(0, 37)])
            assert agg.fold(joined)[0] == 0
            pr = agg.fetch()
    finally:
        agg.end()
    sel = np.flatnonzero((a < 2**30) & (b > 0.25) & (fk < nd))
    assert nitems == len(sel)
    pos = np.empty(nd, dtype=np.int64)
    pos[dkey] = np.arange(nd)
    di = pos[fk[sel]]
    keep = np.array([not dnull[d] and dname[d] >= b"b" for d in di])
    assert 0 < keep.sum() < len(sel)
    g = dgrp[di][keep]
    keys, _ = pr.column(0)
    order = np.argsort(keys)
    ug, inv = np.unique(g, return_inverse=True)
    assert np.array_equal(keys[order], ug)
    assert np.array_equal(pr.column(1)[0][order], np.bincount(inv))
    sums = np.zeros(len(ug), dtype=np.int64)
    np.add.at(sums, inv, a[sel][keep].astype(np.int64))
    assert np.array_equal(pr.column(2)[0][order], sums)


# ---------------------------------------------------------------------------------------------
# 9: refusals (checked on the host or by the kernels: nothing is followed, nothing is copied)
# ---------------------------------------------------------------------------------------------
def refused(outer, inner, dest):
    with pytest.raises(runtime.StromError) as ei:
        with joined_chunk(outer, [inner], [[1]], dest):
            pass
    return ei.value.errcode


def test_mappings_and_chunks_that_do_not_fit_are_refused():
    n = 3000
    outer, *_ = text_cases.text_table(n, 3, "column")          # int4, text, character(10), int8
    inner, *_ = dimension_with_text()                           # int4, text, int4
    rows, *_ = text_cases.text_table(n, 3, "row")
    # a text destination on an int4 source: the outer COLUMN array, a heap tuple, an inner tuple
    assert refused(outer, inner, [(0, 4, "int8"), (0, 1, "text")]) == ERR_CORRUPTION
    assert refused(rows, inner, [(0, 4, "int8"), (0, 1, "character")]) == ERR_CORRUPTION
    assert refused(outer, inner, [(0, 4, "int8"), (1, 3, "text")]) == ERR_CORRUPTION
    # an int8 destination on a text source
    assert refused(outer, inner, [(0, 2, "int8"), (0, 4, "int8")]) == ERR_CORRUPTION
    assert refused(outer, inner, [(1, 2, "int8"), (0, 4, "int8")]) == ERR_CORRUPTION
    # a TUPSLOT outer chunk holds by-value datums
    slots = kds.build_kds("tupslot", [kds.Column("int4", (np.arange(n) % 100 - 50).astype(np.int32)),
                                      kds.Column("int8", np.arange(n, dtype=np.int64))])
    assert refused(slots, inner, [(0, 2, "text"), (1, 1, "int4")]) == ERR_BAD_REQUEST
    # a datum whose header claims more bytes than the chunk holds: never read by that length
    liar = kds.build_kds("column", [kds.Column("int4", (np.arange(1000) % 100 - 50).astype(np.int32)),
                                    kds.Column("text", [b"abc"] * 999 + [b"x" * 200])])
    at = int(kds.decode_column_chunk(liar)[1]["values"].view(np.uint64)[999])
    assert int(liar[at:at + 4].view(np.uint32)[0]) == 204 << 2
    liar[at:at + 4] = np.array([(1 << 29) << 2], dtype="<u4").view(np.uint8)
    assert refused(liar, inner, [(0, 2, "text"), (1, 1, "int4")]) == ERR_CORRUPTION
    # ... an offset whose 4-byte header would end beyond the chunk, and an offset beyond the chunk
    for delta in (-1, 0, 1 << 20):
        liar = kds.build_kds("column", [kds.Column("int4", (np.arange(1000) % 100 - 50).astype(np.int32)),
                                        kds.Column("text", [b"abc"] * 1000)])
        values_off = int(liar[96:100].view(np.uint32)[0])       # coldir[1].values_off (KDS_HEAD_LENGTH(2) == 64)
        liar[values_off + 8 * 500:values_off + 8 * 501] = np.array([kds.KdsHead(liar).length + delta], dtype="<u8").view(np.uint8)
        assert int(kds.decode_column_chunk(liar)[1]["values"].view(np.uint64)[500]) == kds.KdsHead(liar).length + delta
        assert refused(liar, inner, [(0, 2, "text"), (1, 1, "int4")]) == ERR_CORRUPTION
    # the same objects still serve a mapping that fits
    with joined_chunk(outer, [inner], [[1]], [(0, 2, "text"), (0, 4, "int8")]) as (_, image, nitems):
        pass
    assert nitems == n and kds.KdsHead(image).nitems == n


# ---------------------------------------------------------------------------------------------
# 10: nothing moved for fixed widths
# ---------------------------------------------------------------------------------------------
def test_fixed_width_mapping_has_no_heap_area():
    n, nd = 20000, 4000
    rng = np.random.default_rng(61)
    fk = rng.integers(0, int(nd * 1.25), n).astype(np.int32)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    an = rng.random(n) < 0.03
    b = rng.random(n)
    fact = kds.build_kds("column", [kds.Column("int4", fk), kds.Column("int4", a, an), kds.Column("float8", b)])
    dkey = rng.permutation(nd).astype(np.int32)
    dgrp = (dkey % 37).astype(np.int32)
    dval = rng.random(nd) * 10
    dvaln = rng.random(nd) < 0.05
    inner = kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp), kds.Column("float8", dval, dvaln)])
    qual = "(and (int4lt (var 2 int4) (const int4 1073741824)) (float8gt (var 3 float8) (const float8 0.25)))"
    dest = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8"), (1, 3, "float8")]
    with joined_chunk(fact, [inner], [[1]], dest, rowmap_qual=qual) as (_, image, nitems):
        pass
    sel = np.flatnonzero((~an) & (a < 2**30) & (b > 0.25) & (fk < nd))
    assert nitems == len(sel)
    head = kds.KdsHead(image)
    cols = kds.decode_column_chunk(image)
    assert head.usage == 0 and all(c["extra_off"] == 0 for c in cols)
    assert all(int(m["attlen"]) > 0 and int(m["attbyval"]) == 1 for m in head.colmeta)
    # the arrays and nothing behind them (a bitmap's room stays where the column has no NULL)
    want_len = 256 + sum(align(w * nitems, 256) + align(4 * ((nitems + 31) // 32), 256) for w in (4, 4, 8, 8))
    assert head.length == want_len == len(image)
    pos = np.empty(nd, dtype=np.int64)
    pos[dkey] = np.arange(nd)
    di = pos[fk[sel]]
    got = np.stack([cols[0]["values"].astype(np.int64), cols[1]["values"].astype(np.int64),
                    cols[2]["values"].view(np.int64), cols[3]["values"].view(np.int64)], axis=1)
    want = np.stack([dgrp[di].astype(np.int64), a[sel].astype(np.int64), b[sel].view(np.int64),
                     np.where(dvaln, 0.0, dval)[di].view(np.int64)], axis=1)
    assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])
    assert cols[0]["notnull"] is None and cols[1]["notnull"] is None
    nn = cols[3]["notnull"]
    assert nn is not None and int((~nn).sum()) == int(dvaln[di].sum())
    assert cols[0]["stat_flags"] & 1 and cols[0]["minval"] == int(dgrp[di].min()) and cols[0]["maxval"] == int(dgrp[di].max())
