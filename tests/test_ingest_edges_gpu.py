"""
Device ingest (ingest_to_column*, ingest_minmax, ingest_finish: csrc/devlib/strom_ingest.h) and
the join's COLUMN projection at the edges their loops have, against the independent model of
tests/zone_map_model.py (needs an MI355X: -m gpu).  Every device result is checked twice: the
downloaded COLUMN content equals the model of the SOURCE, and each zone map equals the model of
that CONTENT.  All assertions are exact.

STROM_INGEST_MAX_GRID=2 makes the grid-stride loops turn on small chunks: the transposition
strides 512 rows, ingest_minmax strides 512 vectors of 16 bytes.  With nvec = 4685 =
2*4*512 + 512 + 77 vectors the four-loads-in-flight loop runs twice, the one-vector loop once
for every thread and once more for 77 threads, and per_vec - 1 tail rows follow the last vector.
"""
import numpy as np
import pytest

import oracle_binding as oracle
import text_cases
import zone_map_model as zm
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpuscan import GpuScan
from test_ingest_gpu import make_columns
from test_zone_map_cpu import (NUMERIC_CASES, assert_chunk_equals_model, numeric_case_column,
                               short_tuple_chunk, short_tuple_model)

pytestmark = pytest.mark.gpu

NVEC = 4685
STRIDE = 512
NEEDLE_VECS = (0, 511, 512, 1535, 1536, 2047, 2048, 4095, 4096, 4607, 4608, 4684)


def ingest(src_buf, type_oids):
    """upload, transpose on the device, download: the COLUMN image"""
    runtime.init()
    ds = runtime.DeviceStore.upload(src_buf)
    try:
        col, _ = ds.to_column(type_oids)
        try:
            return col.download()
        finally:
            col.release()
    finally:
        ds.release()


def source_model(columns):
    """per column (values with 0 in NULL slots, isnull) of kds.Column inputs"""
    out = []
    for col in columns:
        isnull = (col.isnull.astype(bool) if col.isnull is not None else np.zeros(len(col), dtype=bool))
        vals = col.values.copy()
        vals[isnull] = 0
        out.append((vals, isnull))
    return out


def assert_zone_maps_equal_model_of_content(decoded, sqltypes):
    for c, (dcol, t) in enumerate(zip(decoded, sqltypes)):
        vals, isnull = zm.content(dcol, t)
        want = zm.expected(t, vals, isnull)
        assert zm.same(zm.of_decoded(dcol), want), ("column %d (%s)" % (c, t), zm.of_decoded(dcol), want)


def needle_rows(per_vec):
    """first and last row of every needle vector, first and last tail row"""
    rows = []
    for v in NEEDLE_VECS:
        rows += [v * per_vec, v * per_vec + per_vec - 1]
    rows += [NVEC * per_vec, NVEC * per_vec + per_vec - 2]
    return sorted(set(rows))


@pytest.mark.parametrize("with_nulls", [False, True])
@pytest.mark.parametrize("sqltype", ["char1", "int2", "int4", "int8", "float4", "float8"])
def test_minmax_finds_a_needle_at_every_loop_edge(sqltype, with_nulls, monkeypatch):
    """background 7, one low and one high needle per column: column k has its low needle at
    position k and its high needle at position k+1 (cyclically), so every position is proven
    for the minimum and for the maximum.  with_nulls: 10 % NULLs beside the needles, and a second
    group of columns whose only needle is the high one while the row at the NEXT position is NULL
    -- its slot holds 0, and the minimum must stay 7."""
    monkeypatch.setenv("STROM_INGEST_MAX_GRID", "2")
    attlen = kds.SQL_TYPES[sqltype][1]
    dtype = kds.SQL_TYPES[sqltype][2]
    per_vec = 16 // attlen
    n = NVEC * per_vec + per_vec - 1
    assert NVEC == 2 * 4 * STRIDE + STRIDE + 77 and NVEC > 3 * STRIDE
    rows = needle_rows(per_vec)
    assert rows[-1] == n - 1 and len(rows) == (25 if per_vec == 2 else 26)
    isflt = sqltype.startswith("float")
    rng = np.random.default_rng(attlen + 100 * with_nulls)
    columns, want = [], []
    for group in range(2 if with_nulls else 1):
        for k, at in enumerate(rows):
            nxt = rows[(k + 1) % len(rows)]
            lo, hi = (-1.5, 1e30) if isflt else (-2 - k, 100 + k)
            v = np.full(n, 7, dtype=dtype)
            isnull = None
            if with_nulls:
                isnull = rng.random(n) < 0.1
                isnull[[at, nxt]] = False
            if group == 0:
                v[at], v[nxt] = lo, hi
                want.append((dtype(lo), dtype(hi)))
            else:
                v[at] = hi
                isnull[nxt] = True
                want.append((dtype(7), dtype(hi)))
            columns.append(kds.Column(sqltype, v, isnull))
    assert len(columns) <= 64
    dec = kds.decode_column_chunk(ingest(kds.build_kds("row_flat", columns), [c.type_oid for c in columns]))
    assert_chunk_equals_model(dec, source_model(columns))
    types = [sqltype] * len(columns)
    assert_zone_maps_equal_model_of_content(dec, types)
    for c, (dcol, (lo, hi)) in enumerate(zip(dec, want)):
        if isflt:
            got = (zm.bits_double(dcol["minval"]), zm.bits_double(dcol["maxval"]))
            assert dcol["stat_flags"] == 3 and got == (float(lo), float(hi)), "column %d" % c
        else:
            assert zm.of_decoded(dcol) == (1, int(lo), int(hi)), "column %d" % c


@pytest.mark.parametrize("fmt", ["row", "row_flat", "tupslot"])
def test_transposition_strides_three_passes(fmt, monkeypatch):
    """n = 1637 under two work-groups of 256: passes of 512, 512 and 101 + 512 rows -- the last
    one holds a full wave, a wave of 37 lanes and empty waves"""
    monkeypatch.setenv("STROM_INGEST_MAX_GRID", "2")
    n = 1637
    assert n == 3 * 512 + 64 + 37
    columns = make_columns(n, 9100, 0.1)
    assert sum(c.isnull is not None for c in columns) == 4
    dec = kds.decode_column_chunk(ingest(kds.build_kds(fmt, columns), [c.type_oid for c in columns]))
    assert_chunk_equals_model(dec, source_model(columns))
    assert_zone_maps_equal_model_of_content(dec, [c.sqltype for c in columns])
    assert all(d["stat_flags"] & 1 for d in dec)


def test_default_grid_second_pass_and_four_deep_loop():
    """1 000 003 rows with the grid the device chooses: on 256 CUs the transposition takes a
    second pass (more than 2048 * 256 rows) and ingest_minmax its four-loads-in-flight loop
    (more than 3 * 256 * 256 vectors); the extremes sit in the first and the last row"""
    n = 1000003
    rng = np.random.default_rng(12)
    a = rng.integers(7, 10**6, n).astype(np.int32)
    an = rng.random(n) < 0.05
    an[[0, n - 1]] = False
    a[0], a[n - 1] = -2**31, 2**31 - 1
    b = rng.integers(-10**12, 10**12, n)
    b[0], b[n - 1] = 2**63 - 1, -2**63
    columns = [kds.Column("int4", a, an), kds.Column("int8", b)]
    dec = kds.decode_column_chunk(ingest(kds.build_kds("row_flat", columns), [23, 20]))
    assert_chunk_equals_model(dec, source_model(columns))
    assert_zone_maps_equal_model_of_content(dec, ["int4", "int8"])
    assert zm.of_decoded(dec[0]) == (1, -2**31, 2**31 - 1)
    assert zm.of_decoded(dec[1]) == (1, -2**63, 2**63 - 1)


@pytest.mark.parametrize("fmt", ["row", "row_flat"])
def test_short_tuples(fmt, monkeypatch):
    """tuples with fewer attributes than the chunk has columns (what ALTER TABLE ADD COLUMN leaves
    behind): a column past a tuple's count is NULL, for ingest and for the row reader"""
    monkeypatch.setenv("STROM_INGEST_MAX_GRID", "2")
    buf, cols, natts = short_tuple_chunk(fmt)
    model = short_tuple_model(cols, natts)
    dec = kds.decode_column_chunk(ingest(buf, [c.type_oid for c in cols]))
    assert_chunk_equals_model(dec, model)
    assert_zone_maps_equal_model_of_content(dec, [c.sqltype for c in cols])
    assert all(d["stat_flags"] & 1 for d in dec)
    qual = "(isnull (var 4 float8))"
    rc_o, res_o = oracle.gpuscan(qual, buf)
    assert np.array_equal(np.sort(res_o) - 1, np.flatnonzero(model[3][1]))
    scan = GpuScan(qual).begin()
    try:
        res = scan.scan_chunk(buf)
    finally:
        scan.end()
    assert res.errcode == rc_o == 0
    assert np.array_equal(np.sort(np.asarray(res.results)), np.sort(np.asarray(res_o)))


def test_sixty_four_columns_convert_and_sixty_five_are_refused():
    n = 300
    rng = np.random.default_rng(64)
    names = ("int4", "int2", "int8", "char1", "float8")
    columns = [kds.Column(names[i % 5], rng.integers(-100, 100, n), (rng.random(n) < 0.1) if i % 3 == 0 else None)
               for i in range(65)]
    dec = kds.decode_column_chunk(ingest(kds.build_kds("row", columns[:64]), [c.type_oid for c in columns[:64]]))
    assert len(dec) == 64
    assert_chunk_equals_model(dec, source_model(columns[:64]))
    assert_zone_maps_equal_model_of_content(dec, [c.sqltype for c in columns[:64]])
    with pytest.raises(runtime.StromError) as ei:
        ingest(kds.build_kds("row", columns), [c.type_oid for c in columns])
    assert ei.value.errcode == 101                      # StromError_BadRequestMessage, stated by the host


@pytest.mark.parametrize("fmt,coltype", [("row", "numeric_varlena"), ("row_flat", "numeric_varlena"),
                                         ("tupslot", "numeric")])
def test_numeric_integer_part_bounds_from_ingest(fmt, coltype):
    """the numeric cases of test_zone_map_cpu.py through the device: floor(min), ceil(max)"""
    for strings, flags, lo, hi in NUMERIC_CASES:
        for with_nulls in (False, True):
            col = numeric_case_column(strings, with_nulls, coltype)
            pad = kds.Column("int4", np.arange(len(col), dtype=np.int32))
            dec = kds.decode_column_chunk(ingest(kds.build_kds(fmt, [pad, col]), [23, 1700]))
            assert_chunk_equals_model(dec, source_model([pad, col]))
            assert_zone_maps_equal_model_of_content(dec, ["int4", "numeric"])
            assert zm.of_decoded(dec[1]) == (flags, lo, hi), (strings, with_nulls)


@pytest.mark.parametrize("fmt,coltype", [("row", "numeric_varlena"), ("tupslot", "numeric")])
def test_decimal_column_from_ingest_has_the_scaled_integers_zone_map(fmt, coltype):
    """numeric -> decimal_type(2): int8 at 10^-2 with an ordinary integer zone map (the cN
    operand of the integer-sum bound)"""
    n = 1637
    rng = np.random.default_rng(2)
    for lo, hi in ((700, 10494951), (-5000, 10494951), (-99999, -7)):
        scaled = rng.integers(lo, hi, n)
        isnull = rng.random(n) < 0.1
        isnull[[5, n - 1]] = False
        scaled[5], scaled[n - 1] = hi + 1, lo - 1            # the extremes; NULL slots hold 0
        src = kds.numeric_from_scaled(scaled, 2, isnull)
        dec = kds.decode_column_chunk(ingest(kds.build_kds(fmt, [kds.Column(coltype, src.values, isnull)]),
                                             [kds.decimal_type(2)]))
        want = np.where(isnull, 0, scaled)
        assert np.array_equal(dec[0]["values"], want) and np.array_equal(dec[0]["notnull"], ~isnull)
        assert_zone_maps_equal_model_of_content(dec, ["decimal"])
        assert zm.of_decoded(dec[0]) == (1, lo - 1, hi + 1)


def datum_size(buf, at):
    b0 = int(buf[at])
    if b0 & 1:
        return (b0 >> 1) & 0x7f
    return int(np.frombuffer(buf[at:at + 4].tobytes(), dtype="<u4")[0]) >> 2


def check_text_heap(image, text_cols, payloads):
    """the heap area of an ingested chunk: payloads[i] = per row bytes or None, of column text_cols[i]"""
    head = kds.KdsHead(image)
    dec = kds.decode_column_chunk(image)
    heap_start = dec[text_cols[0]]["extra_off"]
    assert heap_start > 0 and heap_start % 256 == 0
    spans = []
    for c, want in zip(text_cols, payloads):
        assert dec[c]["extra_off"] == heap_start and dec[c]["stat_flags"] == 0
        assert kds.decode_text_column(image, c) == want, "column %d payloads" % c
        offs = dec[c]["values"].view(np.uint64)
        isnull = np.array([w is None for w in want])
        if isnull.any():
            assert np.array_equal(dec[c]["notnull"], ~isnull)
        else:
            assert dec[c]["notnull"] is None
        assert not offs[isnull].any()                           # NULL: offset 0 and a clear bit
        live = offs[~isnull]
        assert (live % 4 == 0).all() and (live >= heap_start).all() and (live < head.usage).all()
        spans += [(int(at), datum_size(image, int(at))) for at in live]
    spans.sort()
    for (a0, s0), (a1, _) in zip(spans, spans[1:]):
        assert a0 + s0 <= a1, "datums overlap"
    assert head.usage == heap_start + sum((s + 3) & ~3 for _, s in spans)
    assert head.length == (head.usage + 255) & ~255
    return dec


@pytest.mark.parametrize("fmt,n,grid", [("row", 1637, "2"), ("row_flat", 1637, "2"), ("row", 50021, None)])
def test_text_heap_bytes(fmt, n, grid, monkeypatch):
    """text / character(n) datums moved by the wave allocator: every byte, every offset, and the
    chunk's 'usage' / 'length' book-keeping"""
    if grid:
        monkeypatch.setenv("STROM_INGEST_MAX_GRID", grid)
    buf, txt, chr10, num, tnull = text_cases.text_table(n, 77 + n, fmt)
    image = ingest(buf, [23, 25, 1042, 20])
    want_txt = [None if tnull[i] else bytes(txt[i]) for i in range(n)]
    dec = check_text_heap(image, [1, 2], [want_txt, [bytes(c) for c in chr10]])
    assert np.array_equal(dec[0]["values"], num) and np.array_equal(dec[3]["values"], np.arange(n))
    assert_zone_maps_equal_model_of_content([dec[0], dec[3]], ["int4", "int8"])


def test_all_null_text_column_takes_no_heap(monkeypatch):
    """no wave has a byte to place: no atomic on 'usage', which stays at the heap's start"""
    monkeypatch.setenv("STROM_INGEST_MAX_GRID", "2")
    n = 1637
    words = [text_cases.WORDS[i % len(text_cases.WORDS)] for i in range(n)]
    columns = [kds.Column("int4", np.arange(n)), kds.Column("text", words, np.ones(n, dtype=bool))]
    image = ingest(kds.build_kds("row", columns), [23, 25])
    check_text_heap(image, [1], [[None] * n])
    head = kds.KdsHead(image)
    assert head.usage == kds.decode_column_chunk(image)[1]["extra_off"] == head.length


def test_join_projection_zone_maps(monkeypatch):
    """the second launch site of ingest_minmax (strom_hashjoin_project_column), two work-groups:
    more than 20 000 joined rows, so that the int4 column's four-deep loop runs; an outer int4
    column and an inner int8 column with NULLs whose live values are all >= 7"""
    monkeypatch.setenv("STROM_INGEST_MAX_GRID", "2")
    runtime.init()
    n, nd = 30011, 3000
    rng = np.random.default_rng(81)
    fk = rng.integers(0, int(nd * 1.2), n).astype(np.int32)
    a = rng.integers(-1000, 1000, n).astype(np.int32)
    hit = np.flatnonzero(fk < nd)
    a[hit[0]], a[hit[-1]] = -2**31, 2**31 - 1
    fact = kds.build_kds("column", [kds.Column("int4", fk), kds.Column("int4", a)])
    dkey = rng.permutation(nd).astype(np.int32)
    dpay = rng.integers(7, 10**12, nd)
    dpn = rng.random(nd) < 0.1
    used = np.zeros(nd, dtype=bool)
    used[fk[hit]] = True
    live = np.flatnonzero(~dpn & used[dkey])
    dpay[live[0]] = 2**63 - 1
    inner = kds.build_kds("row", [kds.Column("int4", dkey), kds.Column("int8", dpay, dpn)])
    ds = runtime.DeviceStore.upload(fact)
    join = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(build_multihash([(inner, [1])]))
    try:
        joined, nitems = join.join_to_column(ds, [(0, 2, "int4"), (1, 2, "int8")])
        try:
            dec = kds.decode_column_chunk(joined.download())
        finally:
            joined.release()
    finally:
        join.end()
        ds.release()
    assert nitems == len(hit) and nitems >= 20000 and nitems // 4 > 3 * STRIDE
    pos = np.empty(nd, dtype=np.int64)
    pos[dkey] = np.arange(nd)
    irow = pos[fk[hit]]
    want = np.stack([a[hit].astype(np.int64), np.where(dpn[irow], 0, dpay[irow]), dpn[irow].astype(np.int64)], axis=1)
    nn = dec[1]["notnull"]
    assert dec[0]["notnull"] is None and nn is not None
    got = np.stack([dec[0]["values"].astype(np.int64), dec[1]["values"].astype(np.int64), (~nn).astype(np.int64)], axis=1)
    assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])
    assert_zone_maps_equal_model_of_content(dec, ["int4", "int8"])
    assert zm.of_decoded(dec[0]) == (1, -2**31, 2**31 - 1)
    assert zm.of_decoded(dec[1]) == (1, int(dpay[irow][~dpn[irow]].min()), 2**63 - 1)
    assert dec[1]["minval"] >= 7
