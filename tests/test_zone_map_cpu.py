"""
Zone maps of the host builder (column_minmax, csrc/datastore.cpp) against the independent model
of tests/zone_map_model.py, at the edges where a bound goes wrong: type extremes, NULL slots
that hold values outside the live range, float specials, and the numeric integer-part bounds
(floor(min), ceil(max): KDS_COLSTAT_INTPART, include/strom_kds.h).  And heap chunks whose
tuples carry fewer attributes than the chunk has columns, through the host's readers.
CPU only: no device call.
"""
from decimal import Decimal

import numpy as np
import pytest

import oracle_binding as oracle
import zone_map_model as zm
from pg_strom_amd import kds

INT_RANGE = {"char1": (-2**7, 2**7 - 1), "int2": (-2**15, 2**15 - 1),
             "int4": (-2**31, 2**31 - 1), "int8": (-2**63, 2**63 - 1)}


def host_zone_map(column):
    return zm.of_decoded(kds.decode_column_chunk(kds.build_kds("column", [column]))[0])


def check_host(sqltype, values, isnull=None):
    np_values = np.asarray(values, dtype=kds.SQL_TYPES[sqltype][2])
    got = host_zone_map(kds.Column(sqltype, np_values, isnull))
    want = zm.expected(sqltype, list(np_values), isnull)
    assert zm.same(got, want), (sqltype, got, want)
    return got


@pytest.mark.parametrize("sqltype", sorted(INT_RANGE))
def test_integer_extremes(sqltype):
    lo, hi = INT_RANGE[sqltype]
    assert check_host(sqltype, [lo, hi]) == (1, lo, hi)
    assert check_host(sqltype, [hi, lo, 0, -1, 1]) == (1, lo, hi)
    assert check_host(sqltype, [lo]) == (1, lo, lo)
    assert check_host(sqltype, [hi]) == (1, hi, hi)
    assert check_host(sqltype, [hi, hi - 1]) == (1, hi - 1, hi)
    assert check_host(sqltype, [lo + 1, lo]) == (1, lo, lo + 1)
    # an extreme in a NULL slot does not count
    assert check_host(sqltype, [lo, 3, hi, 5], [1, 0, 1, 0]) == (1, 3, 5)
    assert check_host(sqltype, [lo, hi], [1, 1]) == (0, 0, 0)


@pytest.mark.parametrize("sqltype", sorted(INT_RANGE) + ["float4", "float8"])
def test_null_slots_do_not_reach_the_bounds(sqltype):
    """every live value is >= 7; the NULL slots hold 0 and values on both sides"""
    rng = np.random.default_rng(5)
    n = 1000
    v = rng.integers(7, 100, n)
    isnull = rng.random(n) < 0.3
    v[isnull] = rng.integers(-100, 127, int(isnull.sum()))
    v[np.flatnonzero(isnull)[:3]] = 0
    got = check_host(sqltype, v, isnull)
    live_min, live_max = int(v[~isnull].min()), int(v[~isnull].max())
    assert live_min >= 7
    if sqltype.startswith("float"):
        assert (zm.bits_double(got[1]), zm.bits_double(got[2])) == (float(live_min), float(live_max))
    else:
        assert got == (1, live_min, live_max)


@pytest.mark.parametrize("sqltype", ["float4", "float8"])
def test_float_specials(sqltype):
    inf, nan = float("inf"), float("nan")
    big = 3.0e38 if sqltype == "float4" else 1.7e308
    tiny = 1e-45 if sqltype == "float4" else 5e-324          # the smallest denormal
    got = check_host(sqltype, [1.0, -inf, inf, 2.0])
    assert (zm.bits_double(got[1]), zm.bits_double(got[2])) == (-inf, inf)
    got = check_host(sqltype, [nan, 1.5, nan, -2.5, nan])
    assert (zm.bits_double(got[1]), zm.bits_double(got[2])) == (-2.5, 1.5)
    assert check_host(sqltype, [nan, nan, nan]) == (0, 0, 0)
    assert check_host(sqltype, [nan, 4.0], [0, 1]) == (0, 0, 0)
    got = check_host(sqltype, [nan, inf])
    assert (zm.bits_double(got[1]), zm.bits_double(got[2])) == (inf, inf)
    for zeros in ([0.0, -0.0], [-0.0, 0.0], [-0.0], [0.0], [-0.0, 3.0], [-3.0, -0.0, 0.0]):
        got = check_host(sqltype, zeros)
        assert got[0] == 3
    check_host(sqltype, [big, -big, tiny, -tiny])
    check_host(sqltype, [tiny, big])
    check_host(sqltype, [-big, -tiny])
    check_host(sqltype, [-inf, nan, -1.0, 7.0], [1, 0, 0, 0])


# (values, flags, minval, maxval): section "Numeric" of the zone-map contract
NUMERIC_CASES = [
    (["0.5", "2.25", "7.75"], 4, 0, 8),
    (["-0.5", "-2.25", "-7.75"], 4, -8, 0),
    (["0"], 4, 0, 0),
    (["1E-25"], 4, 0, 1),
    (["-1E-25"], 4, -1, 0),
    (["3", "-12", "1000000", "0", "144115188075855871"], 4, -12, 144115188075855871),
    (["-5", "-4"], 4, -5, -4),
    (["2.5", "1E+20", "-1"], 0, 0, 0),
    (["-1E+20"], 0, 0, 0),
    (["9E+18", "-9E+18", "0.1"], 4, -9 * 10**18, 9 * 10**18),
    (["-0.07", "104949.50", "-99.01", "12345678.999"], 4, -100, 12345679),
]


def numeric_case_column(strings, with_nulls, coltype="numeric"):
    """the case's values as a numeric column; with_nulls: NULL rows in between whose slots hold
    images far outside the live range"""
    imgs = [kds.numeric_encode(Decimal(s)) for s in strings]
    isnull = None
    if with_nulls:
        noise = [kds.numeric_encode(Decimal(s)) for s in ("-123456.5", "1E+25", "98765.25")]
        imgs = [noise[0]] + imgs[:1] + [noise[1]] + imgs[1:] + [noise[2]]
        isnull = np.zeros(len(imgs), dtype=bool)
        isnull[[0, 2, len(imgs) - 1]] = True
    assert None not in imgs
    return kds.Column(coltype, np.array(imgs, dtype=np.uint64), isnull)


@pytest.mark.parametrize("with_nulls", [False, True])
@pytest.mark.parametrize("case", range(len(NUMERIC_CASES)))
def test_numeric_integer_part_bounds(case, with_nulls):
    strings, flags, lo, hi = NUMERIC_CASES[case]
    want = zm.expected("numeric", [Decimal(s) for s in strings])
    assert want == (flags, lo, hi)                      # the model states what the contract lists
    col = numeric_case_column(strings, with_nulls)
    got = host_zone_map(col)
    assert got == want, (strings, got, want)
    # and the model reads the same from the column's own images
    live = [zm.numeric_image_value(x) for i, x in enumerate(col.values)
            if col.isnull is None or not col.isnull[i]]
    assert zm.expected("numeric", live) == want
    if flags:
        assert all(abs(Decimal(s)) <= max(abs(got[1]), abs(got[2])) for s in strings)


def test_numeric_all_null_column_has_no_bounds():
    col = kds.Column("numeric", np.array([kds.numeric_encode("5.5")] * 3, dtype=np.uint64), np.ones(3, dtype=bool))
    assert host_zone_map(col) == (0, 0, 0) == zm.expected("numeric", [Decimal("5.5")] * 3, [1, 1, 1])


# ---------------------------------------------------------------------
# heap tuples with fewer attributes than the chunk has columns
# ---------------------------------------------------------------------
def short_tuple_chunk(fmt, n=1637, seed=41):
    """(chunk, columns, natts): int4, int8 (with NULLs), int2, float8; every third tuple cut to
    1..3 attributes.  The model: a column past a tuple's attribute count is NULL."""
    rng = np.random.default_rng(seed)
    cols = [kds.Column("int4", rng.integers(-2**31, 2**31, n)),
            kds.Column("int8", rng.integers(-2**62, 2**62, n), rng.random(n) < 0.2),
            kds.Column("int2", rng.integers(-30000, 30000, n)),
            kds.Column("float8", rng.normal(size=n) * 100)]
    buf = kds.build_kds(fmt, cols)
    natts = np.full(n, 4)
    rows = np.arange(0, n, 3)
    natts[rows] = 1 + (np.arange(len(rows)) % 3)
    zm.shorten_tuples(buf, rows, natts[rows])
    return buf, cols, natts


def short_tuple_model(cols, natts):
    """per column (values with 0 in NULL slots, isnull)"""
    out = []
    for c, col in enumerate(cols):
        isnull = (natts <= c)
        if col.isnull is not None:
            isnull = isnull | col.isnull.astype(bool)
        vals = col.values.copy()
        vals[isnull] = 0
        out.append((vals, isnull))
    return out


def assert_chunk_equals_model(decoded, model):
    for c, (dcol, (vals, isnull)) in enumerate(zip(decoded, model)):
        if isnull.any():
            assert dcol["notnull"] is not None and np.array_equal(dcol["notnull"], ~isnull), "column %d NULLs" % c
        else:
            assert dcol["notnull"] is None or dcol["notnull"].all(), "column %d NULLs" % c
        assert np.array_equal(dcol["values"], vals.view(dcol["values"].dtype)), "column %d values" % c


@pytest.mark.parametrize("fmt", ["row", "row_flat"])
def test_tuple_offsets_find_every_tuple(fmt):
    """the first column's value sits t_hoff bytes into each tuple (no NULL in these rows)"""
    n = 1000
    a = np.random.default_rng(1).integers(-2**31, 2**31, n).astype(np.int32)
    buf = kds.build_kds(fmt, [kds.Column("int4", a), kds.Column("int8", np.arange(n))])
    offs = zm.tuple_offsets(buf)
    assert len(offs) == n and len(set(offs)) == n
    for r in (0, 1, 184, 185, 186, 511, n - 1):
        at = offs[r] + int(buf[offs[r] + 22])
        assert int(np.frombuffer(buf[at:at + 4].tobytes(), dtype="<i4")[0]) == int(a[r])
        assert (int(buf[offs[r] + 18]) | (int(buf[offs[r] + 19]) << 8)) & 0x07ff == 2


@pytest.mark.parametrize("fmt", ["row", "row_flat"])
def test_short_tuples_through_the_host_readers(fmt):
    buf, cols, natts = short_tuple_chunk(fmt)
    model = short_tuple_model(cols, natts)
    n = len(natts)
    assert (natts < 4).sum() > 500 and {1, 2, 3, 4} == set(natts.tolist())
    # strom_kds_to_column: values and NULLs
    assert_chunk_equals_model(kds.decode_column_chunk(kds.kds_to_column(buf)), model)
    # strom_kds_fetch and the oracle's row reader agree with the model, cell by cell
    for c, (vals, isnull) in enumerate(model):
        sqltype = cols[c].sqltype
        oid, v, isn, err = oracle.eval_rows("(var %d %s)" % (c + 1, sqltype), buf)
        assert not err.any() and np.array_equal(isn, isnull), "column %d oracle NULLs" % c
        mask = (1 << (8 * cols[c].attlen)) - 1
        raw = vals.view("<i%d" % cols[c].attlen).astype(np.int64).view(np.uint64) & np.uint64(mask)
        assert np.array_equal(v[~isnull] & np.uint64(mask), raw[~isnull]), "column %d oracle values" % c
        for r in list(range(0, 40)) + [n - 2, n - 1]:
            fnull, image = kds.kds_fetch(buf, r, c)
            assert fnull == bool(isnull[r])
            if not fnull:
                assert (image & mask) == int(raw[r])
