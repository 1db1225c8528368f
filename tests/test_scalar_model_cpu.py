"""
The scalar device functions against an independent model, without a GPU.

tests/scalar_model.py states what every catalog entry flagged DEVFUNC_NEEDS_MATHLIB or
DEVFUNC_NEEDS_TIMELIB returns, from the reference's sources.  Here:
  * completeness  -- the catalog (strom_codegen_catalog_entry) and the model's rules cover each other,
    so a function added later without a rule fails this suite;
  * anchors       -- hand-derived cases that keep the model from floating free;
  * model = oracle -- every function over its full edge grid through oracle.eval_rows: value,
    nullness and error flag agree exactly (floats by bit pattern);
  * the chunks and CASE expressions the GPU tests use give the same outcomes through the oracle's
    GpuScan and GpuPreAgg, so what is left to the device is the device.
"""
import numpy as np
import pytest

import oracle_binding as oracle
import scalar_cases as cases
import scalar_model as model
from pg_strom_amd import kds

NB, NE = model.DATE_NOBEGIN, model.DATE_NOEND
TNB, TNE = model.TS_NOBEGIN, model.TS_NOEND
DAY = model.USECS_PER_DAY
JD0 = -model.POSTGRES_EPOCH_JDATE            # Julian day 0 as a date
I2, I4, I8, F4, F8 = "int2", "int4", "int8", "float4", "float8"
DT, TM, TS = "date", "time", "timestamp"
f4, f8 = np.float32, np.float64
RECHECK, NULL = "recheck", "null"


def test_catalog_listing_is_bounded_and_stable():
    from pg_strom_amd._lib import lib
    n = lib.strom_codegen_catalog_count()
    assert n > 300 and lib.strom_codegen_catalog_count() == n
    assert lib.strom_codegen_catalog_entry(-1, None, None, None, None) == -1
    assert lib.strom_codegen_catalog_entry(n, None, None, None, None) == -1
    assert lib.strom_codegen_catalog_entry(0, None, None, None, None) == 1       # int2(int4): out pointers may be NULL
    entries = cases.catalog()
    assert len(entries) == n and len(set(e[:2] for e in entries)) == n           # (name, argument types) is the key
    assert ("pi", (), 701, model.DEVFUNC_NEEDS_MATHLIB) in entries
    assert ("date_pli", (1082, 23), 1082, model.DEVFUNC_NEEDS_TIMELIB) in entries


def test_model_and_catalog_cover_each_other():
    """every in-scope catalog entry has a model rule of the same return type, and every rule names
    a catalog entry"""
    funcs = cases.in_scope_functions()
    assert len(funcs) > 250
    missing = [f for f in funcs if (f[0], f[1]) not in model.RULES]
    assert not missing, "catalog entries without a model rule: %r" % (missing,)
    wrong = [f for f in funcs if model.return_type(f[0], f[1]) != f[2]]
    assert not wrong, "return types differ: %r" % (wrong,)
    known = set((f[0], f[1]) for f in funcs)
    orphans = [k for k in model.RULES if k not in known]
    assert not orphans, "model rules without a catalog entry: %r" % (orphans,)
    # nothing in scope is a transcendental, numeric or text function
    all_names = set(e[0] for e in cases.catalog())
    assert model.OUT_OF_SCOPE <= all_names


# (function, argument types, arguments) -> value | NULL | RECHECK, each derived by hand from the
# line it cites (opencl_mathlib.h = M, opencl_timelib.h = T, codegen.c = C, opencl_common.h = K;
# "policy": the recheck-instead-of-wrap rule of strom_mathlib.h / strom_timelib.h)
ANCHORS = [
    # infinite dates: T:335-336, 353-354 "can't change infinity"; T:397-401 swaps the arguments
    ("date_pli", (DT, I4), (NE, -1), NE),
    ("date_pli", (DT, I4), (NB, 2147483647), NB),
    ("date_mii", (DT, I4), (NB, -5), NB),
    ("date_mii", (DT, I4), (NE, 1), NE),
    ("integer_pl_date", (I4, DT), (7, NE), NE),
    ("integer_pl_date", (I4, DT), (-7, NB), NB),
    # finite dates: T:338, 356; the sum leaving int4 wraps there -- policy
    ("date_pli", (DT, I4), (NE - 1, 1), NE),                # fits int4: the reference's sum, T:338
    ("date_pli", (DT, I4), (NE - 1, 2), RECHECK),
    ("date_pli", (DT, I4), (NE - 2, 1), NE - 1),
    ("date_mii", (DT, I4), (NB + 1, 2), RECHECK),
    ("date_mii", (DT, I4), (10, 3), 7),
    # T:368-372: an infinite operand goes back to the CPU
    ("date_mi", (DT, DT), (NE, 0), RECHECK),
    ("date_mi", (DT, DT), (0, NB), RECHECK),
    ("date_mi", (DT, DT), (NE, NE), RECHECK),
    ("date_mi", (DT, DT), (NE - 1, -2), RECHECK),           # T:376 wraps -- policy
    ("date_mi", (DT, DT), (5, -5), 10),
    # date(timestamp): T:204-209 (timestamp2tm fails below Julian day 0), 236-250
    ("date", (TS,), (JD0 * DAY - 1,), RECHECK),
    ("date", (TS,), (JD0 * DAY,), JD0),
    ("date", (TS,), (-1,), -1),                             # T:199-203: floor, not truncation
    ("date", (TS,), (DAY - 1,), 0),
    ("date", (TS,), (TNB,), NB),
    ("date", (TS,), (TNE,), NE),
    ("date", (TS,), (TNE - 1,), 106751991),                 # (2^63 - 2) // 86400000000
    ("date", (TS,), (TNB + 1,), RECHECK),                   # day -106751992, far below Julian day 0
    # time(timestamp): T:269-270 NULL and no error for an infinite timestamp; 271-275; 279-283
    ("time", (TS,), (TNE,), NULL),
    ("time", (TS,), (TNB,), NULL),
    ("time", (TS,), (-1,), DAY - 1),
    ("time", (TS,), (JD0 * DAY - 1,), RECHECK),
    ("time", (TS,), (JD0 * DAY,), 0),
    # timestamp(date): T:297-306 infinities map; 311-317 overflow test
    ("timestamp", (DT,), (NE,), TNE),
    ("timestamp", (DT,), (NB,), TNB),
    ("timestamp", (DT,), (106751991,), 106751991 * DAY),
    ("timestamp", (DT,), (106751992,), RECHECK),
    ("timestamp", (DT,), (-106751991,), -106751991 * DAY),
    ("timestamp", (DT,), (-106751992,), RECHECK),
    # datetime_pl: T:390-392; the sum wrapping is policy
    ("datetime_pl", (DT, TM), (NE, 5), TNE),
    ("datetime_pl", (DT, TM), (1, 5), DAY + 5),
    ("datetime_pl", (DT, TM), (106751991, DAY), RECHECK),
    ("datetime_pl", (DT, TM), (106751992, None), NULL),     # strict first: no recheck
    ("timedate_pl", (TM, DT), (7, -1), -DAY + 7),
    # date against timestamp: T:417-426 ..., the promoted date compared raw
    ("date_eq_timestamp", (DT, TS), (NE, TNE), 1),
    ("date_lt_timestamp", (DT, TS), (1, DAY + 1), 1),
    ("date_lt_timestamp", (DT, TS), (106751992, 0), RECHECK),
    ("date_lt_timestamp", (DT, TS), (106751992, None), NULL),
    ("timestamp_ge_date", (TS, DT), (TNB, NB), 1),
    ("timestamp_cmp_date", (TS, DT), (TNE - 1, NE), -1),
    ("date_cmp_timestamp", (DT, TS), (NB, TNB + 1), -1),
    # integer division and remainder: M:455-468 (zero, MIN / -1), 476-492, 787-808
    ("int4div", (I4, I4), (-2**31, -1), RECHECK),
    ("int4div", (I4, I4), (-2**31 + 1, -1), 2**31 - 1),
    ("int4div", (I4, I4), (7, 0), RECHECK),
    ("int4div", (I4, I4), (-7, 2), -3),                     # truncation towards zero
    ("int24div", (I2, I4), (-32768, -1), 32768),            # an int4 result: fits
    ("int42div", (I4, I2), (-2**31, -1), RECHECK),
    ("int2div", (I2, I2), (-32768, -1), RECHECK),
    ("int8div", (I8, I8), (-2**63, -1), RECHECK),
    ("int2mod", (I2, I2), (-32768, -1), 0),                 # M:802-803
    ("int4mod", (I4, I4), (-7, 2), -1),                     # sign of the dividend
    ("int8mod", (I8, I8), (1, 0), RECHECK),
    # add / subtract / multiply: M:45-50, 111-116, 176-181
    ("int8mul", (I8, I8), (2**32, 2**31), RECHECK),
    ("int8mul", (I8, I8), (-2**32, 2**31), -2**63),
    ("int8mul", (I8, I8), (-2**63, -1), RECHECK),
    ("int2pl", (I2, I2), (32767, 1), RECHECK),
    ("int24pl", (I2, I4), (32767, 1), 32768),
    ("int4mi", (I4, I4), (-2**31, 1), RECHECK),
    ("int84mi", (I8, I4), (-2**63 + 1, 1), -2**63),
    # unary: C:312-321 wrap at MIN -- policy
    ("int4abs", (I4,), (-2**31,), RECHECK),
    ("abs", (I8,), (-2**63,), RECHECK),
    ("int2um", (I2,), (-32768,), RECHECK),
    ("int2um", (I2,), (32767,), -32767),
    ("int4not", (I4,), (-1,), 0),
    # shifts: C:436-443, the count modulo the promoted width; C:682 casts the result back
    ("int2shl", (I2, I4), (1, 16), 0),                      # 65536 as int2
    ("int2shl", (I2, I4), (1, 15), -32768),
    ("int2shl", (I2, I4), (1, 32), 1),                      # count & 31
    ("int4shl", (I4, I4), (1, 33), 2),
    ("int4shl", (I4, I4), (1, 31), -2**31),
    ("int8shl", (I8, I4), (1, 64), 1),                      # count & 63
    ("int8shl", (I8, I4), (3, 63), -2**63),
    ("int8shr", (I8, I4), (-2**63, 63), -1),                # arithmetic
    ("int4shr", (I4, I4), (-8, -1), -1),                    # count 31
    # casts: C:650 is a bare cast; rint and the range check are policy (dtoi4, dtoi8, dtof, i8toi4)
    ("int4", (F8,), (f8(2147483647.5),), RECHECK),          # rint gives 2147483648
    ("int4", (F8,), (f8(2147483647.4999),), 2147483647),
    ("int4", (F8,), (f8(-2147483648.5),), -2**31),          # half to even
    ("int4", (F8,), (f8(2.5),), 2),
    ("int4", (F8,), (f8(3.5),), 4),
    ("int4", (F8,), (f8(np.nan),), RECHECK),
    ("int2", (F8,), (f8(32767.5),), RECHECK),
    ("int2", (F4,), (f4(-32768.5),), -32768),
    ("int8", (F8,), (f8(2.0**63),), RECHECK),
    ("int8", (F8,), (f8(-2.0**63),), -2**63),
    ("int8", (F8,), (np.nextafter(f8(2.0**63), f8(0)),), 2**63 - 1024),
    ("int8", (F4,), (f4(2.0**63),), RECHECK),
    ("int2", (I4,), (32768,), RECHECK),
    ("int4", (I8,), (-2**31 - 1,), RECHECK),
    ("int4", (I8,), (-2**31,), -2**31),
    ("float4", (F8,), (f8(1e-50),), RECHECK),               # underflow to zero
    ("float4", (F8,), (f8(1e39),), RECHECK),                # overflow to infinity
    ("float4", (F8,), (f8(np.inf),), f4(np.inf)),
    ("float4", (F8,), (f8(2.0**-150),), RECHECK),           # the tie rounds to even: zero
    ("float4", (F8,), (np.nextafter(f8(2.0**-150), f8(1)),), f4(2.0**-149)),
    ("float4", (I8,), (2**63 - 1,), f4(2.0**63)),
    ("float4", (I4,), (16777217,), f4(16777216.0)),         # 2^24 + 1: the tie goes to even
    ("float8", (I8,), (2**53 + 1,), f8(2.0**53)),
    ("int4", ("bool",), (1,), 1),
    # float arithmetic: CHECKFLOATVAL M:25-27 as used at M:66-72, 358-377, 680-694
    ("float8mul", (F8, F8), (f8(1e200), f8(1e200)), RECHECK),
    ("float8mul", (F8, F8), (f8(1e-200), f8(1e-200)), RECHECK),
    ("float8mul", (F8, F8), (f8(0.0), f8(-1.0)), f8(-0.0)),
    ("float8mul", (F8, F8), (f8(np.inf), f8(0.0)), f8(np.nan)),
    ("float8mul", (F8, F8), (f8(2.0**-537), f8(2.0**-537)), f8(2.0**-1074)),
    ("float4mul", (F4, F4), (f4(2.0**-75), f4(2.0**-74)), f4(2.0**-149)),
    ("float4mul", (F4, F4), (f4(2.0**-75), f4(2.0**-75)), RECHECK),
    ("float8div", (F8, F8), (f8(1.0), f8(-0.0)), RECHECK),
    ("float8div", (F8, F8), (f8(1.0), f8(np.inf)), RECHECK),        # M:688-690: zero is valid only for a zero dividend
    ("float8div", (F8, F8), (f8(0.0), f8(np.inf)), f8(0.0)),
    ("float8pl", (F8, F8), (np.finfo(f8).max, np.finfo(f8).max), RECHECK),
    ("float48pl", (F4, F8), (f4(0.1), f8(0.0)), f8(f4(0.1))),
    # comparisons
    ("btfloat8cmp", (F8, F8), (f8(np.nan), f8(np.inf)), 1),         # K:1553-1560
    ("btfloat8cmp", (F8, F8), (f8(np.nan), f8(np.nan)), 0),
    ("btfloat48cmp", (F4, F8), (f4(0.1), f8(0.1)), 1),              # 0.1f is above 0.1
    ("float8eq", (F8, F8), (f8(0.0), f8(-0.0)), 1),
    ("float8gt", (F8, F8), (f8(np.nan), f8(np.inf)), 1),            # PostgreSQL's order (see the rule)
    ("int48lt", (I4, I8), (-2**31, -2**31 - 1), 0),
    ("btint28cmp", (I2, I8), (-32768, -2**63), 1),                  # K:1550-1551
    ("bpcharlt", ("char1", "char1"), (0x20, 1), 1),                 # the blank is the empty string
    ("bpchargt", ("char1", "char1"), (-1, 0x7f), 1),                # 0xff above 0x7f: unsigned
    # float8 functions: C:471-490
    ("round", (F8,), (f8(2.5),), f8(2.0)),
    ("round", (F8,), (f8(-0.5),), f8(-0.0)),
    ("ceil", (F8,), (f8(-0.5),), f8(-0.0)),
    ("trunc", (F8,), (f8(-1.5),), f8(-1.0)),
    ("sqrt", (F8,), (f8(-1.0),), RECHECK),
    ("sqrt", (F8,), (f8(-0.0),), f8(-0.0)),
    ("sqrt", (F8,), (f8(2.0),), f8(1.4142135623730951)),
    ("sign", (F8,), (f8(np.nan),), f8(0.0)),
    ("int8pl", (I8, I8), (None, 2**63 - 1), NULL),
]


def test_anchor_table_is_what_the_issue_asks_for():
    assert len(ANCHORS) >= 60
    assert len(set((a[0], a[1], repr(a[2])) for a in ANCHORS)) == len(ANCHORS)


@pytest.mark.parametrize("i", range(len(ANCHORS)), ids=["%s-%d" % (a[0], i) for i, a in enumerate(ANCHORS)])
def test_model_anchor(i):
    name, argtypes, args, want = ANCHORS[i]
    value, isnull, recheck = model.evaluate(name, argtypes, args)
    if want is RECHECK:
        assert (isnull, recheck) == (True, True)
    elif want is NULL:
        assert (isnull, recheck) == (True, False)
    else:
        assert (isnull, recheck) == (False, False)
        rettype = model.return_type(name, argtypes)
        assert model.same_value((name, argtypes), rettype, want, model.value_image(rettype, value)), value


def test_grids_hold_what_they_must():
    g8 = model.grid("int8")
    for v in (-2**63, -2**63 + 1, -2, -1, 0, 1, 2, 2**63 - 2, 2**63 - 1, 32767, -32767, 32768, -32768,
              32769, -32769, 2**31 - 1, -2**31 + 1, 2**31, -2**31, 2**31 + 1, -2**31 - 1, None):
        assert v in g8
    assert model.SHIFT_COUNTS == [-1, 0, 1, 15, 16, 31, 32, 33, 63, 64, 65]
    assert model.LAST_TS_DAY == 106751991 and model.LAST_TS_DAY * DAY <= 2**63 - 1 < (model.LAST_TS_DAY + 1) * DAY
    for v in (NB, NB + 1, NE - 1, NE, -2451546, -2451545, -2451544, -106751992, -106751991, -106751990,
              106751990, 106751991, 106751992, -1, 0, 1, None):
        assert v in model.grid("date")
    for k in (-2451546, -2451545, -1, 0, 1):
        for d in (-1, 0, 1):
            assert k * DAY + d in model.grid("timestamp")
    for v in (TNB, TNB + 1, TNE - 1, TNE, None):
        assert v in model.grid("timestamp")
    assert model.grid("time") == [0, 1, DAY - 1, DAY, None]
    u8 = [v for v in model.grid("float8", "unary") if v is not None]
    for v in (2147483647.5, 2147483648.0, 2147483646.5, -2147483648.5, 32767.5, -32768.5, 2.0**63,
              float(np.nextafter(f8(2.0**63), f8(0))), 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
              2.5, -2.5, 1e-50, float(np.finfo(f4).max)):
        assert any(float(x) == v for x in u8), v
    assert sum(1 for x in u8 if np.isnan(x)) == 1 and any(x == 0 and np.signbit(x) for x in u8)
    # a unary function gets its whole grid, a binary one the cross product, below about 1500 rows
    assert max(len(model.rows(n, a)) for n, a in model.RULES) < 1500


def _function_chunk(argtypes, rows):
    cols = []
    for i, t in enumerate(argtypes):
        dtype = kds.SQL_TYPES[t][2]
        vals = np.array([1 if r[i] is None else r[i] for r in rows], dtype=dtype)
        cols.append(kds.Column(t, vals, np.array([r[i] is None for r in rows], dtype=np.uint8)))
    if not cols:
        cols = [kds.Column("int4", np.zeros(len(rows), dtype=np.int32))]
    return kds.build_kds("column", cols)


def test_model_agrees_with_oracle_on_every_function_and_row():
    """value, nullness and error flag of every in-scope function over its full grid: the oracle
    (oracle.eval_rows) against the model, exactly"""
    bad, nrows = [], 0
    for name, argtypes, rettype in cases.in_scope_functions():
        rows = model.rows(name, argtypes)
        buf = _function_chunk(argtypes, rows)
        expr = "(%s%s)" % (name, "".join(" (var %d %s)" % (i + 1, t) for i, t in enumerate(argtypes)))
        oid, values, isnull, err = oracle.eval_rows(expr, buf)
        assert oid == model.OIDS[rettype], (name, oid)
        for r, row in enumerate(rows):
            value, want_null, want_recheck = model.evaluate(name, argtypes, row)
            what = "%s(%s)" % (name, ", ".join("NULL" if a is None else repr(a) for a in row))
            if (err[r] != 0) != want_recheck or (want_recheck and err[r] != 2):
                bad.append("%s: error %d, model recheck %s" % (what, err[r], want_recheck))
            elif bool(isnull[r]) != want_null:
                bad.append("%s: NULL %s, model %s" % (what, bool(isnull[r]), want_null))
            elif not want_null and not model.same_value((name, argtypes), rettype, value, int(values[r])):
                bad.append("%s: 0x%x, model %r" % (what, int(values[r]), value))
        nrows += len(rows)
    assert nrows > 50000
    assert not bad, "%d rows differ, first: %s" % (len(bad), "; ".join(bad[:12]))


@pytest.mark.parametrize("rettype", cases.RETURN_TYPES)
def test_case_programs_give_the_model_through_the_oracle(rettype):
    """the chunk and the CASE expressions of test_scalar_model_gpu.py, evaluated by the oracle's
    GpuScan and GpuPreAgg: recheck set, passing set and values are the model's"""
    case = cases.return_type_case(rettype)
    assert case.functions
    for ids in case.groups():
        expr = case.case_expr(ids)
        mine = case.rows_of(ids)
        rc, res = oracle.gpuscan("(isnotnull %s)" % expr, case.buf)
        want_recheck = mine[case.recheck[mine]]
        want_pass = mine[~case.isnull[mine]]
        assert np.array_equal(np.sort(-res[res < 0] - 1), want_recheck)
        assert np.array_equal(np.sort(res[res > 0] - 1), want_pass)
        ok = mine[~case.recheck[mine]]
        rc, v, isn = oracle.gpupreagg("(gpupreagg (key (var 1 int4)) (pmax %s))" % case.carried_expr(ids), case.buf, 2,
                                      row_map=ok.astype(np.int32), max_groups=len(ok) + 1)
        assert rc == 0 and len(v) == len(ok)
        order = np.argsort(v[:, 0].astype(np.int64))
        assert np.array_equal(v[order, 0].astype(np.int64), ok)
        bad = case.check_values(ok, v[order, 1], isn[order, 1])
        assert not bad, "%d rows differ, first: %s" % (len(bad), "; ".join(bad[:8]))
