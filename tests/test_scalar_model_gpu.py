"""
The scalar device functions (strom_mathlib.h, strom_timelib.h) on the device against the
independent model of tests/scalar_model.py (needs an MI355X: -m gpu).

Every pair of an in-scope function and a row of its edge grid is checked for all three outcomes:
the recheck flag, nullness, the value.  The construction is tests/scalar_cases.py's: one COLUMN
chunk per return type, one CASE expression per group of functions, so a program serves some
thirty functions and a row evaluates its own function only.
  * recheck / NULL  GpuScan on (isnotnull E): the rows sent back are the model's recheck rows, the
                    rows that pass are the model's error-free non-NULL rows.
  * values          GpuPreAgg keyed by the row number with (pmax E), fed the model's error-free rows
                    only through a row map; the fold's status must be clean, so a recheck the
                    model does not know cannot hide.  One row per group: pmax is the value itself.
                    pmax carries out every return type as it is but two: bool goes through the
                    widening cast int4(bool), float4 through float8(float4) -- exact, and in-scope
                    functions themselves, checked directly by the int4 and float8 cases.
Comparison is exact: integers and date-likes by value, floats by bit pattern (all NaNs one value).
"""
import numpy as np
import pytest

import scalar_cases as cases
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpupreagg import GpuPreAgg
from pg_strom_amd.gpuscan import GpuScan

pytestmark = pytest.mark.gpu


def test_case_is_lazy_on_the_device():
    """(case ..) is emitted as a C ternary: the branch not taken is not evaluated, so it raises
    nothing.  Every program below relies on it."""
    n = 200
    sel = (np.arange(n) % 3 == 0).astype(np.int32)
    div = (np.arange(n) % 2).astype(np.int32)                   # every other divisor is zero
    buf = kds.build_kds("column", [kds.Column("int4", sel), kds.Column("int4", div)])
    expr = ("(case (when (int4eq (var 1 int4) (const int4 1)) (int4div (const int4 6) (var 2 int4)))"
            " (else (const int4 7)))")
    scan = GpuScan("(isnotnull %s)" % expr).begin()
    try:
        res = scan.scan_chunk(buf)
    finally:
        scan.end()
    assert np.array_equal(res.recheck_rows(), np.flatnonzero((sel == 1) & (div == 0)))
    assert np.array_equal(res.passed_rows(), np.flatnonzero((sel == 0) | (div != 0)))
    assert len(res.recheck_rows()) > 20 and np.count_nonzero((sel == 0) & (div == 0)) > 20


def _differing(case, got, want):
    """the rows only one side has: how many per function, then the first few in full"""
    rows = np.setxor1d(got, want)
    per_function = {}
    for r in rows:
        name = case.functions[case.fid[r]][0]
        per_function[name] = per_function.get(name, 0) + 1
    return "%r; first: %s" % (per_function, "; ".join(
        case.describe(r) + (" device only" if r in got else " model only") for r in rows[:8]))


@pytest.mark.parametrize("rettype", cases.RETURN_TYPES)
def test_recheck_and_null_rows_are_the_models(rettype):
    case = cases.return_type_case(rettype)
    assert case.functions and case.recheck.any() and case.isnull.any()      # nothing passes for want of rows
    for ids in case.groups():
        mine = case.rows_of(ids)
        scan = GpuScan("(isnotnull %s)" % case.case_expr(ids)).begin()
        try:
            res = scan.scan_chunk(case.buf)
        finally:
            scan.end()
        want = mine[case.recheck[mine]]
        got = res.recheck_rows()
        assert np.array_equal(got, want), "recheck rows differ: " + _differing(case, got, want)
        want = mine[~case.isnull[mine]]
        got = res.passed_rows()
        assert np.array_equal(got, want), "non-NULL rows differ: " + _differing(case, got, want)


@pytest.mark.parametrize("rettype", cases.RETURN_TYPES)
def test_values_are_the_models(rettype):
    case = cases.return_type_case(rettype)
    runtime.init()
    assert case.functions
    for ids in case.groups():
        mine = case.rows_of(ids)
        ok = mine[~case.recheck[mine]]
        assert len(ok)
        agg = GpuPreAgg("(gpupreagg (key (var 1 int4)) (pmax %s))" % case.carried_expr(ids)).begin([(0, case.nrows)])
        try:
            status = agg.fold(case.buf, row_map=ok.astype(np.int32))[0]
            assert status == 0, "the device rechecks a row the model calls error-free"
            pr = agg.fetch()
        finally:
            agg.end()
        keys = pr.values[:, 0].astype(np.int64) & 0xFFFFFFFF
        order = np.argsort(keys)
        assert np.array_equal(keys[order], ok)
        bad = case.check_values(ok, pr.values[order, 1], pr.isnull[order, 1])
        assert not bad, "%d rows differ, first: %s" % (len(bad), "; ".join(bad[:8]))
