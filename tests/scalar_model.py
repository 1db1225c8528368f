"""
An independent model of the scalar device functions (strom_mathlib.h, strom_timelib.h): what each
catalog entry flagged DEVFUNC_NEEDS_MATHLIB or DEVFUNC_NEEDS_TIMELIB returns for given arguments,
written from the reference's sources and not from this project's device code or CPU oracle.

Plain Python: int for integers, dates and times; numpy.float32 / numpy.float64 scalars for floats,
so every rounding is IEEE's.  No ctypes, nothing of the package or the oracle is imported.

    evaluate(name, argtypes, args) -> (value, isnull, recheck)     args: a value or None (NULL) each

Rules, in this order:
  * strict: a NULL argument gives NULL and no recheck.
  * the arithmetic is the reference's; every rule cites its file:line there (opencl_mathlib.h,
    opencl_timelib.h, opencl_textlib.h, opencl_common.h, and the templates of codegen.c:211-630 as
    devfunc_setup_* expand them, codegen.c:632-802).
  * the project's written policy (headers of strom_mathlib.h and strom_timelib.h): where the
    reference would wrap or produce a value PostgreSQL refuses, the outcome is recheck -- integer,
    date and timestamp overflow, a narrowing cast out of range, division by zero, MIN / -1, float
    overflow, float underflow to zero from non-zero inputs, sqrt of a negative number.
  * where the reference and PostgreSQL return different VALUES the rule says which one is modelled
    and why (float comparisons with a NaN, round(), the sign of sign()'s zero, bpchar(1)).

Out of scope (they have models of their own): the transcendental functions, numeric, text and
character(n).

The edge grids are exported too: grid(type) per argument type, rows(name, argtypes) per function.
"""
import itertools

import numpy as np

# STROM_*OID (strom_kds.h); the sql names are the IR's and kds.SQL_TYPES'
OIDS = {"bool": 16, "int2": 21, "int4": 23, "int8": 20, "float4": 700, "float8": 701,
        "date": 1082, "time": 1083, "timestamp": 1114, "char1": 1042}
TYPE_OF_OID = {v: k for k, v in OIDS.items()}
DEVFUNC_NEEDS_TIMELIB = 0x0008
DEVFUNC_NEEDS_MATHLIB = 0x0040

INT_RANGE = {"int2": (-2**15, 2**15 - 1), "int4": (-2**31, 2**31 - 1), "int8": (-2**63, 2**63 - 1)}
DATE_NOBEGIN, DATE_NOEND = -2**31, 2**31 - 1            # DATEVAL_NOBEGIN / DATEVAL_NOEND, opencl_timelib.h:26-27
TS_NOBEGIN, TS_NOEND = -2**63, 2**63 - 1                # DT_NOBEGIN / DT_NOEND, opencl_timelib.h:57-58
USECS_PER_DAY = 86400000000                             # opencl_timelib.h:52
POSTGRES_EPOCH_JDATE = 2451545                          # date2j(2000, 1, 1), opencl_timelib.h:75
# the last day whose microseconds fit int64 (pgfn_date_timestamp's overflow test, opencl_timelib.h:311-317)
LAST_TS_DAY = (2**63 - 1) // USECS_PER_DAY

OUT_OF_SCOPE = {"cbrt", "dcbrt", "exp", "dexp", "ln", "dlog1", "log", "dlog10", "power", "pow", "dpow",
                "degrees", "radians", "acos", "asin", "atan", "atan2", "cos", "sin", "tan"}

RECHECK = (None, True, True)
NULL = (None, True, False)


def _ok(v):
    return (v, False, False)


def in_scope(name, flags):
    return bool(flags & (DEVFUNC_NEEDS_MATHLIB | DEVFUNC_NEEDS_TIMELIB)) and name not in OUT_OF_SCOPE


# ---------------------------------------------------------------------------------------------
# the rules: RULES[(name, (argtype, ...))] = (result type, function of the non-NULL arguments)
# ---------------------------------------------------------------------------------------------
RULES = {}
SIGN_OF_ZERO_UNSPECIFIED = set()        # rule keys whose zero result may carry either sign


def _rule(name, argtypes, rettype, fn):
    key = (name, tuple(argtypes))
    assert key not in RULES, key
    RULES[key] = (rettype, fn)


def _checked_int(rettype, v):
    """policy: a result outside the result type is CpuReCheck where the reference tests for it
    (SAMESIGN, opencl_mathlib.h:45-50, 111-116, 176-181 ...) and also where it would wrap"""
    lo, hi = INT_RANGE[rettype]
    return _ok(v) if lo <= v <= hi else RECHECK


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _cdiv(a, b):
    """C's '/': truncation towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


FAMILIES = [("int2", "int2", "int2", "int2"), ("int24", "int2", "int4", "int4"),
            ("int28", "int2", "int8", "int8"), ("int42", "int4", "int2", "int4"),
            ("int4", "int4", "int4", "int4"), ("int48", "int4", "int8", "int8"),
            ("int82", "int8", "int2", "int8"), ("int84", "int8", "int4", "int8"),
            ("int8", "int8", "int8", "int8")]
# result = the wider operand, PostgreSQL's signatures (pg_proc); the reference's templates
# instantiate a few of them with other types (opencl_mathlib.h:78-83), SURVEY.md Appendix C
for pfx, x, y, r in FAMILIES:
    # BASIC_INT_ADDFUNC_TEMPLATE, opencl_mathlib.h:34-53 (instances 77-87): sum, SAMESIGN test
    _rule(pfx + "pl", (x, y), r, lambda a, b, r=r: _checked_int(r, a + b))
    # BASIC_INT_SUBFUNC_TEMPLATE, opencl_mathlib.h:100-119 (instances 143-153)
    _rule(pfx + "mi", (x, y), r, lambda a, b, r=r: _checked_int(r, a - b))
    # pgfn_int2mul .. pgfn_int8mul, opencl_mathlib.h:167-356: product, tested by dividing back
    _rule(pfx + "mul", (x, y), r, lambda a, b, r=r: _checked_int(r, a * b))
    # pgfn_int2div .. pgfn_int8div, opencl_mathlib.h:447-670: zero divisor -> CpuReCheck (455-459);
    # divisor -1 negates, and MIN / -1 is CpuReCheck (460-468); otherwise C's truncating '/'.
    # int24div / int28div / int48div have no -1 branch (476-492): their quotient always fits.
    _rule(pfx + "div", (x, y), r, lambda a, b, r=r: RECHECK if b == 0 else _checked_int(r, _cdiv(a, b)))
    # "b:==" .. "b:<=" (codegen.c:326-413) through devfunc_setup_oper_both (codegen.c:662-693):
    # C's comparison after the usual arithmetic conversions, exact for every pair of integers
    _rule(pfx + "eq", (x, y), "bool", lambda a, b: _ok(int(a == b)))
    _rule(pfx + "ne", (x, y), "bool", lambda a, b: _ok(int(a != b)))
    _rule(pfx + "lt", (x, y), "bool", lambda a, b: _ok(int(a < b)))
    _rule(pfx + "le", (x, y), "bool", lambda a, b: _ok(int(a <= b)))
    _rule(pfx + "gt", (x, y), "bool", lambda a, b: _ok(int(a > b)))
    _rule(pfx + "ge", (x, y), "bool", lambda a, b: _ok(int(a >= b)))
    # "f:devfunc_int_comp" (codegen.c:447-455); devfunc_int_comp, opencl_common.h:1550-1551
    _rule("bt" + pfx + "cmp", (x, y), "int4", lambda a, b: _ok((a > b) - (a < b)))


def _float_check(val, inf_is_valid, zero_is_valid):
    """CHECKFLOATVAL, opencl_mathlib.h:25-27"""
    if (np.isinf(val) and not inf_is_valid) or (val == 0.0 and not zero_is_valid):
        return RECHECK
    return _ok(val)


FLOAT_T = {"float4": np.float32, "float8": np.float64}
FFAMILIES = [("float4", "float4", "float4", "float4"), ("float48", "float4", "float8", "float8"),
             ("float84", "float8", "float4", "float8"), ("float8", "float8", "float8", "float8")]


def _farith(op, r):
    T = FLOAT_T[r]

    def fn(a, b):
        with np.errstate(all="ignore"):
            a, b = T(a), T(b)       # float4 op float8: C converts the float4 operand to double
            either_inf = bool(np.isinf(a) or np.isinf(b))
            if op == "pl":          # BASIC_FLOAT_ADDFUNC_TEMPLATE, opencl_mathlib.h:55-75 (89-92)
                return _float_check(a + b, either_inf, True)
            if op == "mi":          # BASIC_FLOAT_SUBFUNC_TEMPLATE, opencl_mathlib.h:121-141 (155-158)
                return _float_check(a - b, either_inf, True)
            if op == "mul":         # pgfn_float4mul .. pgfn_float8mul, opencl_mathlib.h:358-440
                return _float_check(a * b, either_inf, bool(a == 0.0 or b == 0.0))
            # pgfn_float4div .. pgfn_float8div, opencl_mathlib.h:672-782: a zero divisor of either
            # sign is CpuReCheck (680-684), then CHECKFLOATVAL (688-694)
            if b == 0.0:
                return RECHECK
            return _float_check(a / b, either_inf, bool(a == 0.0))
    return fn


def _pg_float_cmp(a, b):
    """devfunc_float_comp, opencl_common.h:1553-1560: NaN = NaN, NaN above every number"""
    a, b = np.float64(a), np.float64(b)         # float4 -> float8 is exact
    if np.isnan(a):
        return 0 if np.isnan(b) else 1
    if np.isnan(b):
        return -1
    return int(a > b) - int(a < b)


for pfx, x, y, r in FFAMILIES:
    for op in ("pl", "mi", "mul", "div"):
        _rule(pfx + op, (x, y), r, _farith(op, r))
    # "b:==" .. "b:<=" (codegen.c:335-338 .. 410-413; devfunc_setup_oper_both, codegen.c:662-693):
    # the reference emits C's bare comparison, which is IEEE's -- false for every operator but !=
    # when an operand is NaN.  PostgreSQL (float8_cmp_internal) orders NaN above every number and
    # equal to itself, and so does the reference's own three-way compare (opencl_common.h:1553).
    # On rows WITHOUT a NaN the two agree and the model is the reference.  On rows with one the
    # model is PostgreSQL's order, not the reference's: it is this project's written policy
    # (strom_mathlib.h, "Deliberate differences"), these functions are also the equality behind
    # float join and grouping keys, where NaN = NaN is needed to put NaNs together, and no
    # CpuReCheck is raised, so a wrong answer here would reach the query's result.
    _rule(pfx + "eq", (x, y), "bool", lambda a, b: _ok(int(_pg_float_cmp(a, b) == 0)))
    _rule(pfx + "ne", (x, y), "bool", lambda a, b: _ok(int(_pg_float_cmp(a, b) != 0)))
    _rule(pfx + "lt", (x, y), "bool", lambda a, b: _ok(int(_pg_float_cmp(a, b) < 0)))
    _rule(pfx + "le", (x, y), "bool", lambda a, b: _ok(int(_pg_float_cmp(a, b) <= 0)))
    _rule(pfx + "gt", (x, y), "bool", lambda a, b: _ok(int(_pg_float_cmp(a, b) > 0)))
    _rule(pfx + "ge", (x, y), "bool", lambda a, b: _ok(int(_pg_float_cmp(a, b) >= 0)))
    # "f:devfunc_float_comp" (codegen.c:456-459), opencl_common.h:1553-1560; here the reference and
    # PostgreSQL (btfloat8cmp) agree
    _rule("bt" + pfx + "cmp", (x, y), "int4", lambda a, b: _ok(_pg_float_cmp(a, b)))

for t in ("int2", "int4", "int8"):
    bits = {"int2": 16, "int4": 32, "int8": 64}[t]
    # BASIC_INT_MODFUNC_TEMPLATE, opencl_mathlib.h:787-808: zero divisor -> CpuReCheck (797-801),
    # divisor -1 -> 0 without dividing (802-803), otherwise C's '%' (sign of the dividend)
    _rule(t + "mod", (t, t), t,
          lambda a, b: RECHECK if b == 0 else _ok(0 if b == -1 else a - b * _cdiv(a, b)))
    # "l:-" (codegen.c:312-314, there under the names int2mi ..; devfunc_setup_oper_either,
    # codegen.c:695-726): a bare negation, which wraps at MIN -- policy: CpuReCheck
    _rule(t + "um", (t,), t, lambda a, t=t: _checked_int(t, -a))
    # "l:+" (codegen.c:305-307)
    _rule(t + "up", (t,), t, lambda a: _ok(a))
    # "f:abs" / "af:abs" (codegen.c:319-321, 464-466; devfunc_setup_func_decl, codegen.c:728-802):
    # OpenCL's abs() cast back to the signed type wraps at MIN -- policy: CpuReCheck
    _rule(t + "abs", (t,), t, lambda a, t=t: _checked_int(t, abs(a)))
    _rule("abs", (t,), t, lambda a, t=t: _checked_int(t, abs(a)))
    # "b:~" (codegen.c:431-433), "b:&" (416-418), "b:|" (421-423), "b:^" (426-428)
    _rule(t + "not", (t,), t, lambda a: _ok(~a))
    _rule(t + "and", (t, t), t, lambda a, b: _ok(a & b))
    _rule(t + "or", (t, t), t, lambda a, b: _ok(a | b))
    _rule(t + "xor", (t, t), t, lambda a, b: _ok(a ^ b))
    # "b:<<" / "b:>>" (codegen.c:436-443; devfunc_setup_oper_both casts the result to the result
    # type, codegen.c:682): OpenCL C takes the count modulo the width of the PROMOTED left operand
    # (OpenCL C 6.3.j) -- 32 for int2 and int4, 64 for int8; '>>' of a signed value is arithmetic.
    # (PostgreSQL's C shift is undefined for such counts; x86 gives the same.)
    mask = 63 if t == "int8" else 31
    _rule(t + "shl", (t, "int4"), t, lambda a, n, mask=mask, bits=bits: _ok(_wrap(a << (n & mask), bits)))
    _rule(t + "shr", (t, "int4"), t, lambda a, n, mask=mask, bits=bits: _ok(_wrap(a >> (n & mask), bits)))

for t in ("float4", "float8"):
    # "l:-" / "l:+" (codegen.c:308-309, 315-316), "l:fabs" / "af:fabs" (322-323, 467-468):
    # sign operations, exact; no CHECKFLOATVAL
    _rule(t + "um", (t,), t, lambda a, T=FLOAT_T[t]: _ok(-T(a)))
    _rule(t + "up", (t,), t, lambda a, T=FLOAT_T[t]: _ok(T(a)))
    _rule(t + "abs", (t,), t, lambda a, T=FLOAT_T[t]: _ok(np.abs(T(a))))
    _rule("abs", (t,), t, lambda a, T=FLOAT_T[t]: _ok(np.abs(T(a))))

# booleq / boolne: PostgreSQL's (bool.c); the reference's catalog has no entry for them, the
# three-way compare is "f:devfunc_int_comp" (codegen.c:446)
_rule("booleq", ("bool", "bool"), "bool", lambda a, b: _ok(int(bool(a) == bool(b))))
_rule("boolne", ("bool", "bool"), "bool", lambda a, b: _ok(int(bool(a) != bool(b))))
_rule("btboolcmp", ("bool", "bool"), "int4", lambda a, b: _ok(int(bool(a)) - int(bool(b))))


def _char1_key(c):
    """bpchar_truelen (opencl_textlib.h:154-167): a blank is padding, so ' ' is the empty string,
    which sorts below every character (bpchar_compare, 189-190)"""
    c &= 0xFF
    return -1 if c == 0x20 else c


# bpchar(1) carried by value: pgfn_bpchareq .. pgfn_bpcharcmp over bpchar_compare
# (opencl_textlib.h:169-283) for one-byte strings.  The reference compares the bytes as signed
# cl_char (181-184); PostgreSQL's bpcharcmp is memcmp, unsigned.  They differ for bytes above 0x7f
# and nothing is rechecked: the model is PostgreSQL's, this project's stated choice
# (strom_mathlib.h, "bytewise (unsigned) comparison").
for op, f in (("eq", lambda c: c == 0), ("ne", lambda c: c != 0), ("lt", lambda c: c < 0),
              ("le", lambda c: c <= 0), ("gt", lambda c: c > 0), ("ge", lambda c: c >= 0)):
    _rule("bpchar" + op, ("char1", "char1"), "bool",
          lambda a, b, f=f: _ok(int(f(_char1_key(a) - _char1_key(b)))))
_rule("bpcharcmp", ("char1", "char1"), "int4",
      lambda a, b: _ok(int(_char1_key(a) > _char1_key(b)) - int(_char1_key(a) < _char1_key(b))))


# ---- casts: "a/c:" (codegen.c:213-237) through devfunc_setup_cast (codegen.c:632-659) ------------
def int_to_float(v, T):
    """(float)v / (double)v: round to nearest, ties to even, in exact integer arithmetic"""
    p = 24 if T is np.float32 else 53
    m = abs(v)
    n = m.bit_length()
    if n > p:
        shift = n - p
        q, rem, half = m >> shift, m & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
        m = q << shift
    return T(float(-m if v < 0 else m))         # at most p significant bits: exact


def _float_to_int(rettype):
    lo, hi = INT_RANGE[rettype]

    def fn(a):
        # the reference's bare (cl_int)arg.value (codegen.c:650) truncates and is undefined out of
        # range; PostgreSQL's dtoi2 / dtoi4 / dtoi8 round to nearest-even (rint) and refuse what
        # does not fit.  Policy: rint, then CpuReCheck outside [MIN, MAX] (NaN included).
        r = np.rint(np.float64(a))
        if np.isnan(r) or r < np.float64(lo) or r >= np.float64(hi + 1):      # -2^n and 2^n are exact
            return RECHECK
        return _ok(int(r))
    return fn


for src in ("int2", "int4", "int8"):
    for dst in ("int2", "int4", "int8"):
        if src != dst:
            # widening is exact; narrowing: the bare cast wraps -- policy: CpuReCheck out of range
            _rule(dst, (src,), dst, lambda a, dst=dst: _checked_int(dst, a))
    for dst in ("float4", "float8"):
        _rule(dst, (src,), dst, lambda a, T=FLOAT_T[dst]: _ok(int_to_float(a, T)))
for src in ("float4", "float8"):
    for dst in ("int2", "int4", "int8"):
        _rule(dst, (src,), dst, _float_to_int(dst))
_rule("float8", ("float4",), "float8", lambda a: _ok(np.float64(np.float32(a))))      # exact


def _float8_float4(a):
    # the bare (cl_float) cast rounds to nearest; PostgreSQL's dtof refuses an overflow to infinity
    # and an underflow to zero (CHECKFLOATVAL) -- policy: CpuReCheck
    with np.errstate(all="ignore"):
        a = np.float64(a)
        return _float_check(np.float32(a), bool(np.isinf(a)), bool(a == 0.0))


_rule("float4", ("float8",), "float4", _float8_float4)
_rule("int4", ("bool",), "int4", lambda a: _ok(int(bool(a))))        # codegen.c:218

# ---- float8 functions -------------------------------------------------------------------------
for n in ("ceil", "ceiling"):       # "f:ceil", codegen.c:471-472
    _rule(n, ("float8",), "float8", lambda a: _ok(np.ceil(np.float64(a))))
_rule("floor", ("float8",), "float8", lambda a: _ok(np.floor(np.float64(a))))      # codegen.c:475
for n in ("round", "dround"):
    # "f:round" (codegen.c:484-485): OpenCL's round() takes halves away from zero; PostgreSQL's
    # dround (float.c) is rint(), halves to even.  No recheck can tell them apart; the model is
    # PostgreSQL's, whose output is the reference's own expected result (input/make_expected.sh:22-28,
    # the ground DESIGN.md section 4 gives for every change towards PostgreSQL).  strom_mathlib.h's
    # header names this rounding for the float -> int casts only; round() follows it by the same reason.
    _rule(n, ("float8",), "float8", lambda a: _ok(np.rint(np.float64(a))))
for n in ("trunc", "dtrunc"):       # "f:trunc", codegen.c:489-490
    _rule(n, ("float8",), "float8", lambda a: _ok(np.trunc(np.float64(a))))


def _sign(a):
    a = np.float64(a)
    return _ok(np.float64(1.0 if a > 0 else (-1.0 if a < 0 else 0.0)))


# "f:sign" (codegen.c:486): OpenCL's sign() is 1, -1, a zero of the argument's sign, and 0 for NaN;
# PostgreSQL's dsign gives +0 for both zeros and for NaN.  The sign of a zero result is unspecified.
_rule("sign", ("float8",), "float8", _sign)
SIGN_OF_ZERO_UNSPECIFIED.add(("sign", ("float8",)))
for n in ("sqrt", "dsqrt"):
    # "f:sqrt" (codegen.c:487-488) gives NaN for a negative argument, PostgreSQL's dsqrt refuses
    # it -- policy: CpuReCheck.  sqrt(-0.0) is -0.0 in both.  IEEE sqrt is correctly rounded.
    _rule(n, ("float8",), "float8",
          lambda a: RECHECK if np.float64(a) < 0 else _ok(np.sqrt(np.float64(a))))
_rule("pi", (), "float8", lambda: _ok(np.float64(3.14159265358979323846)))       # pgfn_dpi, opencl_mathlib.h:840-848


# ---- date / time / timestamp ----------------------------------------------------------------------
def _date_is_infinite(d):
    return d in (DATE_NOBEGIN, DATE_NOEND)               # DATE_NOT_FINITE, opencl_timelib.h:33


def _date_timestamp(d):
    """pgfn_date_timestamp, opencl_timelib.h:288-320"""
    if d == DATE_NOBEGIN:
        return _ok(TS_NOBEGIN)                           # 297-301
    if d == DATE_NOEND:
        return _ok(TS_NOEND)                             # 302-306
    ts = d * USECS_PER_DAY                               # 311
    return _ok(ts) if -2**63 <= ts <= 2**63 - 1 else RECHECK      # 313-317


def _timestamp_split(t):
    """timestamp2tm, opencl_timelib.h:189-220: (days since 2000-01-01, microseconds of the day), or
    None where it fails -- a Julian day below 0 (204-209).  Its other bound, a Julian day above
    INT_MAX, is out of reach: int64 microseconds end at day LAST_TS_DAY."""
    date, time = divmod(t, USECS_PER_DAY)               # TMODULO + the fix-up of 199-203: floor
    if date + POSTGRES_EPOCH_JDATE < 0:
        return None
    return date, time


def _timestamp_date(t):
    """pgfn_timestamp_date, opencl_timelib.h:227-257"""
    if t == TS_NOBEGIN:
        return _ok(DATE_NOBEGIN)                         # 236-240
    if t == TS_NOEND:
        return _ok(DATE_NOEND)                           # 241-245
    s = _timestamp_split(t)
    if s is None:
        return RECHECK                                   # 246-250
    return _ok(s[0])          # date2j(j2date(jd)) - epoch (253-254) is jd - epoch again


def _timestamp_time(t):
    """pgfn_timestamp_time, opencl_timelib.h:260-286"""
    if t in (TS_NOBEGIN, TS_NOEND):
        return NULL                                      # 269-270: NULL, no error
    s = _timestamp_split(t)
    if s is None:
        return RECHECK                                   # 271-275
    return _ok(s[1])                                     # 279-283 rebuilds the microseconds of the day


def _date_pli(d, n):
    """pgfn_date_pli, opencl_timelib.h:325-341; the sum wraps there (338) -- policy: CpuReCheck"""
    if _date_is_infinite(d):
        return _ok(d)                                    # 335-336: can't change infinity
    return _checked_int("int4", d + n)


def _date_mii(d, n):
    """pgfn_date_mii, opencl_timelib.h:343-359"""
    if _date_is_infinite(d):
        return _ok(d)                                    # 353-354
    return _checked_int("int4", d - n)


def _date_mi(a, b):
    """pgfn_date_mi, opencl_timelib.h:361-379"""
    if _date_is_infinite(a) or _date_is_infinite(b):
        return RECHECK                                   # 368-372
    return _checked_int("int4", a - b)                   # 376 wraps -- policy: CpuReCheck


def _datetime_pl(d, t):
    """pgfn_datetime_pl, opencl_timelib.h:381-395"""
    ts = _date_timestamp(d)                              # 390
    if ts[1] or ts[0] in (TS_NOBEGIN, TS_NOEND):         # 391: an infinite timestamp stays
        return ts
    s = ts[0] + t                                        # 392 wraps -- policy: CpuReCheck
    return _ok(s) if -2**63 <= s <= 2**63 - 1 else RECHECK


_rule("timestamp", ("date",), "timestamp", _date_timestamp)
_rule("date", ("timestamp",), "date", _timestamp_date)
_rule("time", ("timestamp",), "time", _timestamp_time)
# "ta/c:" alias casts (codegen.c:542, 545, 546): the value as it is
_rule("date", ("date",), "date", lambda a: _ok(a))
_rule("time", ("time",), "time", lambda a: _ok(a))
_rule("timestamp", ("timestamp",), "timestamp", lambda a: _ok(a))
_rule("date_pli", ("date", "int4"), "date", _date_pli)
_rule("date_mii", ("date", "int4"), "date", _date_mii)
_rule("date_mi", ("date", "date"), "int4", _date_mi)
_rule("integer_pl_date", ("int4", "date"), "date", lambda n, d: _date_pli(d, n))    # opencl_timelib.h:397-401
_rule("datetime_pl", ("date", "time"), "timestamp", _datetime_pl)
_rule("timedate_pl", ("time", "date"), "timestamp", lambda t, d: _datetime_pl(d, t))   # opencl_timelib.h:403-407

_CMP_OPS = (("eq", lambda c: c == 0), ("ne", lambda c: c != 0), ("lt", lambda c: c < 0),
            ("le", lambda c: c <= 0), ("gt", lambda c: c > 0), ("ge", lambda c: c >= 0))
for t in ("date", "time", "timestamp"):
    # "t/b:==" .. (codegen.c:558-563, 581-586, 589-594): the raw values compared, so the
    # infinities sort at the ends; "t/f:devfunc_int_comp" (564, 587, 595-596)
    for op, f in _CMP_OPS:
        _rule("%s_%s" % (t, op), (t, t), "bool", lambda a, b, f=f: _ok(int(f((a > b) - (a < b)))))
    _rule(t + "_cmp", (t, t), "int4", lambda a, b: _ok((a > b) - (a < b)))


def _date_vs_ts(f, date_first):
    # pgfn_date_eq_timestamp .. pgfn_timestamp_cmp_date, opencl_timelib.h:412-661: the date is
    # promoted by pgfn_date_timestamp (417, 544 ...), a promotion that fails is CpuReCheck, then the
    # raw values are compared.  (The reference promotes BEFORE it looks at the other argument's
    # NULL flag, 417-419, and so would flag a row whose answer is NULL anyway; the strictness rule
    # comes first here, as in PostgreSQL, where a strict function is not called at all.)
    def fn(a, b):
        ts = _date_timestamp(a if date_first else b)
        if ts[1]:
            return ts
        l, r = (ts[0], b) if date_first else (a, ts[0])
        return _ok(int(f((l > r) - (l < r))))
    return fn


for op, f in _CMP_OPS + (("cmp", lambda c: c),):
    _rule("date_%s_timestamp" % op, ("date", "timestamp"), "int4" if op == "cmp" else "bool",
          _date_vs_ts(f, True))
    _rule("timestamp_%s_date" % op, ("timestamp", "date"), "int4" if op == "cmp" else "bool",
          _date_vs_ts(f, False))


def evaluate(name, argtypes, args):
    """(value, isnull, recheck) of one call; args: a value or None (NULL) per argument"""
    rettype, fn = RULES[(name, tuple(argtypes))]
    if any(a is None for a in args):
        return NULL
    return fn(*args)


def return_type(name, argtypes):
    return RULES[(name, tuple(argtypes))][0]


# ---------------------------------------------------------------------------------------------
# edge grids
# ---------------------------------------------------------------------------------------------
def _int_grid(t):
    lo, hi = INT_RANGE[t]
    g = [lo, lo + 1, -2, -1, 0, 1, 2, hi - 1, hi]
    for n in ("int2", "int4"):                  # the neighbours of every narrower type's bounds
        b = INT_RANGE[n][1] + 1                 # 32768, 2^31
        if b < hi:
            g += [b - 1, b, b + 1, -b + 1, -b, -b - 1]
    return sorted(set(g))


def _flimits(T):
    fi = np.finfo(T)
    tiny = T(fi.smallest_subnormal)
    return dict(min_denormal=tiny, max_denormal=np.nextafter(T(fi.tiny), T(0)),
                min_normal=T(fi.tiny), max_normal=T(fi.max))


def _float_core(T):
    """the values every float argument takes, also inside a cross product: zeros, infinities, NaN,
    the ends of the denormal and normal ranges, the halves of round-half-to-even, and operands
    whose products and quotients land in the denormals, on zero, on the largest finite number
    and beyond it"""
    L = _flimits(T)
    g = [T(0.0), T(-0.0), T(np.inf), T(-np.inf), T(np.nan),
         L["min_denormal"], L["max_denormal"], L["min_normal"], L["max_normal"],
         -L["min_denormal"], -L["max_normal"],
         T(0.5), T(-0.5), T(1.5), T(-1.5), T(2.5), T(-2.5), T(1.0), T(2.0), T(3.0),
         L["max_normal"] / T(2),                 # x 2.0 = the largest finite number, exactly
         # the cast bounds of int4 and int8 (exact in either type): sums and differences next to them
         T(2.0) ** 31, -T(2.0) ** 31, T(2.0) ** 63, -T(2.0) ** 63]
    if T is np.float64:
        # 2^-537 squared is the smallest denormal; 2^512 squared overflows; 1e-160 x 1e-150 is a
        # denormal, 1e-160 squared underflows to zero; 1e-160 / 2^512 is a denormal
        g += [T(2.0) ** -537, T(2.0) ** 512, T(1e-160), T(1e-150),
              np.float64(np.finfo(np.float32).max), np.float64(np.finfo(np.float32).smallest_subnormal)]
    else:
        g += [T(2.0) ** -75, T(2.0) ** -74, T(2.0) ** 64, T(1e-20), T(1e-25)]
    return g


def _float_cast_edges(T):
    """what only a cast can get wrong (unary functions): each integer target's bounds +-0.5 and
    +-1 -- at 2^31 in float4 and at 2^63 the representable neighbours -- and, for float8, values
    just inside and outside float4's range at both ends"""
    g = []
    for t in ("int2", "int4", "int8"):
        lo, hi = INT_RANGE[t]
        for bound in (lo, hi + 1):                          # -2^n and 2^n: exact in either type
            b = T(float(bound))
            g += [b, np.nextafter(b, T(np.inf)), np.nextafter(b, T(-np.inf))]
            for d in (0.5, 1.0, 1.5, 2.0):
                for v in (float(bound) + d, float(bound) - d):
                    if abs(bound) < 2**52 and T(v) == np.float64(v):      # representable: use it as it is
                        g.append(T(v))
    if T is np.float64:
        g += [T(2147483647.4999), T(-2147483648.4999), T(32767.4999), T(1e-50), T(-1e-50)]
        f4 = np.finfo(np.float32)
        fmax = np.float64(f4.max)
        over = np.float64(2.0) ** 128 - np.float64(2.0) ** 103     # half way to 2^128: rounds to infinity
        tie0 = np.float64(2.0) ** -150                              # half way to the smallest denormal: rounds to 0
        g += [np.nextafter(fmax, np.inf), np.nextafter(over, 0.0), over, -over,
              tie0, np.nextafter(tie0, 1.0), -tie0, np.nextafter(np.float64(f4.tiny), 0.0)]
    return g


def _unique_floats(values, T):
    seen, out = set(), []
    for v in values:
        v = T(v)
        key = "nan" if np.isnan(v) else v.tobytes()
        if key not in seen:
            seen.add(key)
            out.append(v)
    return out


SHIFT_COUNTS = [-1, 0, 1, 15, 16, 31, 32, 33, 63, 64, 65]
DATE_GRID = sorted(set([DATE_NOBEGIN, DATE_NOBEGIN + 1, DATE_NOEND - 1, DATE_NOEND,
                        -POSTGRES_EPOCH_JDATE - 1, -POSTGRES_EPOCH_JDATE, -POSTGRES_EPOCH_JDATE + 1,
                        -LAST_TS_DAY - 1, -LAST_TS_DAY, -LAST_TS_DAY + 1,
                        LAST_TS_DAY - 1, LAST_TS_DAY, LAST_TS_DAY + 1, -1, 0, 1]))
TIMESTAMP_GRID = sorted(set([TS_NOBEGIN, TS_NOBEGIN + 1, TS_NOEND - 1, TS_NOEND, -1, 0, 1] +
                            [k * USECS_PER_DAY + d
                             for k in (-POSTGRES_EPOCH_JDATE - 1, -POSTGRES_EPOCH_JDATE, -1, 0, 1)
                             for d in (-1, 0, 1)]))
TIME_GRID = [0, 1, USECS_PER_DAY - 1, USECS_PER_DAY]
# bpchar(1): byte 0 and a control character (both ABOVE the blank), the blank (padding: the empty
# string), letters, the ends of 7-bit and 8-bit bytes -- as the signed bytes a column holds
CHAR1_GRID = [0, 1, 0x20, 0x41, 0x61, 0x7f, -128, -1]


def grid(t, role="binary"):
    """the argument values of type t, NULL (None) last; role "unary" adds the cast edges"""
    if t in INT_RANGE:
        g = _int_grid(t)
    elif t in FLOAT_T:
        T = FLOAT_T[t]
        g = _unique_floats(_float_core(T) + (_float_cast_edges(T) if role == "unary" else []), T)
    else:
        g = {"bool": [0, 1], "date": DATE_GRID, "time": TIME_GRID, "timestamp": TIMESTAMP_GRID,
             "char1": CHAR1_GRID}[t]
    return list(g) + [None]


def rows(name, argtypes):
    """the grid rows of one function: its whole grid for a unary one, the cross product for a
    binary one; the count argument of a shift runs over SHIFT_COUNTS"""
    argtypes = tuple(argtypes)
    if len(argtypes) == 0:
        return [()]
    if len(argtypes) == 1:
        return [(v,) for v in grid(argtypes[0], "unary")]
    g2 = (SHIFT_COUNTS + [None]) if name[-3:] in ("shl", "shr") else grid(argtypes[1])
    return list(itertools.product(grid(argtypes[0]), g2))


# ---------------------------------------------------------------------------------------------
# comparing outcomes
# ---------------------------------------------------------------------------------------------
def value_image(t, v):
    """a value as the 64-bit datum image the chunks and results carry"""
    if t == "float4":
        return int(np.array([v], dtype=np.float32).view(np.uint32)[0])
    if t == "float8":
        return int(np.array([v], dtype=np.float64).view(np.uint64)[0])
    return int(v) & 0xFFFFFFFFFFFFFFFF


def same_value(key, rettype, want, got_image):
    """is the 64-bit image 'got_image' the model's value 'want'?  Exact: integers by value, floats
    by bit pattern with all NaNs one value; -0.0 is not +0.0 unless the rule leaves the sign open"""
    if rettype in FLOAT_T:
        T = FLOAT_T[rettype]
        if T is np.float32:
            got = np.array([got_image & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]
        else:
            got = np.array([got_image], dtype=np.uint64).view(np.float64)[0]
        if np.isnan(want) or np.isnan(got):
            return bool(np.isnan(want) and np.isnan(got))
        if want == 0 and got == 0 and key in SIGN_OF_ZERO_UNSPECIFIED:
            return True
        return T(want).tobytes() == T(got).tobytes()
    bits = {"bool": 8, "char1": 8, "int2": 16, "int4": 32, "date": 32}.get(rettype, 64)
    got = _wrap(int(got_image), bits)
    if rettype == "bool":
        return bool(got) == bool(want)
    return got == int(want)
