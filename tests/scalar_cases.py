"""
What the scalar-function tests share: the in-scope part of the device function catalog (read
through strom_codegen_catalog_entry), and the chunks and expressions that put scalar_model's grids
in front of an evaluator -- the CPU oracle (test_scalar_model_cpu.py) or the device
(test_scalar_model_gpu.py).

One COLUMN chunk per return type (ReturnTypeCase):
    column 1   the row number
    column 2   a function id
    then two argument columns per argument type, ARG_TYPES order: a function's i-th argument of
    type t is column arg_attno(t, i).  A row holds grid values in the columns its function reads
    and 1 everywhere else.
One expression per group of functions,
    (case (when (int4eq (var 2 int4) (const int4 K)) (f_K args)) ... (else (const T null)))
so a row evaluates its own function only (CASE is lazy) and what it raises belongs to that function.
"""
import ctypes

import numpy as np

import scalar_model as model
from pg_strom_amd import kds
from pg_strom_amd._lib import lib

ARG_TYPES = ("bool", "int2", "int4", "int8", "float4", "float8", "date", "time", "timestamp", "char1")
FUNCS_PER_PROGRAM = 32


def catalog():
    """every catalog entry: (name, argument type oids, return type oid, flags)"""
    out = []
    for i in range(lib.strom_codegen_catalog_count()):
        name = ctypes.c_char_p()
        args = (ctypes.c_int32 * 4)()
        ret, flags = ctypes.c_int32(0), ctypes.c_int32(0)
        nargs = lib.strom_codegen_catalog_entry(i, ctypes.byref(name), args, ctypes.byref(ret),
                                                ctypes.byref(flags))
        assert nargs != -2, "catalog entry %d has more than STROM_CATALOG_MAX_ARGS arguments" % i
        assert nargs >= 0
        out.append((name.value.decode(), tuple(args[:nargs]), ret.value, flags.value))
    return out


def in_scope_functions():
    """[(name, argument type names, return type name)] of the entries scalar_model covers"""
    out = []
    for name, args, ret, flags in catalog():
        if model.in_scope(name, flags):
            out.append((name, tuple(model.TYPE_OF_OID[a] for a in args), model.TYPE_OF_OID[ret]))
    return out


def arg_attno(t, i):
    return 3 + 2 * ARG_TYPES.index(t) + i


def call_expr(name, argtypes):
    return "(%s%s)" % (name, "".join(" (var %d %s)" % (arg_attno(t, i), t)
                                      for i, t in enumerate(argtypes)))


class ReturnTypeCase(object):
    """the chunk of every in-scope function that returns 'rettype', and the model's outcome per row"""

    def __init__(self, rettype, functions):
        self.rettype = rettype
        self.functions = [f for f in functions if f[2] == rettype]       # function id = index
        fid, args, want = [], [], []
        for k, (name, argtypes, _) in enumerate(self.functions):
            for row in model.rows(name, argtypes):
                fid.append(k)
                args.append(row)
                want.append(model.evaluate(name, argtypes, row))
        if len(fid) % 64 == 0:          # keep a partial last wave, with the NULLs the grids end in
            fid.append(fid[-1]), args.append(args[-1]), want.append(want[-1])
        self.fid = np.array(fid, dtype=np.int32)
        self.args, self.want = args, want
        self.nrows = n = len(fid)
        assert n < 100000 and n % 64 != 0
        cols = [kds.Column("int4", np.arange(n, dtype=np.int32)), kds.Column("int4", self.fid)]
        for t in ARG_TYPES:
            dtype = kds.SQL_TYPES[t][2]
            for i in range(2):
                vals, nulls = np.ones(n, dtype=dtype), np.zeros(n, dtype=np.uint8)
                for r in range(n):
                    at = self.functions[fid[r]][1]
                    if i < len(at) and at[i] == t:
                        if args[r][i] is None:
                            nulls[r] = 1
                        else:
                            vals[r] = args[r][i]
                cols.append(kds.Column(t, vals, nulls))
        self.buf = kds.build_kds("column", cols)
        self.recheck = np.array([w[2] for w in want], dtype=bool)
        self.isnull = np.array([w[1] for w in want], dtype=bool)

    def groups(self):
        """the function ids, FUNCS_PER_PROGRAM at a time: one program each"""
        ids = list(range(len(self.functions)))
        return [ids[i:i + FUNCS_PER_PROGRAM] for i in range(0, len(ids), FUNCS_PER_PROGRAM)]

    def case_expr(self, ids):
        whens = "".join(" (when (int4eq (var 2 int4) (const int4 %d)) %s)" %
                        (k, call_expr(self.functions[k][0], self.functions[k][1])) for k in ids)
        return "(case%s (else (const %s null)))" % (whens, self.rettype)

    def carried_expr(self, ids):
        """case_expr in a form (pmax ..) carries out unchanged: bool through the widening cast
        int4(bool), float4 through float8(float4) -- both exact, both in-scope functions that the
        int4 and float8 cases check directly; every other type as it is"""
        wrap = {"bool": "(int4 %s)", "float4": "(float8 %s)"}.get(self.rettype, "%s")
        return wrap % self.case_expr(ids)

    def rows_of(self, ids):
        return np.flatnonzero(np.isin(self.fid, ids))

    def describe(self, r):
        name, argtypes, _ = self.functions[self.fid[r]]
        return "%s(%s) row %d" % (name, ", ".join("NULL" if a is None else repr(a) for a in self.args[r]), r)

    def check_values(self, rows, images, isnull):
        """the evaluator's 64-bit images / NULL flags of 'rows' against the model; returns the
        descriptions of the rows that differ"""
        bad = []
        for r, img, isn in zip(rows, images, isnull):
            value, want_null, _ = self.want[r]
            name, argtypes, _ = self.functions[self.fid[r]]
            if bool(isn) != want_null:
                bad.append("%s: NULL %s, model %s" % (self.describe(r), bool(isn), want_null))
            elif want_null:
                continue
            elif self.rettype == "float4":          # carried as float8: the widened value, bit for bit
                if not model.same_value((name, argtypes), "float8", np.float64(value), int(img)):
                    bad.append("%s: float8 image 0x%x, model %r" % (self.describe(r), int(img), value))
            elif not model.same_value((name, argtypes), self.rettype, value, int(img)):
                bad.append("%s: 0x%x, model %r" % (self.describe(r), int(img), value))
        return bad


RETURN_TYPES = ("bool", "int2", "int4", "int8", "float4", "float8", "date", "time", "timestamp")
_CASES = {}


def return_type_case(rettype):
    """built once and shared; nobody changes it"""
    if rettype not in _CASES:
        _CASES[rettype] = ReturnTypeCase(rettype, in_scope_functions())
    return _CASES[rettype]
