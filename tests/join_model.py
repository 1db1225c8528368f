"""
The model of GpuHashJoin's join types (include/strom_hip.h, "Join types"): a nested-loop join in
numpy over small arrays, shared by the CPU and the GPU tests.

For depth d a PREFIX is the outer row plus what depths 1 .. d-1 contributed (an inner row id, or -1
for "no entry").  Per depth the model builds the boolean matrix prefix x entry: every key equal --
a NULL on either side is never equal -- and the qual, a Python callable, true.  The matrix is all
the model knows; the four join types read it as the header's table says:

    inner  the prefix goes on once per candidate, with the entry's row id
    left   ... and once with -1 if it has none
    semi   once with -1 if it has at least one candidate, else not at all
    anti   once with -1 if it has none, else not at all

The result is the exact set of records (outer row + 1, row id or -1 per relation).  A device record
is translated with records_to_rowids(): entry_rowids where the slot is not 0, -1 for a 0 slot.
Both sides are lexsorted and compared exactly.
"""
import numpy as np

from pg_strom_amd.gpuhashjoin import entry_rowids

JOIN_TYPES = ("inner", "left", "semi", "anti")
BLOCK_CELLS = 1 << 25                           # matrix cells per block of prefixes (32 MB of bool)


class Key(object):
    """one hash key: outer(orow, irows) -> (values, isnull) per prefix, where orow is the int
    array of outer rows and irows[d - 1] the inner row ids of depth d (-1: no entry); the inner
    column as (values, isnull or None).  Values compare with ==; a NULL equals nothing."""

    def __init__(self, outer, inner_values, inner_isnull=None):
        self.outer = outer
        self.inner_values = np.asarray(inner_values)
        self.inner_isnull = (np.zeros(len(self.inner_values), dtype=bool) if inner_isnull is None
                             else np.asarray(inner_isnull, dtype=bool))


class Rel(object):
    """one inner relation: nrows entries, its keys, its join type, and its qual -- a callable
    qual(orow, irows, entry) over broadcastable arrays (orow and irows[..] are [n, 1], entry is
    [1, nrows]) that returns True exactly where the ON clause is true (NULL and false: False)"""

    def __init__(self, nrows, keys, jointype="inner", qual=None):
        assert jointype in JOIN_TYPES
        self.nrows = nrows
        self.keys = keys
        self.jointype = jointype
        self.qual = qual


def outer_column(values, isnull=None):
    """the outer(..) of a key that is a plain outer column"""
    values = np.asarray(values)
    isn = np.zeros(len(values), dtype=bool) if isnull is None else np.asarray(isnull, dtype=bool)
    return lambda orow, irows: (values[orow], isn[orow])


def inner_column(depth, values, isnull=None):
    """the outer(..) of a key that is a column of relation `depth`: NULL where the prefix has no
    entry there (a NULL-extended LEFT relation)"""
    values = np.asarray(values)
    isn = np.zeros(len(values), dtype=bool) if isnull is None else np.asarray(isnull, dtype=bool)

    def fn(orow, irows):
        ir = irows[depth - 1]
        none = ir < 0
        at = np.where(none, 0, ir)
        return values[at], isn[at] | none
    return fn


def candidates(rel, orow, irows):
    """(prefix index, entry index) of every candidate, prefix-major, and the count per prefix"""
    npre = len(orow)
    pis, eis = [], []
    step = max(1, BLOCK_CELLS // max(1, rel.nrows))
    keyvals = [k.outer(orow, irows) for k in rel.keys]
    entry = np.arange(rel.nrows)[None, :]
    for lo in range(0, npre, step):
        hi = min(npre, lo + step)
        m = np.ones((hi - lo, rel.nrows), dtype=bool)
        for k, (ov, on) in zip(rel.keys, keyvals):
            eq = np.asarray(ov[lo:hi])[:, None] == k.inner_values[None, :]
            m &= np.asarray(eq, dtype=bool)
            m[np.asarray(on[lo:hi], dtype=bool), :] = False         # a NULL equals nothing
            m[:, k.inner_isnull] = False
        if rel.qual is not None:
            q = rel.qual(orow[lo:hi, None], [ir[lo:hi, None] for ir in irows], entry)
            m &= np.broadcast_to(np.asarray(q, dtype=bool), m.shape)
        pi, ei = np.nonzero(m)
        pis.append(pi + lo)
        eis.append(ei)
    pi = np.concatenate(pis) if pis else np.zeros(0, dtype=np.int64)
    ei = np.concatenate(eis) if eis else np.zeros(0, dtype=np.int64)
    return pi, ei, np.bincount(pi, minlength=npre)


def join_model(outer_rows, rels, memo=None, stats=None):
    """the records of the join of the outer rows `outer_rows` (row ids; a row map's order and
    repeats are kept) with `rels`: int64 [n, 1 + len(rels)] of (outer row + 1, row id or -1 ..).
    memo: a dict that keeps the candidates of depth 1, which do not depend on any join type, for
    the next call over the same data.  stats: a list that receives the candidate count per prefix
    of every depth."""
    orow = np.asarray(outer_rows, dtype=np.int64)
    irows = []
    for d, rel in enumerate(rels, 1):
        if d == 1 and memo is not None and "depth1" in memo:
            pi, ei, cnt = memo["depth1"]
        else:
            pi, ei, cnt = candidates(rel, orow, irows)
            if d == 1 and memo is not None:
                memo["depth1"] = (pi, ei, cnt)
        if stats is not None:
            stats.append(cnt)
        none = np.flatnonzero(cnt == 0)
        if rel.jointype == "inner":
            take, new = pi, ei
        elif rel.jointype == "left":
            take = np.concatenate([pi, none])
            new = np.concatenate([ei, np.full(len(none), -1, dtype=np.int64)])
        elif rel.jointype == "semi":
            take = np.flatnonzero(cnt > 0)
            new = np.full(len(take), -1, dtype=np.int64)
        else:
            take = none
            new = np.full(len(take), -1, dtype=np.int64)
        orow = orow[take]
        irows = [ir[take] for ir in irows] + [np.asarray(new, dtype=np.int64)]
    return np.stack([orow + 1] + irows, axis=1).astype(np.int64).reshape(-1, 1 + len(rels))


def sorted_records(recs):
    recs = np.asarray(recs)
    return recs[np.lexsort(recs.T[::-1])]


def records_to_rowids(device_kmhash, records):
    """device records (outer row + 1, entry offsets) -> the model's form: the entry's row id where
    the slot is not 0, -1 where it is"""
    records = np.asarray(records)
    out = np.empty(records.shape, dtype=np.int64)
    out[:, 0] = records[:, 0]
    for d in range(1, records.shape[1]):
        offs = records[:, d]
        have = offs != 0
        col = np.full(len(offs), -1, dtype=np.int64)
        if have.any():
            col[have] = entry_rowids(device_kmhash, d, offs[have]).astype(np.int64)
        out[:, d] = col
    return out


def prefix_kinds(cnt):
    """does a depth's candidate count per prefix show every kind: none, exactly one, several?"""
    cnt = np.asarray(cnt)
    return bool((cnt == 0).any() and (cnt == 1).any() and (cnt > 1).any())


# ---------------------------------------------------------------------------------------------
# the cases both test files run: the data, the spec for a choice of join types, the model's Rels
# ---------------------------------------------------------------------------------------------
def duplicates_case(nouter=2000, ninner=500, seed=3):
    """one relation on an int4 key: inner keys repeated 1 .. 3 times, NULL keys on both sides"""
    from pg_strom_amd import kds
    rng = np.random.default_rng(seed)
    base = rng.permutation(2 * ninner)[:ninner]
    pk = np.repeat(base, rng.integers(1, 4, ninner))[:ninner].astype(np.int32)
    rng.shuffle(pk)
    pkn = rng.random(ninner) < 0.05
    fk = rng.integers(-5, 2 * ninner + 5, nouter).astype(np.int32)
    fkn = rng.random(nouter) < 0.05
    return dict(pk=pk, pkn=pkn, fk=fk, fkn=fkn,
                inner=kds.build_kds("row_flat", [kds.Column("int4", pk, pkn),
                                                 kds.Column("int4", np.arange(ninner, dtype=np.int32))]),
                outer=lambda fmt="column": kds.build_kds(fmt, [kds.Column("int4", fk, fkn)]))


def one_rel_spec(jointype=None, sqltype="int4"):
    return "(gpuhashjoin (rel (hashkey (var 1 %s) 1 %s)%s))" % (
        sqltype, sqltype, "" if jointype is None else " (jointype %s)" % jointype)


def one_rel_model(case, jointype):
    return [Rel(len(case["pk"]), [Key(outer_column(case["fk"], case["fkn"]), case["pk"], case["pkn"])], jointype)]


PARAM_V2 = 6                                    # (param 0 int2) of the several-relation specs


def general_data(nouter=5000, ninner=300, seed=41):
    """the tables of the several-relation cases: duplicates and NULL keys in every relation"""
    rng = np.random.default_rng(seed)
    d = {}
    # relation 1: (a, b) is the key, c feeds the qual, link is the next relation's key
    d["a"] = rng.integers(0, 60, ninner).astype(np.int32)
    d["an"] = rng.random(ninner) < 0.04
    d["b"] = rng.integers(0, 4, ninner).astype(np.int64)
    d["c"] = rng.random(ninner)
    d["link"] = rng.integers(0, 400, ninner).astype(np.int32)
    d["linkn"] = rng.random(ninner) < 0.05
    # relations 2 and 3: pk is the key, v feeds the qual
    for r in ("2", "3"):
        d["pk" + r] = rng.integers(0, 300, ninner).astype(np.int32)
        d["pk%sn" % r] = rng.random(ninner) < 0.04
        d["v" + r] = rng.integers(0, 9, ninner).astype(np.int16)
    # the outer chunk
    d["fa"] = rng.integers(0, 70, nouter).astype(np.int32)
    d["fan"] = rng.random(nouter) < 0.02
    d["fb"] = rng.integers(0, 4, nouter).astype(np.int16)
    d["fc"] = rng.random(nouter)
    d["fd"] = rng.integers(0, 400, nouter).astype(np.int32)
    d["fdn"] = rng.random(nouter) < 0.03
    return d


def general_chunks(d, fmt):
    """(outer chunk in `fmt`, [relation 1, 2, 3])"""
    from pg_strom_amd import kds
    outer = kds.build_kds(fmt, [kds.Column("int4", d["fa"], d["fan"]), kds.Column("int2", d["fb"]),
                                kds.Column("float8", d["fc"]), kds.Column("int4", d["fd"], d["fdn"])])
    t1 = kds.build_kds("row", [kds.Column("int4", d["a"], d["an"]), kds.Column("int8", d["b"]),
                               kds.Column("float8", d["c"]), kds.Column("int4", d["link"], d["linkn"])])
    t2 = kds.build_kds("row_flat", [kds.Column("int4", d["pk2"], d["pk2n"]), kds.Column("int2", d["v2"])])
    t3 = kds.build_kds("row_flat", [kds.Column("int4", d["pk3"], d["pk3n"]), kds.Column("int2", d["v3"])])
    return outer, [t1, t2, t3]


def _jt(t):
    return "" if t is None else " (jointype %s)" % t


def two_rel_spec(t1, t2):
    """TWO_REL_SPEC of test_hashjoin_edges_gpu.py with a join type per relation (None: not named).
    The second relation is keyed by relation 1's link column where relation 1 exposes columns,
    by the outer column 4 where it is semi / anti."""
    key2 = "(var 4 int4)" if t1 in ("semi", "anti") else "(ivar 1 4 int4)"
    return ("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (hashkey (int8 (var 2 int2)) 2 int8)"
            " (qual (float8gt (ivar 1 3 float8) (var 3 float8)))%s)"
            " (rel%s (hashkey %s 1 int4) (qual (int2lt (ivar 2 2 int2) (param 0 int2)))))" % (_jt(t1), _jt(t2), key2))


def _rel1(d, jointype):
    return Rel(len(d["a"]), [Key(outer_column(d["fa"], d["fan"]), d["a"], d["an"]),
                             Key(outer_column(d["fb"].astype(np.int64)), d["b"])],
               jointype, lambda orow, irows, e: d["c"][e] > d["fc"][orow])


def two_rel_model(d, t1, t2):
    t1, t2 = t1 or "inner", t2 or "inner"
    outer2 = (outer_column(d["fd"], d["fdn"]) if t1 in ("semi", "anti")
              else inner_column(1, d["link"], d["linkn"]))
    return [_rel1(d, t1),
            Rel(len(d["pk2"]), [Key(outer2, d["pk2"], d["pk2n"])], t2,
                lambda orow, irows, e: d["v2"][e] < PARAM_V2)]


THREE_REL_SPEC = ("(gpuhashjoin (rel (jointype left) (hashkey (var 1 int4) 1 int4) (hashkey (int8 (var 2 int2)) 2 int8)"
                  " (qual (float8gt (ivar 1 3 float8) (var 3 float8))))"
                  " (rel (hashkey (ivar 1 4 int4) 1 int4) (jointype semi) (qual (int2lt (ivar 2 2 int2) (param 0 int2))))"
                  " (rel (hashkey (var 4 int4) 1 int4) (qual (int2gt (ivar 3 2 int2) (var 2 int2))) (jointype anti)))")


def three_rel_model(d):
    return [_rel1(d, "left"),
            Rel(len(d["pk2"]), [Key(inner_column(1, d["link"], d["linkn"]), d["pk2"], d["pk2n"])], "semi",
                lambda orow, irows, e: d["v2"][e] < PARAM_V2),
            Rel(len(d["pk3"]), [Key(outer_column(d["fd"], d["fdn"]), d["pk3"], d["pk3n"])], "anti",
                lambda orow, irows, e: d["v3"][e] > d["fb"][orow])]
