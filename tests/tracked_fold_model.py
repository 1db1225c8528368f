"""
The numpy model of a fused lookup or star fold with ONE tracked relation (RIGHT / FULL joins:
strom_submit_gpupreagg_lookup_tracked and _lookup_unmatched, include/strom_hip.h), on top of Dim.partner()
and fold_rule of the existing tests, both imported unchanged.

    result = (fact JOIN the other relations, by their join types) RIGHT | FULL JOIN tracked

- The per-chunk fold is the typed fold: fold_rule over ALL relations, tracked one included (inner: RIGHT,
  left: FULL).  Tracking changes no row of it.
- Row i of the tracked dimension is MATCHED when some fact row of some chunk has it as its partner
  (Dim.partner() == i: key not NULL, inside the range, slot present) and survives every OTHER relation
  (fold_rule over the others).  The WHERE plays no part.
- The unmatched pass emits every other row of the dimension once: the columns the tracked relation serves
  from that row, every other virtual column NULL.

test_lookup_tracked_cpu.py holds matched / unmatched against tests/outer_join_model.py over the nested-loop
join_model, with the tracked relation last.
"""
import numpy as np

from test_lookup_join_types_gpu import fold_rule
from test_star_lookup_gpu import NULLKEY


def others_keep(partners, jointypes, tracked):
    """bool per fact row: kept by every relation but the tracked one (1-based)"""
    rest = [q for q in range(len(partners)) if q != tracked - 1]
    if not rest:
        return np.ones(len(partners[tracked - 1]), dtype=bool)
    return fold_rule([partners[q] for q in rest], [jointypes[q] for q in rest])


def matched_rows(chunks, jointypes, tracked):
    """chunks: [partners of one chunk] (partners[d]: Dim.partner() of relation d + 1) -> the sorted rows of
    the tracked dimension that some fact row matched"""
    seen = [np.zeros(0, dtype=np.int64)]
    for partners in chunks:
        p = partners[tracked - 1]
        seen.append(p[(p >= 0) & others_keep(partners, jointypes, tracked)])
    return np.unique(np.concatenate(seen)).astype(np.int64)


def folded_rows(partners, jointypes):
    """bool per fact row of one chunk: folded by the per-chunk request (before the WHERE)"""
    return fold_rule(partners, jointypes)


def unmatched_rows(dim, matched):
    """the rows of the tracked dimension the unmatched pass emits"""
    return np.setdiff1d(np.arange(dim.nd, dtype=np.int64), matched)


def slot_of(dim, rows):
    """slots of dimension rows in the table's DIRECT index: key - the smallest key"""
    return (dim.key[rows] - dim.key.min()).astype(np.int64)


def matches_image(dim, matched):
    """the flag image of strom_gpupreagg_lookup_matches_fetch: one byte per slot, 1 = matched"""
    img = np.zeros(int(dim.key.max() - dim.key.min()) + 1, dtype=np.uint8)
    img[slot_of(dim, matched)] = 1
    return img


def tracked_model(chunks, dims, jointypes, tracked):
    """(matched rows, [folded mask per chunk], unmatched rows) of the tracked dimension dims[tracked - 1]"""
    matched = matched_rows(chunks, jointypes, tracked)
    return matched, [folded_rows(p, jointypes) for p in chunks], unmatched_rows(dims[tracked - 1], matched)


class Rows(object):
    """virtual joined rows by column: name -> (values, isnull)"""

    def __init__(self, **cols):
        self.cols = {k: (np.asarray(v), np.asarray(n, dtype=bool)) for k, (v, n) in cols.items()}
        self.n = len(next(iter(self.cols.values()))[0]) if self.cols else 0

    def take(self, sel):
        return Rows(**{k: (v[sel], n[sel]) for k, (v, n) in self.cols.items()})

    @staticmethod
    def concat(parts):
        parts = [p for p in parts if p is not None]
        return Rows(**{k: (np.concatenate([p.cols[k][0].astype(np.float64) if p.cols[k][0].dtype.kind == "f"
                                           else p.cols[k][0].astype(np.int64) for p in parts]),
                           np.concatenate([p.cols[k][1] for p in parts])) for k in parts[0].cols})


def served_rows(dim, colno, rows):
    """(values, isnull) of dimension column colno (0-based among dim.cols) for dimension rows"""
    _, v, isn = dim.cols[colno]
    return v[rows], isn[rows]


def null_column(n, dtype=np.int64):
    return np.zeros(n, dtype=dtype), np.ones(n, dtype=bool)


def aggregate(rows, key="key", a="a", b="b", mx=None, mn=None):
    """GROUP BY key: nrows, psum(int8 a), psum(b), [pmax(mx)], [pmin(mn)] over the virtual rows (after the WHERE): a dict
    with the unique keys (NULLKEY for NULL) and per aggregate (values, isnull) -- a sum or a max over no
    non-NULL input is NULL"""
    kv, kn = rows.cols[key]
    keys = np.where(kn, NULLKEY, kv.astype(np.int64))
    uk, inv = (np.unique(keys, return_inverse=True) if len(keys) else (keys, np.zeros(0, dtype=np.int64)))
    inv = inv.reshape(-1)
    ng = len(uk)
    out = {"keys": uk, "nrows": np.bincount(inv, minlength=ng)}
    av, an = rows.cols[a]
    suma = np.zeros(ng, dtype=np.int64)
    np.add.at(suma, inv[~an], av[~an].astype(np.int64))
    out["suma"] = (suma, np.bincount(inv[~an], minlength=ng) == 0)
    bv, bn = rows.cols[b]
    out["sumb"] = (np.bincount(inv[~bn], weights=bv[~bn].astype(np.float64), minlength=ng),
                   np.bincount(inv[~bn], minlength=ng) == 0)
    if mx is not None:
        mv, mxnull = rows.cols[mx]
        wmax = np.full(ng, -np.inf)
        np.maximum.at(wmax, inv[~mxnull], mv[~mxnull].astype(np.float64))
        out["max"] = (wmax, np.isinf(wmax))
    if mn is not None:
        mv, mnull = rows.cols[mn]
        wmin = np.full(ng, np.inf)
        np.minimum.at(wmin, inv[~mnull], mv[~mnull].astype(np.float64))
        out["min"] = (wmin, np.isinf(wmin))
    return out


def check_partial_rows(keys, cols, want):
    """partial rows (test_star_lookup_gpu.partial_rows with one key) against aggregate(): keys, counts,
    integer sums and max bit-exact, float8 sums rtol 1e-12, NULLs where no input was not NULL"""
    assert np.array_equal(keys[:, 0], want["keys"]), (keys[:, 0], want["keys"])
    assert not cols[0][1].any() and np.array_equal(cols[0][0], want["nrows"])
    sa, san = want["suma"]
    assert np.array_equal(cols[1][1], san)
    assert np.array_equal(cols[1][0][~san], sa[~san])
    sb, sbn = want["sumb"]
    assert np.array_equal(cols[2][1], sbn)
    assert np.allclose(cols[2][0][~sbn], sb[~sbn], rtol=1e-12, atol=0)
    if "max" in want:
        mv, mn = want["max"]
        assert np.array_equal(cols[3][1], mn)
        assert np.array_equal(cols[3][0][~mn].astype(np.float64), mv[~mn])
    if "min" in want:
        mv, mn = want["min"]
        assert np.array_equal(cols[4][1], mn)
        assert np.array_equal(cols[4][0][~mn].astype(np.float64), mv[~mn])
