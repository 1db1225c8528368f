"""
What the fused folds refuse, and with which error code (strom_submit_gpupreagg_lookup, _joined and
_lookup_star; needs an MI355X: -m gpu).

The three calls answer similar faults with different codes -- an outer column index of -1 is
DataStoreCorruption for the one-table calls and BadRequest for the star.  The codes below are the
contract: they were recorded from the calls as they stood before their host code was merged into
one mapping builder, and the builder keeps every one of them.  A refusal launches nothing and
leaves the session usable: after the refusals one good request is folded and compared with numpy
over the joined rows (test_star_lookup_gpu.py's model and bars), whose counts would show a chunk
that had been folded on the way.  The aggregate and the first join are the programs every build
makes ahead, and the one-table lookup folds with the run-time form of its kernel (the form built
FOR a mapping is test_chain_gpu.py's), so that little is compiled here.
"""
import ctypes

import numpy as np
import pytest

from pg_strom_amd import kds, runtime
from pg_strom_amd._lib import lib
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash, STROM_RESULTS_ON_DEVICE
from pg_strom_amd.gpupreagg import GpuPreAgg
from test_star_lookup_gpu import Dim, open_joins, partial_rows, model_groups, check_count_and_sums

pytestmark = pytest.mark.gpu

BAD_REQUEST = 101                               # StromError_BadRequestMessage
CORRUPTION = 300                                # StromError_DataStoreCorruption
DIMREC_MAXCOLS = 16                             # HASHJOIN_DIMREC_MAXCOLS
N = 5003
NGROUPS = 53
SPEC = "(gpupreagg (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))"
# one table -- var 1: the dimension's column 2; var 2, 3: fact columns 3, 4
ONE_COLUMNS = [(1, 2, "int4"), (0, 3, "int4"), (0, 4, "float8")]
# star -- var 1: dimension 1's column 2; var 2: fact column 3; var 3: dimension 2's column 2
STAR_COLUMNS = [(1, 2, "int4"), (0, 3, "int4"), (2, 2, "float8")]
JOIN_ON_1 = "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))"
_WORLD = {}


def world():
    """the dimensions and the fact chunk (host images): computed once, shared, left unchanged"""
    if not _WORLD:
        rng = np.random.default_rng(2917)
        d1 = Dim(rng, 500, key_lo=-70)
        d1.add("int4", (d1.key % NGROUPS).astype(np.int32), rng.random(500) < 0.04)
        d2 = Dim(rng, 400, key_lo=100)
        d2.add("float8", rng.random(400) * 10)
        k1, k1n = d1.fact_keys(rng, N, True)
        k2, k2n = d2.fact_keys(rng, N, True)
        a = rng.integers(0, 2**31, N, dtype=np.int64).astype(np.int32)
        b = rng.random(N)
        k5 = rng.integers(0, 100, N).astype(np.int16)
        cols = [kds.Column("int4", k1, k1n), kds.Column("int4", k2, k2n), kds.Column("int4", a),
                kds.Column("float8", b), kds.Column("int2", k5)]
        dup = Dim(rng, 500)
        dup.key[:50] = dup.key[50:100]                              # duplicate keys
        dup.add("int4", np.arange(500, dtype=np.int32)).add("float8", rng.random(500))
        small = np.arange(80)
        _WORLD.update(d1=d1, d2=d2, k1=k1, k1n=k1n, k2=k2, k2n=k2n, a=a, b=b, dup=dup,
                      fact=kds.build_kds("column", cols), fact_row=kds.build_kds("row", cols),
                      int2_dim=kds.build_kds("row_flat", [kds.Column("int2", small.astype(np.int16)),
                                                          kds.Column("int4", small.astype(np.int32)),
                                                          kds.Column("float8", small * 0.5)]))
    return _WORLD


def compare_with_numpy(pr, partners, float_of=None):
    """the good request's partial rows against numpy over the joined rows: group keys (a NULL key
    is a group), count(*) and the integer sum bit-exact, the float8 sum within rtol 1e-12.
    float_of: (dimension, partner rows) whose last column is summed instead of fact column 4"""
    w = world()
    d1 = w["d1"]
    sel = np.flatnonzero(np.all([p >= 0 for p in partners], axis=0))
    p1 = partners[0][sel]
    uk, inv = model_groups([(d1.cols[0][1][p1], d1.cols[0][2][p1])])
    keys, cols = partial_rows(pr, 1)
    assert len(uk) > 1 and np.array_equal(keys, uk)
    b = w["b"][sel] if float_of is None else float_of[0].cols[-1][1][float_of[1][sel]]
    check_count_and_sums(cols, inv, len(uk), w["a"][sel], b)


class Sessions(object):
    """a dense session, a hashed one and one without a domain, over one program"""

    def __init__(self):
        self.agg = GpuPreAgg(SPEC).begin([(0, NGROUPS)])
        self.hashed = GpuPreAgg(SPEC).begin_hashed()
        err = ctypes.c_int(0)
        pb = ctypes.create_string_buffer(self.agg.parambuf, len(self.agg.parambuf))
        # (the C call with no domain: the first chunk would fix it)
        self.nodomain = lib.strom_gpupreagg_create(self.agg.program.key, self.agg.codegen._targets_c,
                                                   len(self.agg.targets), pb, None, 0, ctypes.byref(err))
        assert self.nodomain

    def end(self):
        lib.strom_gpupreagg_release(self.nodomain)
        self.agg.end()
        self.hashed.end()


def expect(code, call):
    with pytest.raises(runtime.StromError) as ei:
        call()
    print("refused with %d (contract: %d)" % (ei.value.errcode, code))
    assert ei.value.errcode == code, ei.value


@pytest.mark.parametrize("mode", ["lookup", "joined"])
def test_one_table_refusals_keep_their_codes_and_fold_nothing(mode, monkeypatch):
    monkeypatch.setenv("STROM_GPUPREAGG_LOOKUP_GENERIC", "1")
    runtime.init()
    w = world()
    d1 = w["d1"]
    ds = runtime.DeviceStore.upload(w["fact"])
    ds_row = runtime.DeviceStore.upload(w["fact_row"])
    joins = []

    def table(spec, dim_chunk):
        joins.append(GpuHashJoin(spec).begin(build_multihash([(dim_chunk, [1])])))
        return joins[-1]

    join = table(JOIN_ON_1, d1.chunk())
    j_dup = table(JOIN_ON_1, w["dup"].chunk())
    j_qual = table("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (qual (int4lt (var 3 int4) (const int4 5)))))",
                   d1.chunk())
    j_int2 = table("(gpuhashjoin (rel (hashkey (var 5 int2) 1 int2)))", w["int2_dim"])
    assert join.table_info(1)["mode"] == "direct" and join.table_info(1)["unique"]
    assert not j_dup.table_info(1)["unique"]
    s = Sessions()
    agg = s.agg

    def refused(code, columns, j=join, owner=agg, session=None, store=ds, flags=STROM_RESULTS_ON_DEVICE):
        saved = owner.session
        if session is not None:
            owner.session = session
        try:
            if mode == "lookup":
                expect(code, lambda: owner.submit_lookup(j, store, columns))
            else:
                jp = j.submit(store, flags=flags)
                try:
                    expect(code, lambda: owner.submit_joined(j, jp, store, columns))
                finally:
                    j.collect(jp)                   # (a refused request leaves the join's task to its owner)
        finally:
            owner.session = saved

    try:
        refused(BAD_REQUEST, [])                                            # ncols 0
        refused(BAD_REQUEST, ONE_COLUMNS + [(0, 3, "int4")] * (65 - len(ONE_COLUMNS)))    # ncols 65
        refused(BAD_REQUEST, [(2, 2, "int4")] + ONE_COLUMNS[1:])            # a depth of 2
        refused(BAD_REQUEST, [(-1, 2, "int4")] + ONE_COLUMNS[1:])           # a depth of -1
        refused(CORRUPTION, [ONE_COLUMNS[0], (0, 0, "int4")] + ONE_COLUMNS[2:])   # outer column index -1
        refused(CORRUPTION, [ONE_COLUMNS[0], (0, 6, "int4")] + ONE_COLUMNS[2:])   # ... one past the chunk
        refused(CORRUPTION, [ONE_COLUMNS[0], (0, 3, "float8")] + ONE_COLUMNS[2:])  # int4 column named float8
        refused(BAD_REQUEST, ONE_COLUMNS, j=j_dup)                          # duplicate keys
        refused(BAD_REQUEST, ONE_COLUMNS, owner=s.hashed)                   # a hashed session
        refused(BAD_REQUEST, ONE_COLUMNS, session=s.nodomain)               # a session without a domain
        refused(BAD_REQUEST, ONE_COLUMNS, store=ds_row)                     # an outer store in ROW format
        refused(BAD_REQUEST, ONE_COLUMNS + [(1, 2, "int4")] * DIMREC_MAXCOLS)     # 1 + 16 inner columns
        if mode == "lookup":
            # only the aggregate's program runs: a WHERE pulled up into the join program would be lost
            refused(BAD_REQUEST, ONE_COLUMNS, j=j_qual)
            refused(BAD_REQUEST, ONE_COLUMNS, j=j_int2)                     # a 2-byte join key
        else:
            refused(BAD_REQUEST, ONE_COLUMNS, flags=0)                      # a join without device results
        # nothing was folded (the counts below would show it), and the session still works
        if mode == "lookup":
            assert agg.collect(agg.submit_lookup(join, ds, ONE_COLUMNS))[0] == 0
        else:
            jp = join.submit(ds, flags=STROM_RESULTS_ON_DEVICE)
            assert agg.collect(agg.submit_joined(join, jp, ds, ONE_COLUMNS))[0] == 0
            assert join.collect(jp).errcode == 0
        pr = agg.fetch()
    finally:
        s.end()
        for j in joins:
            j.end()
        ds.release()
        ds_row.release()
    p1 = d1.partner(w["k1"], w["k1n"])
    compare_with_numpy(pr, [p1])


def test_star_refusals_with_a_code_of_their_own():
    """the star's DataStoreCorruption paths (test_star_lookup_gpu.py has its BadRequest ones), and
    the outer column index of -1 that the one-table calls answer differently"""
    runtime.init()
    w = world()
    d1, d2 = w["d1"], w["d2"]
    ds = runtime.DeviceStore.upload(w["fact"])
    joins = open_joins([d1, d2], [1, 2])
    agg = GpuPreAgg(SPEC).begin([(0, NGROUPS)])
    try:
        expect(CORRUPTION, lambda: agg.submit_lookup_star(joins, ds, [STAR_COLUMNS[0], (0, 6, "int4")] + STAR_COLUMNS[2:]))
        expect(CORRUPTION, lambda: agg.submit_lookup_star(joins, ds, [STAR_COLUMNS[0], (0, 3, "float8")] + STAR_COLUMNS[2:]))
        expect(BAD_REQUEST, lambda: agg.submit_lookup_star(joins, ds, [STAR_COLUMNS[0], (0, 0, "int4")] + STAR_COLUMNS[2:]))
        expect(BAD_REQUEST, lambda: agg.submit_lookup_star(joins, ds, STAR_COLUMNS + [(1, 2, "int4")] * DIMREC_MAXCOLS))
        assert agg.collect(agg.submit_lookup_star(joins, ds, STAR_COLUMNS))[0] == 0
        pr = agg.fetch()
    finally:
        agg.end()
        for j in joins:
            j.end()
        ds.release()
    p1, p2 = d1.partner(w["k1"], w["k1n"]), d2.partner(w["k2"], w["k2n"])
    compare_with_numpy(pr, [p1, p2], float_of=(d2, p2))
