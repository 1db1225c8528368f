"""
GpuScan over resident COLUMN chunks (gpuscan_qual_column_resident): the
request travels as the kernel argument and the kernel publishes its own
result head through a slot of the device's ring.  Checked against numpy on
seeded data (needs an MI355X: -m gpu).  A request on that path moves no
copy: perfmon num_dma_send == 0 tells it from the copied path.

Not covered: a significant per-row error.  Programs on this path take their
parameters by value, and no by-value qual raises one (rows that cannot be
decided go back to the CPU as CpuReCheck); text / character(n) programs,
whose datums can be found corrupt, take the copied path.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as oracle
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuscan import GpuScan, STROM_RESULTS_ON_DEVICE

pytestmark = pytest.mark.gpu

C2_QUAL = "(and (int4lt (var 1 int4) (param 0 int4)) (float8gt (var 2 float8) (param 1 float8)))"
TILE = 1024                      # GPUSCAN_BLOCK * 4 * GPUSCAN_QUADS (defaults)
GRID_TILES = 256 * 4             # work-groups of one launch at the default geometry on MI355X


def table(n, seed, nulls=False):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    b = rng.random(n)
    an = (rng.random(n) < 0.05) if nulls else None
    bn = (rng.random(n) < 0.05) if nulls else None
    return a, b, an, bn


def params(sel):
    """(k, c) with a < k passing 50 % and b > c the rest: sel of the rows overall"""
    if sel == 0.0:
        return np.int32(-1), 2.0
    if sel == 1.0:
        return np.int32(2**31 - 1), -1.0
    return np.int32(2**30), 1.0 - 2 * sel


def want_ids(a, b, an, bn, k, c):
    m = (a < k) & (b > c)
    if an is not None:
        m &= ~an
    if bn is not None:
        m &= ~bn
    return np.flatnonzero(m).astype(np.int64) + 1


def run(scan, ds, flags=0):
    return scan.scan_chunk(ds, flags=flags)


@pytest.fixture(scope="module")
def device():
    runtime.init([0])
    yield


SIZES = sorted({1, 3, 4, 5, 1023, 1024, 1025,
                GRID_TILES * TILE - 1, GRID_TILES * TILE, GRID_TILES * TILE + 1})


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sel", [0.0, 0.1, 1.0])
def test_sizes_and_selectivity(device, n, sel):
    nulls = (n % 2 == 1)
    a, b, an, bn = table(n, 1000 + n, nulls)
    k, c = params(sel)
    buf = kds.build_kds("column", [kds.Column("int4", a, an), kds.Column("float8", b, bn)])
    ds = runtime.DeviceStore.upload(buf)
    scan = GpuScan(C2_QUAL).begin(ext_params=[k, c])
    try:
        want = want_ids(a, b, an, bn, k, c)
        res = run(scan, ds)
        assert res.errcode == 0 and res.nitems == len(want)
        assert np.array_equal(np.sort(res.results.astype(np.int64)), want)
        assert res.perfmon["num_dma_send"] == 0                   # the resident kernel ran
        res = run(scan, ds, STROM_RESULTS_ON_DEVICE)
        assert res.errcode == 0 and res.nitems == len(want)
        assert res.perfmon["num_kern_exec"] == 1 and res.perfmon["time_kern_exec_ns"] > 0
        assert res.perfmon["num_dma_send"] == 0
    finally:
        scan.end()
        ds.release()


def test_stage_flush_boundaries(device):
    """one work-group per CU and every row selected: a work-group's stage (8192 entries) is
    flushed before its 8th tile of 1024 rows, so 7 tiles per work-group need no flush inside
    the walk, one row more needs one, 14 tiles and one row need two"""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    old = os.environ.get("STROM_GPUSCAN_BLOCKS_PER_CU")
    os.environ["STROM_GPUSCAN_BLOCKS_PER_CU"] = "1"          # host policy, read at every launch
    try:
        for n in (7 * ncu * TILE - 1, 7 * ncu * TILE, 7 * ncu * TILE + 1, 14 * ncu * TILE + 1):
            a, b, _, _ = table(n, n)
            k, c = params(1.0)
            ds = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", a), kds.Column("float8", b)]))
            scan = GpuScan(C2_QUAL).begin(ext_params=[k, c])
            try:
                res = run(scan, ds)
            finally:
                scan.end()
                ds.release()
            assert res.errcode == 0 and res.nitems == n and res.perfmon["num_dma_send"] == 0
            assert np.array_equal(np.sort(res.results.astype(np.int64)), np.arange(1, n + 1))
    finally:
        if old is None:
            del os.environ["STROM_GPUSCAN_BLOCKS_PER_CU"]
        else:
            os.environ["STROM_GPUSCAN_BLOCKS_PER_CU"] = old


def test_full_chunk_1e8(device):
    n = 100_000_000
    a, b, _, _ = table(n, 7)
    k, c = params(0.1)
    buf = kds.build_kds("column", [kds.Column("int4", a), kds.Column("float8", b)])
    ds = runtime.DeviceStore.upload(buf)
    del buf
    scan = GpuScan(C2_QUAL).begin(ext_params=[k, c])
    try:
        res = run(scan, ds)
        res2 = run(scan, ds, STROM_RESULTS_ON_DEVICE)
    finally:
        scan.end()
        ds.release()
    want = want_ids(a, b, None, None, k, c)
    assert res.errcode == 0 and res.nitems == len(want) == res2.nitems
    assert np.array_equal(np.sort(res.results.astype(np.int64)), want)


def oracle_check(qual, buf, ds, ext=()):
    rc_o, res_o = oracle.gpuscan(qual, buf, ext)
    scan = GpuScan(qual).begin(ext_params=ext)
    try:
        res = run(scan, ds)
    finally:
        scan.end()
    assert res.errcode == rc_o
    assert res.nitems == len(res_o)
    assert np.array_equal(np.sort(res.results), np.sort(np.asarray(res_o, dtype=np.int32)))
    return res


def test_recheck_rows_and_nan(device):
    rng = np.random.default_rng(6)
    n = 70001
    a = rng.integers(2**31 - 50, 2**31, n, dtype=np.int64).astype(np.int32)
    d = rng.random(n) * 6e9 - 3e9
    d[::97] = np.nan
    d[::101] = np.inf
    buf = kds.build_kds("column", [kds.Column("int4", a), kds.Column("float8", d)])
    ds = runtime.DeviceStore.upload(buf)
    try:
        res = oracle_check("(int4gt (int4pl (var 1 int4) (const int4 25)) (const int4 0))", buf, ds)
        assert len(res.recheck_rows()) > 1000 and len(res.passed_rows()) > 1000
        oracle_check("(float8gt (var 2 float8) (const float8 1e300))", buf, ds)
        oracle_check("(int4gt (int4 (var 2 float8)) (const int4 0))", buf, ds)
    finally:
        ds.release()


def test_rows_to_recheck_then_cursor_reset(device):
    rng = np.random.default_rng(9)
    n = 50000
    x = rng.random(n) * 2 - 1.0                   # ln of a negative value: the row goes back to the CPU
    buf = kds.build_kds("column", [kds.Column("float8", x), kds.Column("float8", x)])
    ds = runtime.DeviceStore.upload(buf)
    try:
        res = oracle_check("(float8gt (ln (var 1 float8)) (const float8 -1))", buf, ds)
        assert len(res.recheck_rows()) > 1000
        # the next request on the same ring slot starts with a zero cursor
        res = oracle_check("(float8gt (var 1 float8) (const float8 0))", buf, ds)
        assert res.errcode == 0 and res.nitems == int(np.count_nonzero(x > 0))
    finally:
        ds.release()


def test_many_requests_in_flight(device):
    """windows 1..8 and 100, two scans with different parameters interleaved; every request's
    nitems and errcode are checked"""
    chunks, data = [], []
    for i in range(6):
        a, b, an, bn = table(30000 + 777 * i, 300 + i, nulls=(i % 2 == 1))
        chunks.append(runtime.DeviceStore.upload(
            kds.build_kds("column", [kds.Column("int4", a, an), kds.Column("float8", b, bn)])))
        data.append((a, b, an, bn))
    p1, p2 = params(0.1), params(0.4)
    s1 = GpuScan(C2_QUAL).begin(ext_params=list(p1))
    s2 = GpuScan(C2_QUAL).begin(ext_params=list(p2))
    try:
        for window in (1, 2, 3, 8, 100):
            pend = []
            for r in range(90 if window == 100 else 12):
                i = r % len(chunks)
                scan, p = (s1, p1) if r % 2 == 0 else (s2, p2)
                flags = STROM_RESULTS_ON_DEVICE if r % 3 == 0 else 0
                pend.append((scan.submit(chunks[i], flags=flags), scan, i, p, flags))
                while len(pend) > window:
                    check_pending(pend.pop(0), data)
            while pend:
                check_pending(pend.pop(0), data)
    finally:
        s1.end()
        s2.end()
        for ds in chunks:
            ds.release()


def check_pending(item, data):
    pending, scan, i, (k, c), flags = item
    res = scan.collect(pending)
    want = want_ids(*data[i], k, c)
    assert res.errcode == 0 and res.nitems == len(want)
    if not flags:
        assert np.array_equal(np.sort(res.results.astype(np.int64)), want)


def test_rowmap_then_mapped_scan(device):
    n = 200003
    a, b, _, _ = table(n, 55)
    k, c = params(0.3)
    buf = kds.build_kds("column", [kds.Column("int4", a), kds.Column("float8", b)])
    ds = runtime.DeviceStore.upload(buf)
    s1 = GpuScan(C2_QUAL).begin(ext_params=[k, c])
    s2 = GpuScan(C2_QUAL).begin(ext_params=[np.int32(2**29), 0.9])
    try:
        rmap, res = s1.scan_to_rowmap(ds)
        first = want_ids(a, b, None, None, k, c)
        assert res.errcode == 0 and res.nitems == len(first) == rmap.nvalids
        res2 = s2.scan_chunk(ds, row_map=rmap)
        m = (a[first - 1] < 2**29) & (b[first - 1] > 0.9)
        assert res2.errcode == 0
        assert np.array_equal(np.sort(res2.results.astype(np.int64)), np.sort(first[m]))
        rmap.release()
    finally:
        s1.end()
        s2.end()
        ds.release()


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuscan import GpuScan, STROM_RESULTS_ON_DEVICE
runtime.init([0])
Q = "(and (int4lt (var 1 int4) (param 0 int4)) (float8gt (var 2 float8) (param 1 float8)))"
for n, nulls in ((1, False), (4097, True), (1000003, False), (2500001, True)):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    b = rng.random(n)
    an = (rng.random(n) < 0.05) if nulls else None
    m = (a < 2**30) & (b > 0.6)
    if nulls:
        m &= ~an
    ds = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", a, an), kds.Column("float8", b)]))
    scan = GpuScan(Q).begin(ext_params=[np.int32(2**30), 0.6])
    res = scan.scan_chunk(ds)
    res2 = scan.scan_chunk(ds, flags=STROM_RESULTS_ON_DEVICE)
    scan.end()
    ds.release()
    assert res.errcode == 0 and res2.errcode == 0, (n, res.errcode)
    assert res.nitems == res2.nitems == int(m.sum()), (n, res.nitems, int(m.sum()))
    assert np.array_equal(np.sort(res.results.astype(np.int64)), np.flatnonzero(m) + 1), n
print("ok")
"""


@pytest.mark.parametrize("knobs", [
    {"STROM_GPUSCAN_BLOCK": "128"},
    {"STROM_GPUSCAN_BLOCK": "512"},
    {"STROM_GPUSCAN_QUADS": "2"},
    {"STROM_GPUSCAN_STAGE": "2048"},
    {"STROM_GPUSCAN_STAGE": "8192", "STROM_GPUSCAN_BLOCKS_PER_CU": "3"},
    {"STROM_GPUSCAN_BLOCKS_PER_CU": "1"},
], ids=lambda d: ",".join("%s=%s" % (k[len("STROM_GPUSCAN_"):], v) for k, v in d.items()))
def test_geometry_knobs(knobs):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **knobs)      # compile-time values of the program and launch values of the host
    out = subprocess.run([sys.executable, "-c", CHILD, root], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]


def test_full_ring_falls_back_to_the_copied_path(device):
    """a slow request first (40 nested sin() over 1e8 rows) holds the scan stream while 100
    small requests queue behind it: the ring's 64 slots run out, the rest take the copied
    path, and every request is right"""
    n = 100_000_000
    x = np.random.default_rng(31).random(n)
    big = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("float8", x)]))
    del x
    slow_expr = "(var 1 float8)"
    for _ in range(40):
        slow_expr = "(sin %s)" % slow_expr
    slow = GpuScan("(float8gt %s (const float8 2))" % slow_expr).begin()
    slow.program.wait()
    a, b, an, bn = table(1000, 5, nulls=True)
    small = runtime.DeviceStore.upload(
        kds.build_kds("column", [kds.Column("int4", a, an), kds.Column("float8", b, bn)]))
    k, c = params(0.4)
    fast = GpuScan(C2_QUAL).begin(ext_params=[k, c])
    fast.program.wait()
    try:
        head = slow.submit(big, flags=STROM_RESULTS_ON_DEVICE)
        pend = [(fast.submit(small, flags=STROM_RESULTS_ON_DEVICE if r % 2 else 0), r % 2) for r in range(100)]
        res = slow.collect(head)
        assert res.errcode == 0 and res.nitems == 0
        want = want_ids(a, b, an, bn, k, c)
        copied = 0
        for p, on_device in pend:
            res = fast.collect(p)
            assert res.errcode == 0 and res.nitems == len(want)
            if not on_device:
                assert np.array_equal(np.sort(res.results.astype(np.int64)), want)
            copied += (res.perfmon["num_dma_send"] > 0)
        assert 0 < copied < 100, copied
    finally:
        slow.end()
        fast.end()
        big.release()
        small.release()
