"""
Consecutive resident GpuScan requests alternate over two streams (csrc/gpuscan.cpp:
gpuscan_launch_resident; STROM_GPUSCAN_SCAN_STREAMS=1 keeps them on one), so the tail of
one scan runs beside the start of the next.  What that must not change: every request's
answer, whichever stream and program it got; the fall to the copied path when the slot ring
is full; and perfmon's kernel time, which is exclusive of the previous scan
(strom_perfmon.time_kern_exec_ns) and so never adds up to more than the wall clock.
Answers come from numpy / torch on seeded data (needs an MI355X: -m gpu).
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from pg_strom_amd import kds, runtime
from pg_strom_amd.gpuscan import GpuScan, STROM_RESULTS_ON_DEVICE

pytestmark = pytest.mark.gpu

C2_QUAL = "(and (int4lt (var 1 int4) (param 0 int4)) (float8gt (var 2 float8) (param 1 float8)))"
# one row; one tile and a row; every work-group of the default grid a tile and one of them two
SIZES = (1, 1025, 1024 * 1024 + 1)
RING_SLOTS = 64                  # Device::SCAN_SLOTS


def table(n, seed):
    """odd sizes carry 5 % NULLs in both columns"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
    b = rng.random(n)
    an = (rng.random(n) < 0.05) if n % 2 == 1 else None
    bn = (rng.random(n) < 0.05) if n % 2 == 1 else None
    return a, b, an, bn


def want_ids(a, b, an, bn, k, c):
    m = (a < k) & (b > c)
    if an is not None:
        m &= ~an
    if bn is not None:
        m &= ~bn
    return np.flatnonzero(m).astype(np.int64) + 1


P10 = (np.int32(2**30), 0.8)             # a < k passes 50 %, b > c 20 % of them: 10 % of the rows
P100 = (np.int32(2**31 - 1), -1.0)       # every row that is not NULL


def upload(data):
    a, b, an, bn = data
    return runtime.DeviceStore.upload(
        kds.build_kds("column", [kds.Column("int4", a, an), kds.Column("float8", b, bn)]))


def many_in_flight_two_programs():
    """12 requests submitted before any is collected: chunk r % 3, session r % 2, results on the
    device for every other pair -- each (chunk, session) goes both ways"""
    runtime.init([0])
    data = [table(n, 4100 + n) for n in SIZES]
    chunks = [upload(d) for d in data]
    sessions = [(GpuScan(C2_QUAL).begin(ext_params=list(p)), p) for p in (P10, P100)]
    want = {(i, j): want_ids(*data[i], *sessions[j][1]) for i in range(len(SIZES)) for j in range(2)}
    assert len(want[(2, 0)]) < len(want[(2, 1)]) // 5        # the two programs differ
    try:
        pend = []
        for r in range(12):
            i, j = r % 3, r % 2
            flags = STROM_RESULTS_ON_DEVICE if (r // 2) % 2 else 0
            pend.append((sessions[j][0].submit(chunks[i], flags=flags), i, j, flags))
        for p, i, j, flags in pend:
            res = sessions[j][0].collect(p)
            assert res.errcode == 0, (i, j, flags, res.errcode)
            assert res.nitems == len(want[(i, j)]), (i, j, flags, res.nitems, len(want[(i, j)]))
            if not flags:
                assert np.array_equal(np.sort(res.results.astype(np.int64)), want[(i, j)]), (i, j)
    finally:
        for s, _ in sessions:
            s.end()
        for ds in chunks:
            ds.release()


@pytest.fixture(scope="module")
def device():
    runtime.init([0])
    yield


def test_many_in_flight_two_programs(device):
    many_in_flight_two_programs()


def test_ring_exhaustion(device):
    """70 requests over the 1025-row chunk, none collected before all are submitted.  They sit
    behind one slow request (40 nested sin() over 1e8 rows), which keeps the completer -- FIFO, it
    gives a slot back when it has seen the request end -- from returning any of the ring's 64 slots
    meanwhile: the first ones take the resident path on alternating streams, the rest the copied
    path on stream 0, and every answer is right.  (The slow program is the one
    test_gpuscan_stream_gpu uses: the suite compiles it once.)"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(31)
    x = torch.rand(100_000_000, dtype=torch.float64, device="cuda", generator=g)
    big = runtime.DeviceStore.from_torch_columns(["float8"], [x])
    del x
    slow_expr = "(var 1 float8)"
    for _ in range(40):
        slow_expr = "(sin %s)" % slow_expr
    slow = GpuScan("(float8gt %s (const float8 2))" % slow_expr).begin()
    slow.program.wait()
    data = table(1025, 4100 + 1025)
    small = upload(data)
    fast = GpuScan(C2_QUAL).begin(ext_params=list(P10))
    fast.program.wait()
    want = want_ids(*data, *P10)
    try:
        head = slow.submit(big, flags=STROM_RESULTS_ON_DEVICE)
        pend = [(fast.submit(small, flags=STROM_RESULTS_ON_DEVICE if r % 2 else 0), r % 2) for r in range(70)]
        res = slow.collect(head)
        assert res.errcode == 0 and res.nitems == 0
        resident = copied = 0
        for p, on_device in pend:
            res = fast.collect(p)
            assert res.errcode == 0 and res.nitems == len(want)
            if not on_device:
                assert np.array_equal(np.sort(res.results.astype(np.int64)), want)
            resident += (res.perfmon["num_dma_send"] == 0)
            copied += (res.perfmon["num_dma_send"] > 0)
        print("resident %d copied %d of 70 (ring: %d slots)" % (resident, copied, RING_SLOTS))
        assert resident >= 1 and copied >= 1, (resident, copied)
    finally:
        slow.end()
        fast.end()
        big.release()
        small.release()


def test_exclusive_kernel_time(device):
    """16 requests back to back over one 32e6-row chunk: with two scans overlapping, a dispatch's
    own begin -> end span covers its predecessor too, and the sum of such spans exceeds the wall
    clock; the exclusive times add up to the span the device was busy, which is within it"""
    import torch
    n = 32_000_000
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    a = torch.randint(0, 2**31, (n,), dtype=torch.int32, device="cuda", generator=g)
    b = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    k, c = P10
    nsel = int(((a < int(k)) & (b > float(c))).sum().item())
    ds = runtime.DeviceStore.from_torch_columns(["int4", "float8"], [a, b])
    scan = GpuScan(C2_QUAL).begin(ext_params=[k, c])
    scan.program.wait()
    try:
        scan.scan_chunk(ds, flags=STROM_RESULTS_ON_DEVICE)      # module load, first touch
        t0 = time.perf_counter_ns()
        pend = [scan.submit(ds, flags=STROM_RESULTS_ON_DEVICE) for _ in range(16)]
        res = [scan.collect(p) for p in pend]
        wall_ns = time.perf_counter_ns() - t0
    finally:
        scan.end()
        ds.release()
    ns = [int(r.perfmon["time_kern_exec_ns"]) for r in res]
    print("wall %.1f us, sum of kernel times %.1f us, each: %s"
          % (wall_ns * 1e-3, sum(ns) * 1e-3, " ".join("%.1f" % (v * 1e-3) for v in ns)))
    assert all(r.errcode == 0 and r.nitems == nsel for r in res)
    assert all(r.perfmon["num_kern_exec"] == 1 and r.perfmon["num_dma_send"] == 0 for r in res)
    assert all(v >= 0 for v in ns)
    assert sum(ns) <= wall_ns, (sum(ns), wall_ns)
    assert max(ns) > 0


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpuscan_overlap_gpu as t
t.many_in_flight_two_programs()
print("ok")
"""


def test_one_scan_stream():
    """the escape hatch: the same requests with every resident scan on stream 0"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, STROM_GPUSCAN_SCAN_STREAMS="1")     # read once, when the device is set up
    out = subprocess.run([sys.executable, "-c", CHILD, root], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]
