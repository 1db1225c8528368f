"""
bench.py's host-side contract, without a GPU: `--gpus N` must start N ranks itself or fail
loudly (never silently run one rank and print n_gpus: 1), and the CPU-baseline legs
(the oracle timed as PostgreSQL's seqscan / hash join / hash aggregate stand-in) work.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_fails_loudly_when_the_gpus_are_not_there():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this box has the GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 2
    assert "--gpus 2 asked for" in p.stderr
    assert p.stdout.strip() == ""


def test_world_size_must_match_gpus():
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 2 and "WORLD_SIZE=4" in p.stderr


def test_cpu_baseline_legs():
    sys.path.insert(0, ROOT)
    import bench
    k, c = np.int32(2**30), 0.8
    for kind in ("scan", "join", "agg", "chain"):
        r = bench.cpu_baseline(kind, k, c, 0.3)
        assert r["value"] > 0 and r["cores"] == 1 and r["kind"] == "port" and r["unit"] == "Mrows/s"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-worker", "agg,1073741824,0.8,0.3"],
                       capture_output=True, text=True, timeout=300)
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["rows"] > 0 and d["seconds"] > 0


def test_steps_must_be_at_least_one():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr


def test_dump_outputs_from_the_scan_answers(tmp_path):
    """--dump-outputs over stand-in chunks whose answers are known: per-chunk counts and errcodes
    of the last step, id sums, and the seeded sample's flags (1 pass, -1 re-check, 0)"""
    import types
    sys.path.insert(0, ROOT)
    import bench

    class Chunk(object):
        def __init__(self, n, seed):
            rng = np.random.default_rng(seed)
            self.nitems, self.a, self.b = n, rng.integers(0, 2**31, n), rng.random(n)

    class Scan(object):
        def scan_chunk(self, ds):
            ids = np.flatnonzero((ds.a < 2**30) & (ds.b > 0.8)).astype(np.int32) + 1
            ids = np.random.default_rng(0).permutation(ids)     # any order, as the device appends
            ids[:3] = -ids[:3]
            return types.SimpleNamespace(nitems=len(ids), errcode=0, results=ids)

    chunks, scan = [Chunk(300_007, 1), Chunk(200_000, 2), Chunk(777, 3)], Scan()
    last = [(scan.scan_chunk(ds).nitems, 0) for ds in chunks]
    bench.dump_outputs(str(tmp_path), 0, scan, chunks, last)
    got = {n: np.load(str(tmp_path / (n + ".npy")))
           for n in ("nitems", "errcode", "selected_rowid_sum", "sample_rows", "selected_sample")}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["nitems"].tolist() == [n for n, _ in last] and not got["errcode"].any()
    offs = np.cumsum([0] + [ds.nitems for ds in chunks])
    rows = got["sample_rows"].astype(np.int64)
    assert len(rows) == offs[-1] and np.all(np.diff(rows) >= 0)
    want = np.zeros(len(rows), dtype=np.float32)
    for i, ds in enumerate(chunks):
        r = scan.scan_chunk(ds).results.astype(np.int64)
        assert got["selected_rowid_sum"][i] == (np.abs(r) - 1).sum()
        flags = np.zeros(ds.nitems, dtype=np.int8)
        flags[np.abs(r) - 1] = np.sign(r)
        m = (rows >= offs[i]) & (rows < offs[i + 1])
        want[m] = flags[rows[m] - offs[i]]
    assert np.array_equal(got["selected_sample"], want) and (want < 0).any()
    # the same inputs give the same files; a count that differs from the timed step's is refused
    again = tmp_path / "again"
    bench.dump_outputs(str(again), 0, scan, chunks, last)
    assert np.array_equal(np.load(str(again / "sample_rows.npy")), got["sample_rows"])
    import pytest
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "bad"), 0, scan, chunks, [(n + 1, e) for n, e in last])
