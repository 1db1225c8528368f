"""The text key dictionary in front of GpuPreAgg (strom_textdict_*) over the table of
gpu_textjoin_probe.py -- 14-byte text keys in a COLUMN chunk -- for the record:
  (a) the first encode, every key new       (probe + settle + emit + rebuilds, device events)
  (b) a repeat encode, the steady state     (median of 5 after one warm-up, device events)
  (c) in the same run: the text-key join and the texteq scan of gpu_textjoin_probe.py
  (d) the whole group_by_text next to an int4-key GROUP BY of the same rows (host clock around
      blocking calls)
The steady-state probe does per row what the text-key join does -- hash, one table probe, one byte
compare -- so (c)'s join time is the yardstick for (b).  No pass / fail rests on a time.
usage: gpu_textdict_probe.py [rows] [distinct keys ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pg_strom_amd import kds, runtime
from pg_strom_amd._lib import lib
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpupreagg import GpuPreAgg
from pg_strom_amd.gpuscan import GpuScan
from pg_strom_amd.textdict import TextDictionary, group_by_text

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000
distincts = [int(float(a)) for a in sys.argv[2:]] or [100_000, 100, 1_000_000]
runtime.init()
SPEC = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)))"


def us(ns):
    return ns * 1e-3


for nd in distincts:
    rng = np.random.default_rng(1)
    pick = rng.integers(0, nd, n)
    t0 = time.perf_counter()
    otxt = [b"cust#%09d" % i for i in pick]
    v = np.arange(n, dtype=np.int64)
    outer = kds.build_kds("column", [kds.Column("text", otxt), kds.Column("int8", v)])
    print("== %d rows, %d distinct 14-byte keys; COLUMN chunk %.1f MB, built in %.1f s"
          % (n, nd, len(outer) / 1e6, time.perf_counter() - t0), flush=True)
    ds = runtime.DeviceStore.upload(outer)
    d = TextDictionary("text")
    # (a) first encode
    enc = d.encode(ds, [0], [1])
    k = d.kernel_ns()
    assert d.num_keys == len(np.unique(pick))
    print("(a) first encode   probe %8.1f us (all probes of the call)  settle %7.1f  emit %7.1f  rebuild %7.1f   -> %d keys"
          % (us(k["probe"]), us(k["settle"]), us(k["emit"]), us(k["rebuild"]), d.num_keys), flush=True)
    ids0 = kds.decode_column_chunk(enc.download())[0]["values"].copy()
    enc.release()
    hinted = TextDictionary("text", nkeys_hint=nd)
    enc = hinted.encode(ds, [0], [1])
    k = hinted.kernel_ns()
    print("(a) ... nkeys_hint=%d: probe %8.1f us  settle %7.1f  emit %7.1f  rebuild %7.1f"
          % (nd, us(k["probe"]), us(k["settle"]), us(k["emit"]), us(k["rebuild"])), flush=True)
    enc.release()
    hinted.release()
    # (b) steady state
    ts = {"probe": [], "emit": [], "settle": [], "rebuild": []}
    for it in range(6):
        enc = d.encode(ds, [0], [1])
        k = d.kernel_ns()
        if it:
            for name in ts:
                ts[name].append(us(k[name]))
        if it == 5:
            assert np.array_equal(kds.decode_column_chunk(enc.download())[0]["values"], ids0)
        enc.release()
    p = np.median(ts["probe"])
    print("(b) repeat encode  probe %8.1f us  %.2f Grows/s (min %.1f max %.1f)   emit %7.1f us   settle %.1f rebuild %.1f"
          % (p, n / p / 1e3, min(ts["probe"]), max(ts["probe"]), np.median(ts["emit"]),
             np.median(ts["settle"]), np.median(ts["rebuild"])), flush=True)
    # (c) the yardsticks of gpu_textjoin_probe.py, same chunk
    words = [b"cust#%09d" % i for i in range(nd)]
    inner = kds.build_kds("row_flat", [kds.Column("text", words), kds.Column("int4", np.arange(nd, dtype=np.int32))])
    join = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 text) 1 text)))", row_population_ratio=1.05).begin(
        build_multihash([(inner, [1])]))
    tj = []
    for _ in range(6):
        r = join.join_chunk(ds, flags=1)
        assert r.nitems == n
        tj.append(us(r.perfmon["time_kern_exec_ns"]))
    print("(c) join on text key %8.1f us  %.2f Grows/s  index %s" % (np.median(tj[1:]), n / np.median(tj[1:]) / 1e3,
                                                                    join.table_info()["mode"]), flush=True)
    join.end()
    scan = GpuScan("(texteq (var 1 text) (const text 'cust#000000042'))").begin()
    tsn = []
    for _ in range(6):
        r = scan.scan_chunk(ds)
        tsn.append(us(r.perfmon["time_kern_exec_ns"]))
    print("(c) scan texteq      %8.1f us  %.2f Grows/s" % (np.median(tsn[1:]), n / np.median(tsn[1:]) / 1e3), flush=True)
    scan.end()
    # (d) whole GROUP BY: text key through the dictionary, int4 key directly
    ichunk = None
    try:
        tg = []
        for _ in range(4):
            lib.strom_synchronize()
            t0 = time.perf_counter()
            pr, keycols = group_by_text([ds], [(0, "text")], SPEC, [1], hashed=(nd > 160000))  # dense slots end there
            tg.append((time.perf_counter() - t0) * 1e6)
        assert len(pr) == d.num_keys and int(pr.column(1)[0].sum()) == n
        ichunk = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", pick.astype(np.int32)), kds.Column("int8", v)]))
        ti = []
        for _ in range(4):
            lib.strom_synchronize()
            t0 = time.perf_counter()
            agg = GpuPreAgg(SPEC).begin_hashed(ngroups_hint=nd) if nd > 160000 else GpuPreAgg(SPEC).begin([(0, nd)])
            assert agg.fold(ichunk)[0] == 0
            pi = agg.fetch()
            agg.end()
            ti.append((time.perf_counter() - t0) * 1e6)
        assert len(pi) == len(pr)
        print("(d) group_by_text    %8.1f us (new dictionary each time: first encode, session, fold, fetch, keys)   int4 key GROUP BY %8.1f us"
              % (np.median(tg[1:]), np.median(ti[1:])), flush=True)
    except runtime.StromError as e:
        print("(d) not run at this key count: %s" % e, flush=True)
    if ichunk is not None:
        ichunk.release()
    d.release()
    ds.release()
