"""joined rows with text columns for a device consumer: the COLUMN projection's two passes against the
round trip through heap tuples, and the fixed-width projection on its own.

usage: python scripts/gpu_join_text_projection_probe.py [text|fixed] [label]
  text   (a) join_to_column, one outer character(10) and one inner text column: HIP-event times of the
             sizing and the projection kernel (STROM_HASHJOIN_PROJECT_TIMING, on stderr), wall time
         (b) the same rows as ROW_FLAT heap tuples to the host, uploaded, ingested (to_column)
  fixed  (c) a fixed-width-only projection of the same join; run it from this tree and from the parent
             commit's tree in turns and compare
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash  # noqa: E402

N, ND = 4_000_000, 100_000
MODES = [b"MAIL", b"SHIP", b"TRUCK", b"AIR", b"REG AIR", b"RAIL", b"FOB"]


def tables(with_text):
    """the same keys either way; the text columns only where they are read (4e6 Python objects)"""
    rng = np.random.default_rng(11)
    fk = rng.integers(0, ND, N, dtype=np.int64).astype(np.int32)          # every fact row has its dimension row
    a = rng.integers(0, 2**31, N, dtype=np.int64).astype(np.int32)
    dkey = rng.permutation(ND).astype(np.int32)
    fcols = [kds.Column("int4", fk), kds.Column("int4", a)]
    icols = [kds.Column("int4", dkey), kds.Column("int4", (dkey % 1000).astype(np.int32))]
    if with_text:
        fcols.append(kds.Column("character", [(MODES[i] + b" " * 10)[:10] for i in rng.integers(0, len(MODES), N)]))
        icols.append(kds.Column("text", [b"Customer#%09d" % k for k in dkey]))
    return kds.build_kds("column", fcols), kds.build_kds("row_flat", icols)


def median_ms(fn, repeat=5):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[1:])), ts


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "text"
    label = sys.argv[2] if len(sys.argv) > 2 else "this tree"
    runtime.init()
    fact, inner = tables(what != "fixed")
    ds = runtime.DeviceStore.upload(fact)
    join = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(build_multihash([(inner, [1])]))
    try:
        t_join, _ = median_ms(lambda: join.join_chunk(ds, flags=1))
        if what == "fixed":
            cols = [(1, 2, "int4"), (0, 2, "int4"), (1, 1, "int4")]

            def fixed():
                joined, _ = join.join_to_column(ds, cols)
                joined.release()
            t, ts = median_ms(fixed, 7)
            print("(c) %-10s fixed-width join_to_column %.3f ms (runs %s), join alone %.3f ms"
                  % (label, t, " ".join("%.3f" % x for x in ts[1:]), t_join), flush=True)
            return
        cols = [(0, 2, "int4"), (0, 3, "character"), (1, 3, "text")]
        os.environ["STROM_HASHJOIN_PROJECT_TIMING"] = "1"
        sys.stderr.flush()

        def to_column():
            joined, nitems = join.join_to_column(ds, cols)
            to_column.length = joined.length
            joined.release()
        t_a, ts = median_ms(to_column)
        del os.environ["STROM_HASHJOIN_PROJECT_TIMING"]
        print("(a) join_to_column, %d joined rows, character(10) + text: wall %.3f ms (runs %s), join alone %.3f ms, "
              "result chunk %.1f MB" % (N, t_a, " ".join("%.3f" % x for x in ts[1:]), t_join, to_column.length / 1e6),
              flush=True)

        def round_trip():
            nitems, dest, _ = join.join_chunk_project_rows(ds, cols, data_bytes=72 * N)
            up = runtime.DeviceStore.upload(dest)
            col, _ = up.to_column([kds.column_type_oid(t) for _, _, t in cols])
            col.release()
            up.release()
        t_b, ts = median_ms(round_trip, 3)
        print("(b) join_chunk_project_rows (ROW_FLAT to the host) + upload + to_column: wall %.3f ms (runs %s)"
              % (t_b, " ".join("%.3f" % x for x in ts[1:])), flush=True)
        print("(a) / (b) = %.3f" % (t_a / t_b), flush=True)
    finally:
        join.end()
        ds.release()


if __name__ == "__main__":
    main()
