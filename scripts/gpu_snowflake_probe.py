"""fact JOIN d1 JOIN d2 (d2 keyed by d1.x) WHERE ... GROUP BY d2.g over a resident fact chunk, three ways:
  (a) the snowflake lookup (strom_submit_gpupreagg_lookup_snowflake): d2 joined into d1's slot records
      once, then the one-table lookup kernel
  (b) the plan that exists without it: the two-relation general join with an (ivar ..) key, the COLUMN
      projection (strom_hashjoin_project_column), then the plain fold of the joined chunk
  (c) the floor: the one-table lookup (strom_submit_gpupreagg_lookup) on d1 serving a d1 column of the
      same narrow width
fact(k1 int4, a int4, b float8), d1 of 1e6 rows, d2 of 1e4 rows, 1000 groups, a WHERE that keeps ~50 %, a
match rate of ~80 % per step.  One process, the three alternating, warm programs, three repetitions each.
(a) and (c): the fold kernel's device events (perfmon) and wall clock; (b): wall clock around join +
projection + fold, and the device events of its fold.  The one-off flattening is timed apart: a NEW d2
table of the same rows (d1's own records and every program warm) makes the first request build d2's
records, compose them into d1's and make the narrow form; that request's wall time over a warm one's.
Asserts that (a)'s partial rows equal (b)'s.  Writes profiles/snowflake_lookup_probe.txt.
usage: gpu_snowflake_probe.py [nrows] [nd1] [nd2] [outfile]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd._lib import lib  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash  # noqa: E402
from pg_strom_amd.gpupreagg import GpuPreAgg  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
nd1 = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
nd2 = int(float(sys.argv[3])) if len(sys.argv) > 3 else 10_000
outfile = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "snowflake_lookup_probe.txt")
REPS = 3
NGROUPS = 1000
QUAL = "(and (int4lt (var 2 int4) (param 0 int4)) (float8gt (var 3 float8) (param 1 float8)))"
EXT = [np.int32(2**30 - 1), 0.0]                # a < 2^30 of [0, 2^31): 50 %
SPEC = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def rows_of(pr):
    keys = np.where(pr.column(0)[1], 10**9, pr.column(0)[0].astype(np.int64))
    order = np.argsort(keys)
    return [keys[order]] + [pr.column(c)[0][order] for c in range(1, len(pr.targets))]


def fmt(v):
    return "[" + " ".join("%.3f" % x for x in v) + "]"


runtime.init()
rng = np.random.default_rng(17)
span1, span2 = int(nd1 * 1.25), int(nd2 * 1.25)     # 80 % of the keys have a partner, at either step
k1 = rng.integers(0, span1, n, dtype=np.int64).astype(np.int32)
a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
b = rng.random(n)
fact = kds.build_kds("column", [kds.Column("int4", k1), kds.Column("int4", a), kds.Column("float8", b)])
del k1, a, b
ds = runtime.DeviceStore.upload(fact)
del fact
say("snowflake lookup probe: %d fact rows, d1 %d rows (key span %d) -> d2 %d rows (key span %d), %d groups, "
    "WHERE keeps 50 %%, %d repetitions" % (n, nd1, span1, nd2, span2, NGROUPS, REPS))
dk1 = rng.permutation(span1)[:nd1].astype(np.int32)
dk2 = rng.permutation(span2)[:nd2].astype(np.int32)
# d1(key, g1, x): g1 as wide as d2.g, x over d2's key span; d2(key, g)
in1 = kds.build_kds("row_flat", [kds.Column("int4", dk1), kds.Column("int4", (dk1 % NGROUPS).astype(np.int32)),
                                 kds.Column("int4", rng.integers(0, span2, nd1).astype(np.int32))])
in2 = kds.build_kds("row_flat", [kds.Column("int4", dk2), kds.Column("int4", (dk2 % NGROUPS).astype(np.int32))])
J1 = "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))"
J2 = "(gpuhashjoin (rel (hashkey (var 3 int4) 1 int4)))"          # var 3 of d1: the parent is its outer relation
j1 = GpuHashJoin(J1).begin(build_multihash([(in1, [1])]))
j2 = GpuHashJoin(J2).begin(build_multihash([(in2, [1])]))
both = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)) (rel (hashkey (ivar 1 3 int4) 1 int4)))")
both.begin(build_multihash([(in1, [1]), (in2, [1])]))
snow_cols = [(2, 2, "int4"), (0, 2, "int4"), (0, 3, "float8")]
floor_cols = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8")]
snow = GpuPreAgg(SPEC).begin([(0, NGROUPS)], ext_params=EXT)
plain = GpuPreAgg(SPEC).begin([(0, NGROUPS)], ext_params=EXT)
floor = GpuPreAgg(SPEC).begin([(0, NGROUPS)], ext_params=EXT)
t = {"a_wall": [], "a_dev": [], "b_wall": [], "b_fold_dev": [], "c_wall": [], "c_dev": []}
packed = {}


def run_snowflake(child):
    snow.reset()
    lib.strom_synchronize()
    t0 = time.perf_counter()
    st, pfm = snow.collect(snow.submit_lookup_snowflake([j1, child], [0, 1], ds, snow_cols, [None, "int4"]))
    t1 = time.perf_counter()
    assert st == 0
    return (t1 - t0) * 1e3, pfm


for rep in range(-1, REPS):                     # (rep -1 warms programs, tables and slot records)
    wall_a, pfm = run_snowflake(j2)
    packed["a"] = pfm["num_kern_prep"]
    rows_a = rows_of(snow.fetch())

    plain.reset()
    lib.strom_synchronize()
    t2 = time.perf_counter()
    joined, nitems = both.join_to_column(ds, snow_cols)
    st, pfm_b = plain.fold(joined)
    t3 = time.perf_counter()
    assert st == 0
    joined.release()
    rows_b = rows_of(plain.fetch())

    floor.reset()
    lib.strom_synchronize()
    t4 = time.perf_counter()
    st, pfm_c = floor.collect(floor.submit_lookup(j1, ds, floor_cols))
    t5 = time.perf_counter()
    assert st == 0
    packed["c"] = pfm_c["num_kern_prep"]

    assert len(rows_a[0]) == len(rows_b[0]) and np.array_equal(rows_a[0], rows_b[0])
    assert np.array_equal(rows_a[1], rows_b[1]) and np.array_equal(rows_a[2], rows_b[2])
    assert np.allclose(rows_a[3], rows_b[3], rtol=1e-12, atol=0)
    if rep < 0:
        continue
    t["a_wall"].append(wall_a)
    t["a_dev"].append((pfm["time_kern_exec_ns"] - pfm["time_kern_proj_ns"]) * 1e-6)
    t["b_wall"].append((t3 - t2) * 1e3)
    t["b_fold_dev"].append((pfm_b["time_kern_exec_ns"] - pfm_b["time_kern_proj_ns"]) * 1e-6)
    t["c_wall"].append((t5 - t4) * 1e3)
    t["c_dev"].append((pfm_c["time_kern_exec_ns"] - pfm_c["time_kern_proj_ns"]) * 1e-6)

# the one-off flattening: a new child table of the same rows, everything else warm
flatten = []
for rep in range(REPS):
    child = GpuHashJoin(J2).begin(build_multihash([(in2, [1])]))
    first, _ = run_snowflake(child)
    warm, _ = run_snowflake(child)
    rows_n = rows_of(snow.fetch())
    assert all(np.array_equal(x, y) for x, y in zip(rows_n[:3], rows_a[:3]))
    flatten.append(first - warm)
    child.end()

say("\n%d joined rows (%.1f %% of the fact rows); packed accumulators: snowflake %d, floor %d"
    % (nitems, 100.0 * nitems / n, packed["a"], packed["c"]))
say("  (a) snowflake lookup      fold kernel %s ms   wall %s ms" % (fmt(t["a_dev"]), fmt(t["a_wall"])))
say("  (b) join + column + fold  fold kernel %s ms   wall %s ms" % (fmt(t["b_fold_dev"]), fmt(t["b_wall"])))
say("  (c) floor: lookup on d1   fold kernel %s ms   wall %s ms" % (fmt(t["c_dev"]), fmt(t["c_wall"])))
a_w, b_w, c_w = np.median(t["a_wall"]), np.median(t["b_wall"]), np.median(t["c_wall"])
a_d, c_d = np.median(t["a_dev"]), np.median(t["c_dev"])
say("  (b) / (a) wall = %.2f (medians; spread of the repetitions: (a) %.3f ms, (b) %.3f ms, (c) %.3f ms)"
    % (b_w / a_w, max(t["a_wall"]) - min(t["a_wall"]), max(t["b_wall"]) - min(t["b_wall"]),
       max(t["c_wall"]) - min(t["c_wall"])))
say("  (a) - (c): fold kernel %+.3f ms (x %.2f; spread (a) %.3f ms, (c) %.3f ms), wall %+.3f ms"
    % (a_d - c_d, a_d / c_d, max(t["a_dev"]) - min(t["a_dev"]), max(t["c_dev"]) - min(t["c_dev"]), a_w - c_w))
say("  one-off flattening per new d2 table (d2's records, compose into d1's %d slots, min/max, narrow): %s ms wall"
    % (span1, fmt(flatten)))
say("  partial rows of (a) == partial rows of (b): keys, counts and integer sums identical, float8 sums within 1e-12")
for obj in (snow, plain, floor, j1, j2, both):
    obj.end()
ds.release()
with open(outfile, "w") as f:
    f.write("\n".join(lines) + "\n")
