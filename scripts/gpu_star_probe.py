"""fact JOIN dim1 JOIN dim2 WHERE ... GROUP BY dim1.g over a resident fact chunk, three ways:
  (a) the star lookup: ONE kernel (strom_submit_gpupreagg_lookup_star)
  (b) the plan that exists without it: the two-relation general join, the COLUMN projection
      (strom_hashjoin_project_column), then the plain fold of the joined chunk
  (floor) the one-dimension lookup (strom_submit_gpupreagg_lookup) on the same chunk
fact(k1 int4, k2 int4, a int4, b float8), two dimensions with narrow slot records, a WHERE that
keeps ~50 %, a match rate of ~80 % per dimension; 1000 and 10000 groups.  One process, the three
alternating, warm programs, three repetitions each.  (a) and the floor: the fold kernel's device
events (perfmon) and wall clock; (b): wall clock around join + projection + fold, and the device
events of its fold -- the join and the projection do not report theirs through this interface.
Asserts that (a)'s partial rows equal (b)'s.  Writes profiles/star_lookup_probe.txt.
usage: gpu_star_probe.py [nrows] [ndim] [outfile]"""
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
nd = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
outfile = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "star_lookup_probe.txt")
REPS = 3
QUAL = "(and (int4lt (var 2 int4) (param 0 int4)) (float8gt (var 3 float8) (param 1 float8)))"
EXT = [np.int32(2**30 - 1), 0.0]                # a < 2^30 of [0, 2^31): 50 %
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def rows_of(pr, nkeys=1):
    keys = np.where(pr.column(0)[1], 10**9, pr.column(0)[0].astype(np.int64))
    order = np.argsort(keys)
    return [keys[order]] + [pr.column(c)[0][order] for c in range(nkeys, len(pr.targets))]


runtime.init()
rng = np.random.default_rng(11)
span = int(nd * 1.25)                           # 80 % of the fact keys have a partner
k1 = rng.integers(0, span, n, dtype=np.int64).astype(np.int32)
k2 = rng.integers(0, span, n, dtype=np.int64).astype(np.int32)
a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
b = rng.random(n)
fact = kds.build_kds("column", [kds.Column("int4", k1), kds.Column("int4", k2), kds.Column("int4", a),
                                kds.Column("float8", b)])
del k1, k2, a, b
ds = runtime.DeviceStore.upload(fact)
del fact
say("star lookup probe: %d fact rows, 2 dimensions of %d rows (key span %d), WHERE keeps 50 %%, %d repetitions"
    % (n, nd, span, REPS))
for ngroups in (1000, 10000):
    dk1 = rng.permutation(span)[:nd].astype(np.int32)
    dk2 = rng.permutation(span)[:nd].astype(np.int32)
    in1 = kds.build_kds("row_flat", [kds.Column("int4", dk1), kds.Column("int4", (dk1 % ngroups).astype(np.int32))])
    in2 = kds.build_kds("row_flat", [kds.Column("int4", dk2), kds.Column("int4", (dk2 % 100).astype(np.int32))])
    j1 = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(build_multihash([(in1, [1])]))
    j2 = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 2 int4) 1 int4)))").begin(build_multihash([(in2, [1])]))
    both = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)) (rel (hashkey (var 2 int4) 1 int4)))")
    both.begin(build_multihash([(in1, [1]), (in2, [1])]))
    # GROUP BY dim1.g; the WHERE also reads dim2's column (always true: values are 0 .. 99), so
    # relation 2 serves a column (narrow records) and the aggregates stay packable -- but the qual
    # is then evaluated AFTER the probes: (a) probes for every row with keys inside both tables
    spec = ("(gpupreagg (qual (and " + QUAL + " (int4lt (var 4 int4) (const int4 100)))) (key (var 1 int4)) (nrows)"
            " (psum (int8 (var 2 int4))) (psum (var 3 float8)))")
    star_cols = [(1, 2, "int4"), (0, 3, "int4"), (0, 4, "float8"), (2, 2, "int4")]
    floor_spec = ("(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4)))"
                  " (psum (var 3 float8)))")
    floor_cols = [(1, 2, "int4"), (0, 3, "int4"), (0, 4, "float8")]
    star = GpuPreAgg(spec).begin([(0, ngroups)], ext_params=EXT)
    plain = GpuPreAgg(spec).begin([(0, ngroups)], ext_params=EXT)
    floor = GpuPreAgg(floor_spec).begin([(0, ngroups)], ext_params=EXT)
    t = {"a_wall": [], "a_dev": [], "b_wall": [], "b_fold_dev": [], "f_wall": [], "f_dev": []}
    packed = {}
    for rep in range(-1, REPS):                 # (rep -1 warms programs, tables and slot records)
        star.reset()
        lib.strom_synchronize()
        t0 = time.perf_counter()
        st, pfm = star.collect(star.submit_lookup_star([j1, j2], ds, star_cols))
        t1 = time.perf_counter()
        assert st == 0
        packed["a"] = pfm["num_kern_prep"]
        rows_a = rows_of(star.fetch())

        plain.reset()
        lib.strom_synchronize()
        t2 = time.perf_counter()
        joined, nitems = both.join_to_column(ds, star_cols)
        st, pfm_b = plain.fold(joined)
        t3 = time.perf_counter()
        assert st == 0
        joined.release()
        rows_b = rows_of(plain.fetch())

        floor.reset()
        lib.strom_synchronize()
        t4 = time.perf_counter()
        st, pfm_f = floor.collect(floor.submit_lookup(j1, ds, floor_cols))
        t5 = time.perf_counter()
        assert st == 0
        packed["floor"] = pfm_f["num_kern_prep"]

        assert len(rows_a) == len(rows_b) and np.array_equal(rows_a[0], rows_b[0])
        assert np.array_equal(rows_a[1], rows_b[1]) and np.array_equal(rows_a[2], rows_b[2])
        assert np.allclose(rows_a[3], rows_b[3], rtol=1e-12, atol=0)
        if rep < 0:
            continue
        t["a_wall"].append((t1 - t0) * 1e3)
        t["a_dev"].append((pfm["time_kern_exec_ns"] - pfm["time_kern_proj_ns"]) * 1e-6)
        t["b_wall"].append((t3 - t2) * 1e3)
        t["b_fold_dev"].append((pfm_b["time_kern_exec_ns"] - pfm_b["time_kern_proj_ns"]) * 1e-6)
        t["f_wall"].append((t5 - t4) * 1e3)
        t["f_dev"].append((pfm_f["time_kern_exec_ns"] - pfm_f["time_kern_proj_ns"]) * 1e-6)
    fmt = lambda v: "[" + " ".join("%.3f" % x for x in v) + "]"     # noqa: E731
    say("\n%d groups, %d joined rows (%.1f %% of the fact rows); packed accumulators: star %d, floor %d"
        % (ngroups, nitems, 100.0 * nitems / n, packed["a"], packed["floor"]))
    say("  (a) star lookup           fold kernel %s ms   wall %s ms" % (fmt(t["a_dev"]), fmt(t["a_wall"])))
    say("  (b) join + column + fold  fold kernel %s ms   wall %s ms" % (fmt(t["b_fold_dev"]), fmt(t["b_wall"])))
    say("  floor: one-table lookup   fold kernel %s ms   wall %s ms" % (fmt(t["f_dev"]), fmt(t["f_wall"])))
    a_w, b_w, f_w = np.median(t["a_wall"]), np.median(t["b_wall"]), np.median(t["f_wall"])
    a_d, f_d = np.median(t["a_dev"]), np.median(t["f_dev"])
    spread = max(max(v) - min(v) for v in (t["a_wall"], t["b_wall"]))
    say("  (b) / (a) wall = %.2f (medians; largest spread of the repetitions %.3f ms, (b) - (a) = %.3f ms)"
        % (b_w / a_w, spread, b_w - a_w))
    say("  the added relation over the floor: fold kernel %+.3f ms (x %.2f), wall %+.3f ms; %.2f ns per 1e2 rows"
        % (a_d - f_d, a_d / f_d, a_w - f_w, (a_d - f_d) * 1e6 / n * 100))
    say("  partial rows of (a) == partial rows of (b): keys, counts and integer sums identical, float8 sums within 1e-12")
    for obj in (star, plain, floor, j1, j2, both):
        obj.end()
ds.release()
with open(outfile, "w") as f:
    f.write("\n".join(lines) + "\n")
