"""GpuHashJoin's join types at the C3 shape (1e8 outer rows, 1e6 inner keys, 80 % of the rows with a
partner): what the one-pass kernels cost for SEMI / ANTI / LEFT next to the inner join they share a
body with, what the general kernel costs for the same joins (STROM_HASHJOIN_NO_FAST=1), and SEMI over
an inner side with every key duplicated -- where an inner join has to take the general kernel and
SEMI does not.  Device-event times of the main kernel (perfmon time_kern_exec_ns), after warm-up,
the variants alternating in one process; every variant's record count is asserted.

  python scripts/gpu_join_types_probe.py [--rows N] [--dim N] [--out FILE] [--parent-tree DIR]
      the probe.  --parent-tree: a built checkout of the commit before join types; its inner
      one-pass time and this tree's are then taken by fresh child processes, parent and new
      alternating, before this process touches the GPU (the parent against itself gives the spread)
  python scripts/gpu_join_types_probe.py --child TREE
      what such a child runs: the inner one-pass join from the package at TREE, one line of output
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/gpu_join_types_probe.py --kernels-only
      a short run of the variants for the profiler (a run of its own: tracing slows the host)
  python scripts/gpu_join_types_probe.py --append-kernel-stats DIR --out FILE
      the join kernels' rows of the profiler's kernel statistics, appended to FILE
"""
import argparse
import csv
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--dim", type=float, default=1e6)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_types_probe.txt"))
ap.add_argument("--parent-tree")
ap.add_argument("--child")
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--append-kernel-stats")
args = ap.parse_args()
n, nd = int(args.rows), int(args.dim)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


if args.append_kernel_stats:
    rows = []
    for f in glob.glob(os.path.join(args.append_kernel_stats, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "hashjoin" in row.get("Name", ""):
                rows.append(row)
    with open(args.out, "a") as fh:
        fh.write("\nrocprofv3 --kernel-trace --stats, a run of its own (--kernels-only: 3 launches per variant):\n")
        fh.write("  %-34s %6s %12s %12s %12s\n" % ("kernel", "calls", "avg us", "min us", "max us"))
        for row in sorted(rows, key=lambda r: r["Name"]):
            fh.write("  %-34s %6s %12.1f %12.1f %12.1f\n" % (
                row["Name"][:34], row["Calls"], float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3,
                float(row["MaxNs"]) / 1e3))
        if not rows:
            fh.write("  (no kernel statistics found under %s)\n" % args.append_kernel_stats)
    sys.exit(0)

tree = args.child or ROOT
sys.path.insert(0, tree)


def inner_one_pass_us(reps=12):
    """median and min of the inner one-pass kernel at the C3 shape, from the package on sys.path"""
    import bench
    from pg_strom_amd import kds, runtime
    from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
    runtime.init()
    fact, (fk, _, _) = bench.c3_chunk_device(n, 0x5eed0003, nd)
    nmatch = int((fk < nd).sum().item())
    dkey, dgrp = bench.c3_dimension(nd, 10000)
    km = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)]), [1])])
    join = GpuHashJoin(bench.C3_JOIN, row_population_ratio=0.8).begin(km)
    ts = []
    for _ in range(reps):
        r = join.join_chunk(fact, flags=1)
        assert r.nitems == nmatch
        ts.append(r.perfmon["time_kern_exec_ns"] * 1e-3)
    join.end()
    return float(np.median(ts[3:])), float(np.min(ts[3:]))


if args.child:
    med, low = inner_one_pass_us()
    print("CHILD %s median_us %.2f min_us %.2f" % (args.child, med, low), flush=True)
    sys.exit(0)

say("join types probe: %d outer rows, %d inner keys, 80 %% of the rows with a partner" % (n, nd))
if args.parent_tree and not args.kernels_only:
    # fresh processes, parent and new alternating; the parent against itself is the spread
    got = {"parent": [], "new": []}
    for label, t in [("parent", args.parent_tree), ("new", ROOT)] * 3:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", t, "--rows", str(n), "--dim", str(nd)],
                             capture_output=True, text=True, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.startswith("CHILD ")]
        if out.returncode != 0 or not line:
            say("child %s failed (rc %d): %s" % (label, out.returncode, out.stderr[-400:]))
            sys.exit(1)                     # nothing more is started on the GPU after a failure
        got[label].append(float(line[0].split()[3]))
    say("inner one-pass kernel, median us per process (3 fresh processes each, alternating):")
    say("  parent commit %s" % " ".join("%.1f" % v for v in got["parent"]))
    say("  this tree     %s" % " ".join("%.1f" % v for v in got["new"]))
    spread = max(got["parent"]) - min(got["parent"])
    say("  spread of the parent against itself %.1f us; this tree's median of medians %.1f against the parent's %.1f"
        % (spread, float(np.median(got["new"])), float(np.median(got["parent"]))))
    inside = min(got["parent"]) - spread <= float(np.median(got["new"])) <= max(got["parent"]) + spread
    say("  this tree's time lies %s the parent's range widened by its spread" % ("INSIDE" if inside else "OUTSIDE"))

import torch  # noqa: E402
import bench  # noqa: E402
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash  # noqa: E402

runtime.init()
fact, (fk, _, _) = bench.c3_chunk_device(n, 0x5eed0003, nd)
nmatch = int((fk < nd).sum().item())
del fk
# the same columns with one row in five matching: ANTI then emits what SEMI emits above
g = torch.Generator(device="cuda")
g.manual_seed(0x5eed0033)
fk2 = torch.randint(0, 5 * nd, (n,), dtype=torch.int32, device="cuda", generator=g)
nmatch2 = int((fk2 < nd).sum().item())
fact2 = runtime.DeviceStore.from_torch_columns(["int4"], [fk2], [(int(fk2.min().item()), int(fk2.max().item()))])
del fk2
torch.cuda.empty_cache()
dkey, dgrp = bench.c3_dimension(nd, 10000)
unique = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)]), [1])])
dkey2, dgrp2 = np.concatenate([dkey, dkey]), np.concatenate([dgrp, dgrp])
doubled = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", dkey2), kds.Column("int4", dgrp2)]), [1])])


def spec(jointype):
    return "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)%s))" % ("" if jointype == "inner" else " (jointype %s)" % jointype)


# (name, join type, table, chunk, general kernel?, records expected, room ratio)
VARIANTS = [
    ("inner            one-pass", "inner", unique, fact, False, nmatch, 0.8),
    ("semi             one-pass", "semi", unique, fact, False, nmatch, 0.8),
    ("anti             one-pass", "anti", unique, fact, False, n - nmatch, 0.2),
    ("anti (1/5 match) one-pass", "anti", unique, fact2, False, n - nmatch2, 0.8),
    ("left             one-pass", "left", unique, fact, False, n, 1.0),
    ("inner            general ", "inner", unique, fact, True, nmatch, 0.8),
    ("semi             general ", "semi", unique, fact, True, nmatch, 0.8),
    ("anti             general ", "anti", unique, fact, True, n - nmatch, 0.2),
    ("left             general ", "left", unique, fact, True, n, 1.0),
    ("inner, keys x2   general ", "inner", doubled, fact, False, 2 * nmatch, 1.6),
    ("semi,  keys x2   one-pass", "semi", doubled, fact, False, nmatch, 0.8),
    ("semi,  keys x2   general ", "semi", doubled, fact, True, nmatch, 0.8),
]
joins = {}
for _, jt, km, _, _, _, ratio in VARIANTS:
    key = (jt, id(km), ratio)
    if key not in joins:
        joins[key] = GpuHashJoin(spec(jt), row_population_ratio=ratio).begin(km)
assert joins[("inner", id(unique), 0.8)].table_info(1)["unique"]
assert not joins[("semi", id(doubled), 0.8)].table_info(1)["unique"]
REPS = 3 if args.kernels_only else 9
times = {name: [] for name, *_ in VARIANTS}
for rep in range(REPS):
    for name, jt, km, chunk, general, want, ratio in VARIANTS:
        if general:
            os.environ["STROM_HASHJOIN_NO_FAST"] = "1"
        else:
            os.environ.pop("STROM_HASHJOIN_NO_FAST", None)
        r = joins[(jt, id(km), ratio)].join_chunk(chunk, flags=1)
        assert r.errcode == 0 and r.nitems == want, (name, r.errcode, r.nitems, want)
        times[name].append(r.perfmon["time_kern_exec_ns"] * 1e-3)
os.environ.pop("STROM_HASHJOIN_NO_FAST", None)
for j in joins.values():
    j.end()
if args.kernels_only:
    sys.exit(0)

say("main kernel, device events, us: median [min .. max] of %d launches after 2 warm-up rounds, variants alternating;"
    % (REPS - 2))
say("bytes = 4 B per outer row (the key column) + 8 B per record")
base = None
for name, jt, km, chunk, general, want, ratio in VARIANTS:
    t = np.array(times[name][2:])
    mid = float(np.median(t))
    nbytes = 4.0 * n + 8.0 * want
    if base is None:
        base = mid
    say("  %s %9.1f [%8.1f .. %8.1f]  %10d records  %6.0f MB  %6.0f GB/s  x%.2f of inner one-pass"
        % (name, mid, float(t.min()), float(t.max()), want, nbytes / 1e6, nbytes / mid / 1e3, mid / base))
med = {name: float(np.median(times[name][2:])) for name, *_ in VARIANTS}
say("semi over duplicated keys: one-pass %.1f us, general %.1f us (x%.2f); the inner join of the same table, general: %.1f us"
    % (med["semi,  keys x2   one-pass"], med["semi,  keys x2   general "],
       med["semi,  keys x2   general "] / med["semi,  keys x2   one-pass"], med["inner, keys x2   general "]))
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
