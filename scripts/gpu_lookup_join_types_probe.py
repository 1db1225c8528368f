"""LEFT / SEMI / ANTI relations fused into the aggregate's pass (strom_submit_gpupreagg_lookup_typed)
at 1e8 fact rows, a 1e6-key dimension, 80 % of the rows with a partner.

  (a) the inner lookup through the OLD call (strom_submit_gpupreagg_lookup), from a built checkout
      of the parent commit (--parent-tree) and from this tree, in fresh child processes, parent
      and new alternating, before this process touches the GPU.  The parent against itself gives
      the spread; this tree's median must lie inside the parent's range widened by that spread.
  (b) typed left / semi / anti, one table, and the star (inner, left, anti), each next to the
      plan it replaces, in this process, alternating, after a warm-up round:
        left, star:  the join with the (jointype ...) program + the COLUMN projection + a plain fold
        semi, anti:  the one-pass join -> row map -> the mapped fold
      Typed: the fold kernel's device events (perfmon) and wall clock; the alternative: wall clock
      around all its steps.  Every variant's folded-row count is asserted against torch, and the
      typed partial rows against the alternative's.

  python scripts/gpu_lookup_join_types_probe.py [--rows N] [--dim N] [--out FILE] [--parent-tree DIR]
  python scripts/gpu_lookup_join_types_probe.py --child TREE     (what a child of (a) runs)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--dim", type=float, default=1e6)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_join_types_probe.txt"))
ap.add_argument("--parent-tree")
ap.add_argument("--child")
args = ap.parse_args()
n, nd = int(args.rows), int(args.dim)
NGROUPS = 10000
REPS = 5
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


tree = args.child or ROOT
sys.path.insert(0, tree)


def inner_lookup_us(reps=12):
    """median and min of the inner lookup's fold kernel, old call, from the package on sys.path"""
    import bench
    from pg_strom_amd import kds, runtime
    from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
    from pg_strom_amd.gpupreagg import GpuPreAgg
    runtime.init()
    fact, (fk, a, b) = bench.c3_chunk_device(n, 0x5eed0003, nd)
    want = int(((fk < nd) & (a < int(bench.CHAIN_EXT[0])) & (b > float(bench.CHAIN_EXT[1]))).sum().item())
    dkey, dgrp = bench.c3_dimension(nd, NGROUPS)
    km = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)]), [1])])
    join = GpuHashJoin(bench.C3_JOIN).begin(km)
    agg = GpuPreAgg(bench.CHAIN_AGG).begin([(0, NGROUPS)], ext_params=bench.CHAIN_EXT)
    ts = []
    for _ in range(reps):
        agg.reset()
        st, pfm = agg.collect(agg.submit_lookup(join, fact, [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8")]))
        assert st == 0 and int(agg.fetch().column(1)[0].sum()) == want
        ts.append((pfm["time_kern_exec_ns"] - pfm["time_kern_proj_ns"]) * 1e-3)
    agg.end()
    join.end()
    return float(np.median(ts[3:])), float(np.min(ts[3:]))


if args.child:
    med, low = inner_lookup_us()
    print("CHILD %s median_us %.2f min_us %.2f" % (args.child, med, low), flush=True)
    sys.exit(0)

say("lookup join types probe: %d fact rows, %d dimension keys, 80 %% of the rows with a partner, %d groups"
    % (n, nd, NGROUPS))
if args.parent_tree:
    got = {"parent": [], "new": []}
    for label, t in [("parent", args.parent_tree), ("new", ROOT)] * 3:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", t, "--rows", str(n), "--dim", str(nd)],
                             capture_output=True, text=True, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.startswith("CHILD ")]
        if out.returncode != 0 or not line:
            say("child %s failed (rc %d): %s" % (label, out.returncode, out.stderr[-400:]))
            sys.exit(1)                     # nothing more is started on the GPU after a failure
        got[label].append(float(line[0].split()[3]))
    say("(a) inner lookup, old call, fold kernel: median us per process (3 fresh processes each, alternating):")
    say("  parent commit %s" % " ".join("%.1f" % v for v in got["parent"]))
    say("  this tree     %s" % " ".join("%.1f" % v for v in got["new"]))
    spread = max(got["parent"]) - min(got["parent"])
    say("  spread of the parent against itself %.1f us; this tree's median of medians %.1f against the parent's %.1f"
        % (spread, float(np.median(got["new"])), float(np.median(got["parent"]))))
    inside = min(got["parent"]) - spread <= float(np.median(got["new"])) <= max(got["parent"]) + spread
    say("  this tree's time lies %s the parent's range widened by its spread" % ("INSIDE" if inside else "OUTSIDE"))
    if not inside:
        # the inner code is meant to be identical: nothing is written to --out, and nothing more is run
        say("FAILED: the inner lookup moved")
        sys.exit(1)

import torch  # noqa: E402
import bench  # noqa: E402
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd._lib import lib  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash, STROM_RESULTS_ON_DEVICE  # noqa: E402
from pg_strom_amd.gpupreagg import GpuPreAgg  # noqa: E402

runtime.init()
g = torch.Generator(device="cuda")
g.manual_seed(0x5eed0071)
span = int(nd * 1.25)
ks = [torch.randint(0, span, (n,), dtype=torch.int32, device="cuda", generator=g) for _ in range(3)]
a = torch.randint(0, 2**31, (n,), dtype=torch.int32, device="cuda", generator=g)
b = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
grp = torch.randint(0, NGROUPS, (n,), dtype=torch.int32, device="cuda", generator=g)
mm = lambda t: (t.min().item(), t.max().item())                # noqa: E731
fact = runtime.DeviceStore.from_torch_columns(["int4"] * 4 + ["float8", "int4"], ks + [a, b, grp],
                                              [mm(x) for x in ks + [a, b, grp]])
EXT = bench.CHAIN_EXT
passes = (a < int(EXT[0])) & (b > float(EXT[1]))
has = [k < nd for k in ks]                      # (the dimension's keys are a permutation of 0 .. nd - 1)
want = {"left": int(passes.sum().item()), "semi": int((passes & has[0]).sum().item()),
        "anti": int((passes & ~has[0]).sum().item()), "star": int((passes & has[0] & ~has[2]).sum().item())}
del ks, a, b, grp, passes, has
torch.cuda.empty_cache()

dkey, dgrp = bench.c3_dimension(nd, NGROUPS)
dim = kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)])
tables = [GpuHashJoin("(gpuhashjoin (rel (hashkey (var %d int4) 1 int4)))" % (r + 1)).begin(build_multihash([(dim, [1])]))
          for r in range(3)]
QUAL = bench.CHAIN_QUAL                          # over (var 2 int4) and (var 3 float8)
AGGS = "(nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"
DIMKEY = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) " + AGGS + ")"
STAR = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) " + AGGS + " (pmax (var 4 int4)))"
# the mapped fold reads the fact chunk's own columns: a, b, g are columns 4, 5, 6
MAPPED = ("(gpupreagg (qual (and (int4lt (var 4 int4) (param 0 int4)) (float8gt (var 5 float8) (param 1 float8))))"
          " (key (var 6 int4)) (nrows) (psum (int8 (var 4 int4))) (psum (var 5 float8)))")
FACT_COLS = [(0, 6, "int4"), (0, 4, "int4"), (0, 5, "float8")]
DIM_COLS = [(1, 2, "int4"), (0, 4, "int4"), (0, 5, "float8")]
STAR_COLS = DIM_COLS + [(2, 2, "int4")]


def rel(attno, jt):
    return "(rel (hashkey (var %d int4) 1 int4)%s)" % (attno, "" if jt == "inner" else " (jointype %s)" % jt)


alt_join = {
    "left": GpuHashJoin("(gpuhashjoin " + rel(1, "left") + ")", row_population_ratio=1.0).begin(build_multihash([(dim, [1])])),
    "semi": GpuHashJoin("(gpuhashjoin " + rel(1, "semi") + ")", row_population_ratio=0.8).begin(build_multihash([(dim, [1])])),
    "anti": GpuHashJoin("(gpuhashjoin " + rel(1, "anti") + ")", row_population_ratio=0.2).begin(build_multihash([(dim, [1])])),
    "star": GpuHashJoin("(gpuhashjoin " + rel(1, "inner") + " " + rel(2, "left") + " " + rel(3, "anti") + ")",
                        row_population_ratio=0.2).begin(build_multihash([(dim, [1])] * 3)),
}
# name -> (tables, join types, typed spec, columns, the alternative's fold spec)
VARIANTS = {
    "left": (tables[:1], ["left"], DIMKEY, DIM_COLS, DIMKEY),
    "semi": (tables[:1], ["semi"], DIMKEY, FACT_COLS, MAPPED),
    "anti": (tables[:1], ["anti"], DIMKEY, FACT_COLS, MAPPED),
    "star": (tables, ["inner", "left", "anti"], STAR, STAR_COLS, STAR),
}
typed = {v: GpuPreAgg(VARIANTS[v][2]).begin([(0, NGROUPS)], ext_params=EXT) for v in VARIANTS}
alt = {v: GpuPreAgg(VARIANTS[v][4]).begin([(0, NGROUPS)], ext_params=EXT) for v in VARIANTS}


def rows_of(pr):
    keys = np.where(pr.column(0)[1], 10**9, pr.column(0)[0].astype(np.int64))
    order = np.argsort(keys)
    return ([keys[order]] + [pr.column(c)[0][order] for c in range(1, len(pr.targets))],
            [pr.column(c)[1][order] for c in range(1, len(pr.targets))])


t = {v: {"dev": [], "wall": [], "alt": []} for v in VARIANTS}
packed = {}
for rep in range(-1, REPS):                     # (rep -1 warms programs, tables and slot records)
    for v, (tbls, jts, spec, cols, _) in VARIANTS.items():
        typed[v].reset()
        lib.strom_synchronize()
        t0 = time.perf_counter()
        st, pfm = typed[v].collect(typed[v].submit_lookup_typed(tbls, jts, fact, cols))
        t1 = time.perf_counter()
        assert st == 0
        packed[v] = pfm["num_kern_prep"]
        rows_t, nulls_t = rows_of(typed[v].fetch())
        assert int(rows_t[1].sum()) == want[v], (v, int(rows_t[1].sum()), want[v])

        alt[v].reset()
        lib.strom_synchronize()
        t2 = time.perf_counter()
        if v in ("semi", "anti"):
            pending = alt_join[v].submit(fact, flags=STROM_RESULTS_ON_DEVICE)
            rmap = alt_join[v].row_map(pending)
            res = alt_join[v].collect(pending)
            assert res.errcode == 0
            st = alt[v].collect(alt[v].submit(fact, row_map=rmap))[0]
            t3 = time.perf_counter()
            rmap.release()
        else:
            joined, nitems = alt_join[v].join_to_column(fact, cols)
            st = alt[v].fold(joined)[0]
            t3 = time.perf_counter()
            joined.release()
        assert st == 0
        rows_a, nulls_a = rows_of(alt[v].fetch())
        assert int(rows_a[1].sum()) == want[v], (v, "alternative", int(rows_a[1].sum()), want[v])
        assert len(rows_t) == len(rows_a) and all(np.array_equal(x, y) for x, y in zip(rows_t[:3], rows_a[:3]))
        assert np.allclose(rows_t[3], rows_a[3], rtol=1e-12, atol=0)
        # every further aggregate (the star's pmax of the left relation's column): NULL flags and values
        assert all(np.array_equal(x, y) for x, y in zip(nulls_t, nulls_a)), v
        for c in range(4, len(rows_t)):
            assert np.array_equal(rows_t[c][~nulls_t[c - 1]], rows_a[c][~nulls_a[c - 1]]), (v, c)
        if rep < 0:
            continue
        t[v]["dev"].append((pfm["time_kern_exec_ns"] - pfm["time_kern_proj_ns"]) * 1e-6)
        t[v]["wall"].append((t1 - t0) * 1e3)
        t[v]["alt"].append((t3 - t2) * 1e3)

say("\n(b) typed lookup next to the plan it replaces, ms: median [min .. max] of %d rounds after a warm-up round,"
    " variants alternating;" % REPS)
say("typed: the fold kernel's device events and wall clock; alternative: wall clock around all of its steps")
ALT_NAME = {"left": "left join + column projection + fold", "semi": "one-pass semi join -> row map -> mapped fold",
            "anti": "one-pass anti join -> row map -> mapped fold",
            "star": "3-relation join (inner, left, anti) + column projection + fold"}
fmt = lambda x: "%8.3f [%8.3f .. %8.3f]" % (float(np.median(x)), min(x), max(x))     # noqa: E731
for v in VARIANTS:
    say("  %-4s %-20s %10d rows folded, packed accumulators %d" % (v, "/".join(VARIANTS[v][1]), want[v], packed[v]))
    say("       typed, fold kernel   %s" % fmt(t[v]["dev"]))
    say("       typed, wall          %s" % fmt(t[v]["wall"]))
    say("       alternative, wall    %s   (%s)" % (fmt(t[v]["alt"]), ALT_NAME[v]))
    say("       alternative / typed, wall medians: %.2f" % (float(np.median(t[v]["alt"])) / float(np.median(t[v]["wall"]))))
say("partial rows of every typed variant == its alternative's: keys, NULL flags, counts, integer sums and the star's pmax"
    " identical, float8 sums within 1e-12")
for obj in list(typed.values()) + list(alt.values()) + list(alt_join.values()) + tables:
    obj.end()
fact.release()
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
