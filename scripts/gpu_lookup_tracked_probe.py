"""RIGHT / FULL joins fused into the aggregate's pass (strom_submit_gpupreagg_lookup_tracked and
_lookup_unmatched) at 1e8 resident fact rows and a 1e6-key dimension: 80 % of the rows with a partner, 20 %
of the slots unmatched, 10000 groups, WHERE keeps 50 % (the protocol of DESIGN 3.7.1).

  (a) the UNTRACKED inner and LEFT lookups through the old calls (strom_submit_gpupreagg_lookup, _lookup_typed),
      from a built checkout of the parent commit (--parent-tree) and from this tree, in fresh child
      processes, parent and new in turns, before this process touches the GPU.  The parent against itself
      gives the spread; this tree's median must lie inside the parent's range widened by that spread.
  (b) the tracked RIGHT and FULL fold kernels next to the inner / LEFT typed kernels of the same mapping,
      device events: the price of the flag request.  Once more WITHOUT a WHERE: a tracked program has no
      qual-first, so under the WHERE it probes twice the rows the untracked one does; without one both probe the
      same rows, and what is left is the flag traffic and the missing next-tile prefetch.
  (c) the unmatched pass alone, device events and wall clock.
  (d) wall clock of chunk fold + unmatched pass against the plan it replaces: the join with (track_matches),
      the COLUMN projection, a plain fold, gpuhashjoin_unmatched, strom_hashjoin_project_column(task, tbl,
      NULL, ..) and a second plain fold.
  In this process the variants alternate, after a warm-up round; every variant's counts are asserted against
  torch, the flag image against torch, and the fused partial rows against the replaced plan's.

  python scripts/gpu_lookup_tracked_probe.py [--rows N] [--dim N] [--out FILE] [--parent-tree DIR]
  python scripts/gpu_lookup_tracked_probe.py --child TREE     (what a child of (a) runs)
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_tracked_probe.txt"))
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


def untracked_us(reps=12):
    """medians of the inner (old call) and the LEFT (typed call) fold kernel, from the package on sys.path"""
    import bench
    from pg_strom_amd import kds, runtime
    from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
    from pg_strom_amd.gpupreagg import GpuPreAgg
    runtime.init()
    fact, (fk, a, b) = bench.c3_chunk_device(n, 0x5eed0003, nd)
    passes = (a < int(bench.CHAIN_EXT[0])) & (b > float(bench.CHAIN_EXT[1]))
    want = {"inner": int(((fk < nd) & passes).sum().item()), "left": int(passes.sum().item())}
    dkey, dgrp = bench.c3_dimension(nd, NGROUPS)
    km = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)]), [1])])
    join = GpuHashJoin(bench.C3_JOIN).begin(km)
    cols = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8")]
    out = {}
    for v in ("inner", "left"):
        agg = GpuPreAgg(bench.CHAIN_AGG).begin([(0, NGROUPS)], ext_params=bench.CHAIN_EXT)
        ts = []
        for _ in range(reps):
            agg.reset()
            pending = agg.submit_lookup(join, fact, cols) if v == "inner" else agg.submit_lookup_typed([join], ["left"], fact, cols)
            st, pfm = agg.collect(pending)
            assert st == 0 and int(agg.fetch().column(1)[0].sum()) == want[v]
            ts.append((pfm["time_kern_exec_ns"] - pfm["time_kern_proj_ns"]) * 1e-3)
        agg.end()
        out[v] = float(np.median(ts[3:]))
    join.end()
    return out


if args.child:
    got = untracked_us()
    print("CHILD %s inner_us %.2f left_us %.2f" % (args.child, got["inner"], got["left"]), flush=True)
    sys.exit(0)

say("lookup tracked probe: %d fact rows, %d dimension keys, 80 %% of the rows with a partner, 20 %% of the slots"
    " unmatched, %d groups" % (n, nd, NGROUPS))
if args.parent_tree:
    got = {("parent", "inner"): [], ("parent", "left"): [], ("new", "inner"): [], ("new", "left"): []}
    for label, t in [("parent", args.parent_tree), ("new", ROOT)] * 3:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", t, "--rows", str(n), "--dim", str(nd)],
                             capture_output=True, text=True, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.startswith("CHILD ")]
        if out.returncode != 0 or not line:
            say("child %s failed (rc %d): %s" % (label, out.returncode, out.stderr[-400:]))
            sys.exit(1)                     # nothing more is started on the GPU after a failure
        got[(label, "inner")].append(float(line[0].split()[3]))
        got[(label, "left")].append(float(line[0].split()[5]))
    say("(a) untracked lookups through the old calls, fold kernel: median us per process (3 fresh processes each, in turns):")
    moved = False
    for v in ("inner", "left"):
        par, new = got[("parent", v)], got[("new", v)]
        spread = max(par) - min(par)
        inside = min(par) - spread <= float(np.median(new)) <= max(par) + spread
        say("  %-5s parent commit %s | this tree %s" % (v, " ".join("%.1f" % x for x in par), " ".join("%.1f" % x for x in new)))
        say("        spread of the parent against itself %.1f us; this tree's median %.1f against the parent's %.1f: %s"
            % (spread, float(np.median(new)), float(np.median(par)), "INSIDE" if inside else "OUTSIDE"))
        moved = moved or not inside
    if moved:
        say("FAILED: an untracked lookup moved")     # (the code is meant to be identical: no profile is written)
        sys.exit(1)

import torch  # noqa: E402
import bench  # noqa: E402
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd._lib import lib  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash  # noqa: E402
from pg_strom_amd.gpupreagg import GpuPreAgg  # noqa: E402

runtime.init()
g = torch.Generator(device="cuda")
g.manual_seed(0x5eed0081)
# keys: 80 % of the rows inside the 80 % of the key range they all share, the rest above every key -- so 80 % of
# the rows have a partner and the upper 20 % of the slots have none (the dimension's keys are 0 .. nd - 1)
k = torch.randint(0, nd, (n,), dtype=torch.int32, device="cuda", generator=g)
cut = int(0.8 * nd)
k = torch.where(k >= cut, k + (nd - cut), k)
a = torch.randint(0, 2**31, (n,), dtype=torch.int32, device="cuda", generator=g)
b = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
mm = lambda t: (t.min().item(), t.max().item())                # noqa: E731
fact = runtime.DeviceStore.from_torch_columns(["int4", "int4", "float8"], [k, a, b], [mm(x) for x in (k, a, b)])
EXT = bench.CHAIN_EXT
passes = (a < int(EXT[0])) & (b > float(EXT[1]))
has = k < nd
want = {"inner": int((passes & has).sum().item()), "left": int(passes.sum().item())}
want_nowhere = {"inner": int(has.sum().item()), "left": n}
want_image = np.zeros(nd, dtype=np.uint8)
want_image[torch.unique(k[has]).cpu().numpy()] = 1
say("rows with a partner %.1f %%, WHERE keeps %.1f %%, slots matched %.1f %%"
    % (100.0 * has.sum().item() / n, 100.0 * passes.sum().item() / n, 100.0 * want_image.sum() / nd))
del k, a, b, passes, has
torch.cuda.empty_cache()

dkey, dgrp = bench.c3_dimension(nd, NGROUPS)
assert np.array_equal(np.sort(dkey), np.arange(nd))
dim = kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)])
table = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(build_multihash([(dim, [1])]))
old_join = {jt: GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4) (jointype %s) (track_matches)))" % jt,
                            row_population_ratio=1.0).begin(build_multihash([(dim, [1])])) for jt in ("inner", "left")}
SPEC = "(gpupreagg (qual " + bench.CHAIN_QUAL + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))"
COLS = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8")]
NOWHERE = "(gpupreagg (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))"
sess = {(jt, kind): GpuPreAgg(SPEC).begin([(0, NGROUPS)], ext_params=EXT)
        for jt in ("inner", "left") for kind in ("typed", "tracked", "old")}
sess.update({(jt, kind): GpuPreAgg(NOWHERE).begin([(0, NGROUPS)])
             for jt in ("inner", "left") for kind in ("typed_nowhere", "tracked_nowhere")})


def rows_of(pr):
    keys = np.where(pr.column(0)[1], 10**9, pr.column(0)[0].astype(np.int64))
    order = np.argsort(keys)
    return [keys[order]] + [pr.column(c)[0][order] for c in range(1, len(pr.targets))]


dev_us = lambda pfm: (pfm["time_kern_exec_ns"] - pfm["time_kern_proj_ns"]) * 1e-3      # noqa: E731
t = {jt: {"typed": [], "tracked": [], "unm_dev": [], "unm_wall": [], "fused_wall": [], "old_wall": [],
          "typed_nowhere": [], "tracked_nowhere": []} for jt in ("inner", "left")}
for rep in range(-1, REPS):                     # (rep -1 warms programs, tables, slot records and flags)
    for jt in ("inner", "left"):
        s = sess[(jt, "typed")]
        s.reset()
        st, pfm = s.collect(s.submit_lookup_typed([table], [jt], fact, COLS))
        assert st == 0 and int(s.fetch().column(1)[0].sum()) == want[jt]
        typed_us = dev_us(pfm)

        s = sess[(jt, "tracked")]
        s.reset()
        if rep >= 0:
            s.reset_lookup_matches()
        lib.strom_synchronize()
        t0 = time.perf_counter()
        st, pfm = s.collect(s.submit_lookup_tracked([table], [jt], 1, fact, COLS))
        t1 = time.perf_counter()
        st2, pfm2 = s.collect(s.submit_lookup_unmatched([table], [jt], 1, COLS))
        t2 = time.perf_counter()
        assert st == 0 and st2 == 0
        rows_f = rows_of(s.fetch())
        assert int(rows_f[1].sum()) == want[jt]        # (the strict WHERE drops every unmatched row: its fact columns are NULL)
        assert np.array_equal(s.lookup_matches(), want_image)

        o, j = sess[(jt, "old")], old_join[jt]
        o.reset()
        j.reset_matches()
        lib.strom_synchronize()
        t3 = time.perf_counter()
        joined, _ = j.join_to_column(fact, COLS)
        assert o.fold(joined)[0] == 0
        rest, nrest = j.unmatched_to_column(COLS)
        assert o.fold(rest)[0] == 0
        t4 = time.perf_counter()
        joined.release()
        rest.release()
        assert nrest == nd - int(want_image.sum())
        rows_o = rows_of(o.fetch())
        assert all(np.array_equal(x, y) for x, y in zip(rows_f[:3], rows_o[:3]))
        assert np.allclose(rows_f[3], rows_o[3], rtol=1e-12, atol=0)
        # without a WHERE: the fold kernels alone (the flags of this session stay set: every store is skipped
        # after the warm-up round, which is the warm case of a many-chunk scan)
        nowhere_us = {}
        for kind in ("typed_nowhere", "tracked_nowhere"):
            s = sess[(jt, kind)]
            s.reset()
            if kind == "typed_nowhere":
                st, pfm3 = s.collect(s.submit_lookup_typed([table], [jt], fact, COLS))
            else:
                st, pfm3 = s.collect(s.submit_lookup_tracked([table], [jt], 1, fact, COLS))
            assert st == 0 and int(s.fetch().column(1)[0].sum()) == want_nowhere[jt]
            nowhere_us[kind] = dev_us(pfm3)
        if rep < 0:
            continue
        t[jt]["typed_nowhere"].append(nowhere_us["typed_nowhere"])
        t[jt]["tracked_nowhere"].append(nowhere_us["tracked_nowhere"])
        t[jt]["typed"].append(typed_us)
        t[jt]["tracked"].append(dev_us(pfm))
        t[jt]["unm_dev"].append(dev_us(pfm2))
        t[jt]["unm_wall"].append((t2 - t1) * 1e6)
        t[jt]["fused_wall"].append((t2 - t0) * 1e6)
        t[jt]["old_wall"].append((t4 - t3) * 1e6)

fmt = lambda x: "%9.1f [%9.1f .. %9.1f]" % (float(np.median(x)), min(x), max(x))     # noqa: E731
say("\nus: median [min .. max] of %d rounds after a warm-up round, variants alternating in one process" % REPS)
for jt, name in (("inner", "RIGHT (inner + tracked)"), ("left", "FULL (left + tracked)")):
    say("%s, %d rows folded" % (name, want[jt]))
    say("  (b) untracked typed fold kernel          %s" % fmt(t[jt]["typed"]))
    say("      tracked fold kernel                  %s   tracked / untracked %.2f"
        % (fmt(t[jt]["tracked"]), float(np.median(t[jt]["tracked"])) / float(np.median(t[jt]["typed"]))))
    say("      without a WHERE: untracked           %s" % fmt(t[jt]["typed_nowhere"]))
    say("      without a WHERE: tracked, flags warm %s   tracked / untracked %.2f"
        % (fmt(t[jt]["tracked_nowhere"]),
           float(np.median(t[jt]["tracked_nowhere"])) / float(np.median(t[jt]["typed_nowhere"]))))
    say("  (c) unmatched pass, kernel               %s" % fmt(t[jt]["unm_dev"]))
    say("      unmatched pass, wall                 %s" % fmt(t[jt]["unm_wall"]))
    say("  (d) chunk fold + unmatched pass, wall    %s" % fmt(t[jt]["fused_wall"]))
    say("      tracked join + projection + fold + unmatched + projection + fold, wall")
    say("                                           %s   replaced plan / fused %.2f"
        % (fmt(t[jt]["old_wall"]), float(np.median(t[jt]["old_wall"])) / float(np.median(t[jt]["fused_wall"]))))
say("every variant's folded-row count == torch's, the flag image == torch's set of matched keys, the fused partial"
    " rows == the replaced plan's (keys, counts, integer sums identical, float8 sums within 1e-12)")
for obj in list(sess.values()) + list(old_join.values()) + [table]:
    obj.end()
fact.release()
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
