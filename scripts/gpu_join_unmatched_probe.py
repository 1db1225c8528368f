"""RIGHT / FULL joins at the C3 shape (1e8 outer rows, 1e6 inner keys, 80 % of the rows with a partner):
what tracking matched entries costs the probe kernels, and what the unmatched pass costs.  Device-event
times of the main kernel (perfmon time_kern_exec_ns), variants alternating in one process, median of 7.

  python scripts/gpu_join_unmatched_probe.py [--rows N] [--dim N] [--out FILE] [--parent-tree DIR]
      (a) with --parent-tree, a built checkout of the commit before this one: the UNTRACKED inner and
          left one-pass kernels from that tree and from this one, by fresh child processes in turns,
          before this process touches the GPU (the parent against itself gives the spread)
      (b) tracked inner and left, one-pass and general: chunk 1 after a reset (flags cold) and chunk 5
          (flags warm), next to the untracked one-pass and general kernels of the same process
      (c) the same with every outer row on ONE key (the hot flag test-before-set exists for)
      (d) the unmatched pass over the 1e6 entries with 20 % of them unmatched
  python scripts/gpu_join_unmatched_probe.py --child TREE --jointype inner|left
      what such a child runs, one line of output
  python scripts/gpu_join_unmatched_probe.py --disasm-compare DIR [--out FILE]
      no GPU: the five main kernels of the untracked C3 inner and left programs, compiled from this
      tree and from the tree DIR, disassembled and compared instruction by instruction; appended to FILE
  python scripts/gpu_join_unmatched_probe.py --resources [--out FILE]
      no GPU: VGPR / SGPR / scratch / LDS of the tracked kernels next to the untracked ones
"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--dim", type=float, default=1e6)
ap.add_argument("--out")
ap.add_argument("--parent-tree")
ap.add_argument("--child")
ap.add_argument("--jointype", default="inner")
ap.add_argument("--disasm-compare")
ap.add_argument("--resources", action="store_true")
ap.add_argument("--turns", type=int, default=3, help="(a): fresh processes per tree")
ap.add_argument("--only-a", action="store_true", help="(a) alone: the in-turn comparison with --parent-tree, then stop")
ap.add_argument("--scan-gbs", type=float, default=5985.0,
                help="the read rate of the scan kernel to hold (d) against: bench.py's roofline 'achieved' figure")
args = ap.parse_args()
n, nd = int(args.rows), int(args.dim)
MAIN_KERNELS = ("gpuhashjoin_main", "gpuhashjoin_main_fast", "gpuhashjoin_main_fast_narrow",
                "gpuhashjoin_main_fast_lds", "gpuhashjoin_main_fast_keyed")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def spec(jointype, tracked=False):
    return "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)%s%s))" % (
        "" if jointype == "inner" else " (jointype %s)" % jointype, " (track_matches)" if tracked else "")


def llvm(tool):
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", tool)


def code_object(tree, spec_text):
    """the program of spec_text compiled by the package at `tree` (a process of its own: one process
    loads one libstrom_hip.so): the path of its code object"""
    prog = ("import sys, os; sys.path.insert(0, %r)\n"
            "from pg_strom_amd import runtime\n"
            "from pg_strom_amd.gpuhashjoin import codegen_gpuhashjoin\n"
            "cg = codegen_gpuhashjoin(%r)\n"
            "p = runtime.DevProgram(cg.source, cg.extra_flags).wait()\n"
            "print('OBJ', os.path.join(os.path.dirname(runtime.__file__), '_cache', '%%016x.hsaco' %% p.key))\n"
            % (tree, spec_text))
    out = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, check=True, cwd=tree).stdout
    return [l for l in out.splitlines() if l.startswith("OBJ ")][0].split(None, 1)[1]


def kernel_texts(path):
    """{kernel: its instructions as text}, addresses and the comments that hold them stripped"""
    out = subprocess.run([llvm("llvm-objdump"), "-d", "--no-show-raw-insn", path],
                         capture_output=True, text=True, check=True).stdout
    res, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            res[cur] = []
            continue
        if cur and line.strip():
            res[cur].append(re.sub(r"\s*//.*$", "", line).strip())
    return res


if args.disasm_compare:
    out_lines = ["", "the five main kernels of the UNTRACKED programs, this tree against the parent's (llvm-objdump -d,",
                 "addresses stripped), instruction by instruction:"]
    for jt in ("inner", "left"):
        mine = kernel_texts(code_object(ROOT, spec(jt)))
        theirs = kernel_texts(code_object(os.path.abspath(args.disasm_compare), spec(jt)))
        for k in MAIN_KERNELS:
            same = (mine[k] == theirs[k])
            out_lines.append("  %-5s %-30s %6d instructions  %s" % (jt, k, len(mine[k]), "IDENTICAL" if same
                             else "DIFFERENT (parent: %d instructions)" % len(theirs[k])))
    print("\n".join(out_lines))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(out_lines) + "\n")
    sys.exit(0)

if args.resources:
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from star_lookup_resources import kernel_resources
    out_lines = ["GpuHashJoin kernels with and without (track_matches), gfx950, default geometry",
                 "%-8s %-9s %-30s %5s %5s %8s %7s" % ("join", "program", "kernel", "VGPR", "SGPR", "scratch", "LDS")]
    for jt in ("inner", "left"):
        for tracked in (False, True):
            res = kernel_resources(code_object(ROOT, spec(jt, tracked)))
            for k in MAIN_KERNELS + (("gpuhashjoin_unmatched", "hashjoin_matches_kernel", "hashjoin_build_index_kernel")
                                     if tracked else ("hashjoin_build_index_kernel",)):
                r = res[k]
                out_lines.append("%-8s %-9s %-30s %5d %5d %8d %7d" % (
                    jt, "tracked" if tracked else "untracked", k, r["vgpr_count"], r["sgpr_count"],
                    r["private_segment_fixed_size"], r["group_segment_fixed_size"]))
    print("\n".join(out_lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(out_lines) + "\n")
    sys.exit(0)

tree = args.child or ROOT
sys.path.insert(0, tree)


def untracked_one_pass_us(jointype, reps=12):
    import bench
    from pg_strom_amd import kds, runtime
    from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
    runtime.init()
    fact, (fk, _, _) = bench.c3_chunk_device(n, 0x5eed0003, nd)
    want = n if jointype == "left" else int((fk < nd).sum().item())
    dkey, dgrp = bench.c3_dimension(nd, 10000)
    km = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)]), [1])])
    join = GpuHashJoin(spec(jointype), row_population_ratio=1.0 if jointype == "left" else 0.8).begin(km)
    ts = []
    for _ in range(reps):
        r = join.join_chunk(fact, flags=1)
        assert r.nitems == want
        ts.append(r.perfmon["time_kern_exec_ns"] * 1e-3)
    join.end()
    return float(np.median(ts[3:]))


if args.child:
    print("CHILD %s %s median_us %.2f" % (args.child, args.jointype, untracked_one_pass_us(args.jointype)), flush=True)
    sys.exit(0)

say("join unmatched probe: %d outer rows, %d inner keys, 80 %% of the rows with a partner" % (n, nd))
if args.parent_tree:
    say("(a) untracked one-pass kernels, median us per process (%d fresh processes each, parent and this tree in turns):" % args.turns)
    for jt in ("inner", "left"):
        got = {"parent": [], "new": []}
        for label, t in [("parent", os.path.abspath(args.parent_tree)), ("new", ROOT)] * args.turns:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", t, "--jointype", jt,
                                  "--rows", str(n), "--dim", str(nd)], capture_output=True, text=True, timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith("CHILD ")]
            if out.returncode != 0 or not line:
                say("child %s failed (rc %d): %s" % (label, out.returncode, out.stderr[-400:]))
                sys.exit(1)                 # nothing more is started on the GPU after a failure
            got[label].append(float(line[0].split()[4]))
        spread = max(got["parent"]) - min(got["parent"])
        mid = float(np.median(got["new"]))
        inside = min(got["parent"]) <= mid <= max(got["parent"])
        say("  %-5s parent %s | this tree %s | parent's spread %.1f us, this tree's median %.1f: %s the parent's own range %.1f .. %.1f"
            % (jt, " ".join("%.1f" % v for v in got["parent"]), " ".join("%.1f" % v for v in got["new"]),
               spread, mid, "INSIDE" if inside else "OUTSIDE", min(got["parent"]), max(got["parent"])))
    if args.only_a:
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        sys.exit(0)

import torch  # noqa: E402
import bench  # noqa: E402
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash  # noqa: E402

runtime.init()
fact, (fk, _, _) = bench.c3_chunk_device(n, 0x5eed0003, nd)
nmatch = int((fk < nd).sum().item())
del fk
one_key = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
hot = runtime.DeviceStore.from_torch_columns(["int4"], [one_key], [(12345, 12345)])
del one_key
# the first 80 % of the key range, 1e7 rows: leaves about 20 % of the entries unmatched
g = torch.Generator(device="cuda")
g.manual_seed(0x5eed0044)
part = torch.randint(0, int(0.8 * nd), (n // 10,), dtype=torch.int32, device="cuda", generator=g)
partial = runtime.DeviceStore.from_torch_columns(["int4"], [part], [(int(part.min().item()), int(part.max().item()))])
del part
torch.cuda.empty_cache()
dkey, dgrp = bench.c3_dimension(nd, 10000)
km = build_multihash([(kds.build_kds("row_flat", [kds.Column("int4", dkey), kds.Column("int4", dgrp)]), [1])])
joins = {(jt, tr): GpuHashJoin(spec(jt, tr), row_population_ratio=1.0).begin(km)
         for jt in ("inner", "left") for tr in (False, True)}
REPS, CHUNKS = 8, 5                                 # the first round is warm-up
rows = []


def run(jt, tracked, general, chunk, want):
    """us of chunk 1 after a reset and of chunk 5, per round"""
    if general:
        os.environ["STROM_HASHJOIN_NO_FAST"] = "1"
    else:
        os.environ.pop("STROM_HASHJOIN_NO_FAST", None)
    j = joins[(jt, tracked)]
    if tracked:
        j.reset_matches()
    ts = []
    for _ in range(CHUNKS):
        r = j.join_chunk(chunk, flags=1)
        assert r.errcode == 0 and r.nitems == want, (jt, tracked, general, r.errcode, r.nitems, want)
        ts.append(r.perfmon["time_kern_exec_ns"] * 1e-3)
    return ts[0], ts[-1]


for label, chunk, wants in (("(b) C3 keys", fact, {"inner": nmatch, "left": n}), ("(c) every outer row on one key", hot, {"inner": n, "left": n})):
    cases = [(jt, tr, gen) for jt in ("inner", "left") for gen in (False, True) for tr in (False, True)]
    times = {c: [] for c in cases}
    for rep in range(REPS):
        for c in cases:
            times[c].append(run(c[0], c[1], c[2], chunk, wants[c[0]]))
    say("%s: main kernel us, median [min .. max] of %d rounds after a warm-up round; chunk 1 follows a reset (flags cold), chunk 5 is warm"
        % (label, REPS - 1))
    med = {}
    for c in cases:
        t = np.array(times[c][1:])
        med[c] = (float(np.median(t[:, 0])), float(np.median(t[:, 1])))
        say("  %-5s %-8s %-9s chunk 1 %8.1f [%8.1f .. %8.1f]   chunk 5 %8.1f [%8.1f .. %8.1f]"
            % (c[0], "general" if c[2] else "one-pass", "tracked" if c[1] else "untracked",
               med[c][0], t[:, 0].min(), t[:, 0].max(), med[c][1], t[:, 1].min(), t[:, 1].max()))
    for jt in ("inner", "left"):
        warm, general = med[(jt, True, False)][1], med[(jt, False, True)][1]
        say("  %-5s condition: warm tracked one-pass %.1f us %s untracked general %.1f us; tracking costs the warm one-pass kernel x%.2f"
            % (jt, warm, "BEATS" if warm < general else "DOES NOT BEAT", general, warm / med[(jt, False, False)][1]))

# (d) the unmatched pass
os.environ.pop("STROM_HASHJOIN_NO_FAST", None)
j = joins[("left", True)]
ts, nun = [], None
for rep in range(REPS):
    j.reset_matches()
    r = j.join_chunk(partial, flags=1)
    assert r.errcode == 0
    u = j.collect(j.submit_unmatched(flags=1))
    assert u.errcode == 0
    nun = u.nitems
    ts.append(u.perfmon["time_kern_exec_ns"] * 1e-3)
area = len(j.matches_image())
t = np.array(ts[1:])
say("(d) unmatched pass: %d of %d entries unmatched (%.1f %%), flag area %d bytes (ONE area: a byte per 32-byte granule holds"
    % (nun, nd, 100.0 * nun / nd, area))
say("    'starts' and 'matched'), %d bytes of records: %.1f us [%.1f .. %.1f] = %.0f GB/s over the area"
    % (8 * nun, float(np.median(t)), t.min(), t.max(), area / float(np.median(t)) / 1e3))
stream_us = (area + 8.0 * nun) / args.scan_gbs / 1e3
say("    its traffic, %d bytes, is %.2f us at the scan kernel's read rate (%.0f GB/s): the pass is a fixed cost (launch, one"
    % (area + 8 * nun, stream_us, args.scan_gbs))
say("    reservation per work-group), once per join")
say("(e) this is the byte per 32-byte granule; a byte per 8-byte granule was measured before it (see below); the bit layout with atomicOr was not tried")
for jn in joins.values():
    jn.end()
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
