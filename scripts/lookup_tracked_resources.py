"""The tracked lookup kernels (RIGHT / FULL joins, strom_submit_gpupreagg_lookup_tracked) and the
unmatched pass: registers per mapping, and the proof that the UNTRACKED kernels did not change (no GPU
needed).

Part 1 -- for each tracked mapping below the program text is what the runtime builds for it, the define
block of gpupreagg.lookup_tracked_defines() in front of the session's source, and for the unmatched pass
the block of gpupreagg.lookup_unmatched_defines(); VGPRs, SGPRs, LDS, scratch and instruction counts are
read from the code object.  The conditions are the typed kernels' (DESIGN 3.7.1): no scratch, VGPR + AGPR
<= 128.  Every tracked mapping is printed next to its typed twin (the same mapping, tracked = 0).

Part 2 -- reported without a bar: tracked mappings next to typed twins that do not fit the register file
themselves.

Part 3 -- with --parent-tree DIR (a built checkout of the parent commit): the inner mappings and the typed
mappings of scripts/lookup_join_types_resources.py are compiled from both trees and the disassembly of the
fold kernels is compared instruction by instruction.

usage: python scripts/lookup_tracked_resources.py [--parent-tree DIR] [> profiles/lookup_tracked_resources.txt]
       (tests/test_lookup_tracked_cpu.py loads TRACKED_MAPPINGS, build_tracked(), build_unmatched() and
       kernel_resources() from here)
"""
import argparse
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def _join_types_module():
    # (it puts the tree named by --tree, or this one, in front of sys.path: import pg_strom_amd after it)
    spec = importlib.util.spec_from_file_location("_lookup_join_types_resources",
                                                  os.path.join(HERE, "lookup_join_types_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


JT = _join_types_module()
kernel_resources = JT.kernel_resources
instruction_counts = JT.instruction_counts
ONE_KERNELS, STAR_KERNELS = JT.ONE_KERNELS, JT.STAR_KERNELS
UNMATCHED_KERNELS = ("gpupreagg_dense_lookup_unmatched",)

# name, aggregate spec, relations as lookup_star_defines() takes them, join types, tracked relation, kernels.
# The typed twins of these (tracked = 0) are the first and third mapping of lookup_join_types_resources.py and
# the inner mapping of its part 2: the parent's kernels hold them without scratch.
_ONE = JT.TYPED_MAPPINGS[0]
_STAR = JT.TYPED_MAPPINGS[2]
TRACKED_MAPPINGS = [
    ("one table, RIGHT: a 4-byte narrow record serves the group key; the qual reads fact columns",
     _ONE[1], _ONE[2], ["inner"], 1, ONE_KERNELS),
    ("one table, FULL: the same mapping, left",
     _ONE[1], _ONE[2], ["left"], 1, ONE_KERNELS),
    ("star (semi, TRACKED left, anti, inner), relation 3 keyed by int8; the qual reads relations 2 and 4",
     _STAR[1], _STAR[2], ["semi", "left", "anti", "inner"], 2, STAR_KERNELS),
]

# reported without a bar, next to typed twins that spill themselves (lookup_join_types_resources.py, last section)
REPORTED_MAPPINGS = [
    ("one table serving the group key AND a pmax column, 4-byte narrow record (the GPU tests' one-table mapping)",
     JT.REPORTED_MAPPINGS[2][1], JT.REPORTED_MAPPINGS[2][2], [["inner"], ["left"]], 1, ONE_KERNELS),
    ("one table, 16-byte plain record, key only",
     JT.REPORTED_MAPPINGS[3][1], JT.REPORTED_MAPPINGS[3][2], [["inner"], ["left"]], 1, ONE_KERNELS),
]


def build_tracked(spec, relations, jointypes, tracked):
    """the tracked lookup program of a mapping, as the runtime builds it (tracked 0: the typed one)"""
    from pg_strom_amd import gpupreagg
    return JT.build_text(spec, gpupreagg.lookup_tracked_defines(relations, jointypes, tracked))


def build_unmatched(spec, relation):
    """the program of the unmatched pass over a tracked relation, as the runtime builds it"""
    from pg_strom_amd import gpupreagg
    return JT.build_text(spec, gpupreagg.lookup_unmatched_defines(relation))


def untracked_mappings():
    """the mappings whose kernels must not change: (name, spec, define block, kernels) -- inner and typed"""
    from pg_strom_amd import gpupreagg
    out = list(JT.inner_mappings())
    for name, spec, relations, jointypes, kernels in JT.TYPED_MAPPINGS:
        out.append(("typed: " + name, spec, gpupreagg.lookup_typed_defines(relations, jointypes), kernels))
    return out


def dump_untracked(outdir):
    doc = []
    for name, spec, defines, kernels in untracked_mappings():
        prog, path = JT.build_text(spec, defines)
        res = kernel_resources(path)
        dis = JT.disassembly(path, kernels)
        doc.append({"name": name, "kernels": {k: {"res": res[k], "text": dis[k]} for k in kernels}})
        prog.release()
    with open(os.path.join(outdir, "untracked.json"), "w") as f:
        json.dump(doc, f)
    return doc


def compare_with_parent(parent_tree, workdir):
    os.makedirs(workdir, exist_ok=True)
    mine = dump_untracked(workdir)
    pdir = os.path.join(workdir, "parent")
    os.makedirs(pdir, exist_ok=True)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", parent_tree, "--dump", pdir], check=True)
    with open(os.path.join(pdir, "untracked.json")) as f:
        theirs = json.load(f)
    print("\n\nuntracked kernels (inner and typed), this tree against the parent commit's (instruction text of the")
    print("disassembly, addresses stripped; sha1 of the text)")
    print("%-30s %7s %7s %5s %5s  %-12s %-12s %s" % ("kernel", "instr", "parent", "VGPR", "par.", "sha1", "parent", ""))
    differ = 0
    for a, b in zip(mine, theirs):
        assert a["name"] == b["name"]
        print("\n%s" % a["name"])
        for k in a["kernels"]:
            ta, tb = a["kernels"][k]["text"], b["kernels"][k]["text"]
            ha = hashlib.sha1("\n".join(ta).encode()).hexdigest()[:12]
            hb = hashlib.sha1("\n".join(tb).encode()).hexdigest()[:12]
            same = (ta == tb and a["kernels"][k]["res"] == b["kernels"][k]["res"])
            differ += (not same)
            print("%-30s %7d %7d %5d %5d  %-12s %-12s %s" % (k, len(ta), len(tb), a["kernels"][k]["res"]["vgpr_count"],
                                                          b["kernels"][k]["res"]["vgpr_count"], ha, hb,
                                                          "identical" if same else "DIFFERENT"))
    print("\n%s" % ("all untracked kernels identical to the parent's" if not differ
                    else "%d untracked kernel(s) differ from the parent's" % differ))
    return differ


def _row(k, label, r, cnt):
    print("%-32s %-26s %5d %5d %6d %8d %7d %7d %6d" % (k, label, r["vgpr_count"], r["sgpr_count"],
                                                      r["group_segment_fixed_size"], r["private_segment_fixed_size"],
                                                      *cnt))


def _report(agg_spec, relations, jointypes, tracked, kernels, barred):
    bad = 0
    for trk in (0, tracked):
        prog, path = build_tracked(agg_spec, relations, jointypes, trk)
        res = kernel_resources(path)
        cnt = instruction_counts(path, kernels)
        for k in kernels:
            if k not in res:
                print("%-32s %-26s (not built: the aggregates are not packable)" % (k, "/".join(jointypes)))
                continue
            _row(k, "/".join(jointypes) + (" tracked %d" % trk if trk else ""), res[k], cnt[k])
            if trk and barred:
                bad += (res[k]["private_segment_fixed_size"] != 0 or res[k]["vgpr_count"] + res[k]["agpr_count"] > 128)
        prog.release()
    prog, path = build_unmatched(agg_spec, relations[tracked - 1])
    res = kernel_resources(path)
    cnt = instruction_counts(path, UNMATCHED_KERNELS)
    for k in UNMATCHED_KERNELS:
        _row(k, "relation %d" % tracked, res[k], cnt[k])
        bad += (res[k]["private_segment_fixed_size"] != 0 or res[k]["vgpr_count"] + res[k]["agpr_count"] > 128)
    prog.release()
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: compare the untracked kernels")
    ap.add_argument("--tree", help="(internal) compile this checkout's pg_strom_amd")
    ap.add_argument("--dump", help="(internal) write the untracked mappings' disassembly into this directory and stop")
    ap.add_argument("--workdir", help="where the two trees' disassembly is kept (default: a temporary directory)")
    args = ap.parse_args()
    if args.dump:
        dump_untracked(args.dump)
        return 0
    print("tracked lookup kernels and the unmatched pass, built FOR a mapping, gfx950, session default geometry")
    print("(1024 threads: 128 VGPRs a wave); every tracked program next to its typed twin")
    print("%-32s %-26s %5s %5s %6s %8s %7s %7s %6s" % ("kernel", "join types", "VGPR", "SGPR", "LDS", "scratch", "instr",
                                                      "g_load", "f_load"))
    bad = 0
    for name, agg_spec, relations, jointypes, tracked, kernels in TRACKED_MAPPINGS:
        print("\n%s\n  %s\n  relations (keylen, reclen, narrow, columns): %r" % (name, agg_spec, relations))
        bad += _report(agg_spec, relations, jointypes, tracked, kernels, True)
    print("\n\nreported without a bar: mappings whose typed twin does not fit the register file itself")
    for name, agg_spec, relations, jointype_sets, tracked, kernels in REPORTED_MAPPINGS:
        print("\n%s\n  %s\n  relations (keylen, reclen, narrow, columns): %r" % (name, agg_spec, relations))
        for jointypes in jointype_sets:
            bad += _report(agg_spec, relations, jointypes, tracked, kernels, False)
    if args.parent_tree:
        bad += compare_with_parent(os.path.abspath(args.parent_tree), args.workdir or tempfile.mkdtemp())
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
