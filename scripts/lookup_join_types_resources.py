"""The typed lookup kernels (LEFT / SEMI / ANTI relations, strom_submit_gpupreagg_lookup_typed):
registers per mapping, and the proof that the INNER kernels did not change (no GPU needed).

Part 1 -- for each typed mapping below the program text is what the runtime builds for it, the
define block of gpupreagg.lookup_typed_defines() in front of the session's source; VGPRs, SGPRs,
LDS, scratch and instruction counts of the dense and packed kernel are read from the code object.
The conditions are the star's: no scratch, VGPR + AGPR <= 128.

Part 2 -- with --parent-tree DIR (a built checkout of the parent commit): the one-table inner
mapping and the three star mappings of scripts/star_lookup_resources.py are compiled from both
trees and the disassembly of gpupreagg_dense_lookup / gpupreagg_packed_lookup (one table) and
their _star forms is compared instruction by instruction.

usage: python scripts/lookup_join_types_resources.py [--parent-tree DIR] [> profiles/lookup_join_types_resources.txt]
       (tests/test_lookup_join_types_cpu.py loads TYPED_MAPPINGS, build() and kernel_resources() from here)
"""
import argparse
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _tree_from_argv():
    for i, a in enumerate(sys.argv):
        if a == "--tree" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
    return ROOT


TREE = _tree_from_argv()            # the checkout whose pg_strom_amd is compiled (--tree: the parent's)
if TREE not in sys.path:
    sys.path.insert(0, TREE)


def _star_module():
    spec = importlib.util.spec_from_file_location("_star_lookup_resources", os.path.join(HERE, "star_lookup_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


STAR = _star_module()
kernel_resources = STAR.kernel_resources
instruction_counts = STAR.instruction_counts

ONE_KERNELS = ("gpupreagg_dense_lookup", "gpupreagg_packed_lookup")
STAR_KERNELS = STAR.KERNELS
QUAL_OUTER = STAR.QUAL_OUTER
AGGS = STAR.AGGS

# name, aggregate spec, relations as lookup_star_defines() takes them, join types, kernels
TYPED_MAPPINGS = [
    ("one table, LEFT: a 4-byte narrow record serves the group key; qual first",
     "(gpupreagg (qual " + QUAL_OUTER + ") (key (var 1 int4)) " + AGGS + ")",
     [(4, 4, True, [0])], ["left"], ONE_KERNELS),
    ("one table, ANTI: the 2-byte presence record, no column; qual first",
     "(gpupreagg (qual (int4lt (var 2 int4) (param 0 int4))) (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))))",
     [(4, 2, True, [])], ["anti"], ONE_KERNELS),
    ("star (semi, left, anti, inner), relation 3 keyed by int8; the qual reads relations 2 and 4",
     "(gpupreagg (qual (and " + QUAL_OUTER + " (int4lt (var 5 int4) (param 2 int4))"
     " (int4gt (var 6 int4) (param 3 int4))))"
     " (key (var 1 int4)) (key (var 4 int4)) " + AGGS + ")",
     [(4, 2, True, []), (4, 4, True, [3, 4]), (8, 2, True, []), (4, 2, True, [5])],
     ["semi", "left", "anti", "inner"], STAR_KERNELS),
]

# Reported without a bar: mappings at which these kernels do NOT all fit the register file, typed and inner side
# by side -- which spills came with the join types and which are older.  (name, spec, relations, [join types], kernels)
_FACTKEY = "(gpupreagg (qual " + QUAL_OUTER + ") (key (var 1 int4)) " + AGGS + ")"
_NOQUAL = "(gpupreagg (key (var 1 int4)) " + AGGS + ")"
_FOUR = [(4, 2, True, [0]), (4, 2, True, [3]), (8, 2, True, []), (4, 2, True, [5])]
REPORTED_MAPPINGS = [
    ("one table, no dimension column: the key and three streamed fact columns, qual first (SEMI / ANTI grouped by a"
     " fact column; the timing probe's mapping)",
     _FACTKEY, [(4, 2, True, [])], [["inner"], ["semi"], ["anti"], ["left"]], ONE_KERNELS),
    ("the same without a qual", _NOQUAL, [(4, 2, True, [])], [["inner"], ["semi"], ["anti"], ["left"]], ONE_KERNELS),
    ("one table serving the group key AND a pmax column, 4-byte narrow record (most one-table LEFT tests; pmax of a"
     " dimension column is not packable: no packed kernel)",
     _FACTKEY[:-1] + " (pmax (var 4 int4)))", [(4, 4, True, [0, 3])], [["inner"], ["left"]], ONE_KERNELS),
    ("one table, 16-byte plain record, key only", _FACTKEY, [(4, 16, False, [0])], [["inner"], ["left"]], ONE_KERNELS),
    ("star of four narrow relations, a program of 24 bytes a row: the code generator keeps GPUPREAGG_QUADS 2 (it sizes"
     " the tile by the program's variables and does not count join keys)",
     "(gpupreagg (qual (and " + QUAL_OUTER + " (int4gt (var 6 int4) (param 2 int4))))"
     " (key (var 1 int4)) (key (var 4 int4)) " + AGGS + ")",
     _FOUR, [["inner"] * 4, ["inner", "left", "anti", "inner"], ["left", "left", "anti", "inner"]], STAR_KERNELS),
    ("star of four narrow relations, the four-relation mapping of scripts/star_lookup_resources.py (28 bytes a row,"
     " GPUPREAGG_QUADS 1)",
     STAR.MAPPINGS[2][1], STAR.MAPPINGS[2][2], [["inner"] * 4, ["inner", "left", "inner", "inner"], ["left"] * 4],
     STAR_KERNELS),
]

# the inner mappings whose kernels must not change: (name, spec, define block, kernels).  The
# one-table block is written out: the parent tree has no function that gives it.
ONE_TABLE_INNER_DEFINES = ("#define GPUPREAGG_LOOKUP_ONLY 1\n#define GPUPREAGG_LOOKUP_INNER_MASK 0x1UL\n"
                           "#define GPUPREAGG_LOOKUP_RECLEN 4\n#define GPUPREAGG_LOOKUP_NARROW 1\n"
                           "#define GPUPREAGG_LOOKUP_KEYLEN 4\n")
ONE_TABLE_INNER = ("one table, inner: a 4-byte narrow record serves the group key; qual first",
                   "(gpupreagg (qual " + QUAL_OUTER + ") (key (var 1 int4)) " + AGGS + ")",
                   [(4, 4, True, [0])])


def inner_mappings():
    from pg_strom_amd import gpupreagg
    out = [(ONE_TABLE_INNER[0], ONE_TABLE_INNER[1], ONE_TABLE_INNER_DEFINES, ONE_KERNELS)]
    for name, spec, relations in STAR.MAPPINGS:
        out.append(("star: " + name, spec, gpupreagg.lookup_star_defines(relations), STAR_KERNELS))
    return out


def build_text(spec, defines):
    """a program of the session's source behind a define block, compiled: (DevProgram, code object path)"""
    from pg_strom_amd import gpupreagg, runtime
    cg = gpupreagg.codegen_gpupreagg(spec)
    prog = runtime.DevProgram(defines + cg.source, cg.extra_flags).wait()
    return prog, os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)


def build(spec, relations, jointypes):
    """the typed lookup program of a mapping, as the runtime builds it"""
    from pg_strom_amd import gpupreagg
    return build_text(spec, gpupreagg.lookup_typed_defines(relations, jointypes))


def disassembly(path, names):
    """{kernel: [instruction text]} -- addresses and symbol offsets stripped"""
    out = subprocess.run([STAR._llvm("llvm-objdump"), "-d", "--no-show-raw-insn", path],
                         capture_output=True, text=True, check=True).stdout
    res, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                res[cur] = []
            continue
        if cur and re.match(r"^\s+[a-z_0-9]+(\s|$)", line):
            res[cur].append(re.sub(r"\s*//.*$", "", line).strip())
    return res


def dump_inner(outdir):
    """the inner mappings' kernels as this TREE compiles them, one JSON file"""
    doc = []
    for name, spec, defines, kernels in inner_mappings():
        prog, path = build_text(spec, defines)
        res = kernel_resources(path)
        dis = disassembly(path, kernels)
        doc.append({"name": name, "kernels": {k: {"res": res[k], "text": dis[k]} for k in kernels}})
        prog.release()
    with open(os.path.join(outdir, "inner.json"), "w") as f:
        json.dump(doc, f)
    return doc


def compare_with_parent(parent_tree, workdir):
    os.makedirs(workdir, exist_ok=True)
    mine = dump_inner(workdir)
    pdir = os.path.join(workdir, "parent")
    os.makedirs(pdir, exist_ok=True)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", parent_tree, "--dump", pdir], check=True)
    with open(os.path.join(pdir, "inner.json")) as f:
        theirs = json.load(f)
    print("\ninner kernels, this tree against the parent commit's (instruction text of the disassembly,")
    print("addresses stripped; sha1 of the text)")
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
    print("\n%s" % ("all inner kernels identical to the parent's" if not differ
                    else "%d inner kernel(s) differ from the parent's" % differ))
    return differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: compare the inner kernels")
    ap.add_argument("--tree", help="(internal) compile this checkout's pg_strom_amd")
    ap.add_argument("--dump", help="(internal) write the inner mappings' disassembly into this directory and stop")
    ap.add_argument("--workdir", help="where the two trees' disassembly is kept (default: a temporary directory)")
    args = ap.parse_args()
    if args.dump:
        dump_inner(args.dump)
        return 0
    print("typed lookup kernels built FOR a mapping, gfx950, session default geometry (1024 threads: 128 VGPRs a wave)")
    print("%-30s %5s %5s %6s %8s %7s %7s %6s" % ("kernel", "VGPR", "SGPR", "LDS", "scratch", "instr", "g_load", "f_load"))
    bad = 0
    for name, agg_spec, relations, jointypes, kernels in TYPED_MAPPINGS:
        prog, path = build(agg_spec, relations, jointypes)
        res = kernel_resources(path)
        cnt = instruction_counts(path, kernels)
        print("\n%s\n  %s\n  relations (keylen, reclen, narrow, columns): %r\n  join types: %r"
              % (name, agg_spec, relations, jointypes))
        for k in kernels:
            r = res[k]
            print("%-30s %5d %5d %6d %8d %7d %7d %6d" % (k, r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"],
                                                       r["private_segment_fixed_size"], *cnt[k]))
            bad += (r["private_segment_fixed_size"] != 0 or r["vgpr_count"] + r["agpr_count"] > 128)
        prog.release()
    print("\n\nreported without a bar: mappings at which the kernels do not all fit, typed next to inner")
    print("%-30s %-28s %5s %5s %8s %7s" % ("kernel", "join types", "VGPR", "SGPR", "scratch", "instr"))
    for name, agg_spec, relations, jointype_sets, kernels in REPORTED_MAPPINGS:
        print("\n%s\n  %s\n  relations (keylen, reclen, narrow, columns): %r" % (name, agg_spec, relations))
        for jointypes in jointype_sets:
            prog, path = build(agg_spec, relations, jointypes)
            res = kernel_resources(path)
            cnt = instruction_counts(path, kernels)
            for k in kernels:
                if k not in res:
                    print("%-30s %-28s (not built: the aggregates are not packable)" % (k, "/".join(jointypes)))
                    continue
                r = res[k]
                print("%-30s %-28s %5d %5d %8d %7d" % (k, "/".join(jointypes), r["vgpr_count"], r["sgpr_count"],
                                                       r["private_segment_fixed_size"], cnt[k][0]))
            prog.release()
    if args.parent_tree:
        import tempfile
        bad += compare_with_parent(os.path.abspath(args.parent_tree), args.workdir or tempfile.mkdtemp())
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
