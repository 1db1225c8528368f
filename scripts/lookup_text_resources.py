"""Registers of the fused join-and-aggregate kernels with and without text variables (no GPU
needed: hiprtc cross-compiles for gfx950).

(a) Programs WITHOUT text variables -- the three star mappings of scripts/star_lookup_resources.py,
    the one-table lookup's default mapping (the canonical scan+join+group-by program built FOR
    inner column 1, 2-byte narrow records, an int4 key) and that session's own program (the
    run-time-mapping lookup, the joined kernel) -- at this tree and at a parent revision: VGPR /
    SGPR / scratch / instruction count must be EQUAL, the text support is compiled away there.
(b) The same figures for a text mapping of each of the five kernels.  Scratch is printed as it is.

The parent's figures come from a checkout of --parent (default HEAD~1) in a temporary directory:
its library is built there and this script runs against it (--figures ROOT prints (a) as JSON).

usage: python scripts/lookup_text_resources.py [--parent REV] [> profiles/lookup_text_resources.txt]
"""
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE = ("gpupreagg_dense_lookup", "gpupreagg_packed_lookup")
STAR = ("gpupreagg_dense_lookup_star", "gpupreagg_packed_lookup_star")
JOINED = ("gpupreagg_dense_joined",)
INT_QUAL = "(and (int4lt (var 2 int4) (param 0 int4)) (float8gt (var 3 float8) (param 1 float8)))"
AGGS = "(key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"
DEFAULT_SPEC = "(gpupreagg (qual " + INT_QUAL + ") " + AGGS + ")"
# text mappings: the qual reads fact columns only (qual-first); var 4 text, var 5 character(10)
TEXT_SPEC = ("(gpupreagg (qual (and (bpchareq (var 5 character) (const character 'MAIL'))"
             " (text_lt (var 4 text) (param 0 text)))) " + AGGS + ")")
TEXT_STAR_SPEC = ("(gpupreagg (qual (bpchareq (var 5 character) (const character 'MAIL')))"
                  " (key (var 1 int4)) (key (var 6 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))")


def one_table_defines(inner_columns, reclen, narrow, keylen):
    """the define block csrc/gpupreagg.cpp (lookup_mapping_program) puts in front of the source"""
    mask = 0
    for c in inner_columns:
        mask |= 1 << c
    return ("#define GPUPREAGG_LOOKUP_ONLY 1\n#define GPUPREAGG_LOOKUP_INNER_MASK 0x%xUL\n"
            "#define GPUPREAGG_LOOKUP_RECLEN %d\n#define GPUPREAGG_LOOKUP_NARROW %d\n"
            "#define GPUPREAGG_LOOKUP_KEYLEN %d\n" % (mask, reclen, 1 if narrow else 0, keylen))


def _star_module(root):
    spec = importlib.util.spec_from_file_location("_star_lookup_resources",
                                                  os.path.join(root, "scripts", "star_lookup_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_text(root, spec, defines):
    """(DevProgram, code object path) of 'defines' + the program of 'spec', by the tree at 'root'"""
    if root not in sys.path:
        sys.path.insert(0, root)
    from pg_strom_amd import gpupreagg, runtime
    cg = gpupreagg.codegen_gpupreagg(spec)
    prog = runtime.DevProgram(defines + cg.source, cg.extra_flags).wait()
    return prog, os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)


def figures(root, res, spec, defines, kernels):
    prog, path = build_text(root, spec, defines)
    try:
        r = res.kernel_resources(path)
        cnt = res.instruction_counts(path, kernels)
        return {k: [r[k]["vgpr_count"], r[k]["sgpr_count"], r[k]["private_segment_fixed_size"]] + list(cnt[k])
                for k in kernels}
    finally:
        prog.release()


def nontext_programs(root, res):
    """[(title, spec, define block, kernels)]: every program of part (a)"""
    if root not in sys.path:
        sys.path.insert(0, root)
    from pg_strom_amd import gpupreagg
    out = [("star: " + name, spec, gpupreagg.lookup_star_defines(rels), STAR) for name, spec, rels in res.MAPPINGS]
    out.append(("one table, default mapping (inner column 1, 2-byte narrow records, int4 key)",
                DEFAULT_SPEC, one_table_defines([0], 2, True, 4), ONE))
    out.append(("the session's own program (run-time mapping; the joined kernel)", DEFAULT_SPEC, "", ONE + JOINED))
    return out


def text_programs(root):
    if root not in sys.path:
        sys.path.insert(0, root)
    from pg_strom_amd import gpupreagg
    return [("one table, text mapping (fact text + character(10) in the qual, qual-first)",
             TEXT_SPEC, one_table_defines([0], 2, True, 4), ONE),
            ("the text session's own program (run-time mapping; the joined kernel)", TEXT_SPEC, "", ONE + JOINED),
            ("star, 2 narrow relations, character(10) in the qual (qual-first)", TEXT_STAR_SPEC,
             gpupreagg.lookup_star_defines([(4, 2, True, [0]), (4, 4, True, [5])]), STAR)]


def build_library(root):
    spec = importlib.util.spec_from_file_location("_strom_build", os.path.join(root, "pg_strom_amd", "build.py"))
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)
    bm.build_library(verbose=False)


def part_a(root):
    res = _star_module(root)
    return [[title, spec, figures(root, res, spec, defs, kernels)]
            for title, spec, defs, kernels in nontext_programs(root, res)]


def parent_part_a(rev):
    tmp = tempfile.mkdtemp(prefix="lookup_text_parent_")
    try:
        tar = subprocess.run(["git", "-C", HERE, "archive", rev], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--figures", tmp],
                             capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


HEAD = "%-30s %5s %5s %8s %7s %7s %6s" % ("kernel", "VGPR", "SGPR", "scratch", "instr", "g_load", "f_load")


def row(kernel, f):
    return "%-30s %5d %5d %8d %7d %7d %6d" % ((kernel,) + tuple(f))


def main(argv):
    if len(argv) >= 2 and argv[0] == "--figures":
        # (the parent's side: its own tree builds its own library; figures as one JSON line)
        build_library(argv[1])
        print(json.dumps(part_a(argv[1])))
        return 0
    rev = argv[1] if len(argv) >= 2 and argv[0] == "--parent" else "HEAD~1"
    build_library(HERE)
    here = part_a(HERE)
    parent = parent_part_a(rev)
    revname = subprocess.run(["git", "-C", HERE, "rev-parse", "--short", rev], capture_output=True, text=True).stdout.strip()
    print("fused join-and-aggregate kernels, gfx950, session default geometry (1024 threads: 128 VGPRs a wave)")
    print("\n(a) programs without text variables: this tree against its parent %s" % revname)
    print(HEAD + "   parent")
    differ = 0
    for (title, spec, f_here), (_, _, f_parent) in zip(here, parent):
        print("\n%s\n  %s" % (title, spec))
        for k in sorted(f_here):
            same = (f_here[k] == f_parent[k])
            differ += (not same)
            print(row(k, f_here[k]) + ("   equal" if same else "   DIFFERS: " + row("", f_parent[k]).strip()))
    print("\n(a): %s" % ("every figure equals the parent's" if not differ else "%d kernel(s) DIFFER from the parent" % differ))
    print("\n(b) text mappings (new with this tree: the parent refuses them)")
    print(HEAD)
    res = _star_module(HERE)
    scratch = 0
    for title, spec, defs, kernels in text_programs(HERE):
        f = figures(HERE, res, spec, defs, kernels)
        print("\n%s\n  %s" % (title, spec))
        for k in sorted(f):
            print(row(k, f[k]))
            scratch += (f[k][2] != 0)
    print("\n(b): %s" % ("no text kernel uses scratch memory" if not scratch
                         else "%d text kernel(s) use scratch memory (figures above)" % scratch))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
