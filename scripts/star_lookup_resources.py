"""The star lookup kernels' registers per mapping (no GPU needed: hiprtc cross-compiles).

For each mapping below the program text is what the runtime builds for it -- the define block of
gpupreagg.lookup_star_defines() in front of the session's source -- and VGPRs, SGPRs, scratch and
instruction counts of gpupreagg_dense_lookup_star / gpupreagg_packed_lookup_star are read from
the code object.  The condition: private_segment_fixed_size == 0 for all of them.

usage: python scripts/star_lookup_resources.py [> profiles/star_lookup_resources.txt]
       (tests/test_star_lookup_cpu.py loads MAPPINGS, build() and kernel_resources() from here)
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("gpupreagg_dense_lookup_star", "gpupreagg_packed_lookup_star")
QUAL_OUTER = "(and (int4lt (var 2 int4) (param 0 int4)) (float8gt (var 3 float8) (param 1 float8)))"
AGGS = "(nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"

# name, aggregate spec, relations as lookup_star_defines() takes them:
# (key length, slot record length, narrow?, [0-based virtual columns served])
MAPPINGS = [
    ("2 relations, both narrow (2- and 4-byte records); qual first",
     "(gpupreagg (qual " + QUAL_OUTER + ") (key (var 1 int4)) (key (var 4 int4)) " + AGGS + ")",
     [(4, 2, True, [0]), (4, 4, True, [3])]),
    ("2 relations, 8-byte and 16-byte records; the qual reads relation 2",
     "(gpupreagg (qual (and " + QUAL_OUTER + " (float8gt (var 4 float8) (param 2 float8))))"
     " (key (var 1 int4)) " + AGGS + ")",
     [(4, 8, False, [0]), (4, 16, False, [3])]),
    ("4 relations, all narrow, relation 3 keyed by int8; the qual reads relations 3 and 4",
     "(gpupreagg (qual (and " + QUAL_OUTER + " (int4lt (var 5 int4) (param 2 int4))"
     " (int4gt (var 6 int4) (param 3 int4))))"
     " (key (var 1 int4)) (key (var 4 int4)) " + AGGS + ")",
     [(4, 2, True, [0]), (4, 2, True, [3]), (8, 4, True, [4]), (4, 2, True, [5])]),
]


def build(spec, relations):
    """the star program of a mapping, compiled: (DevProgram, path of its code object)"""
    from pg_strom_amd import gpupreagg, runtime
    cg = gpupreagg.codegen_gpupreagg(spec)
    source = gpupreagg.lookup_star_defines(relations) + cg.source
    prog = runtime.DevProgram(source, cg.extra_flags).wait()
    return prog, os.path.join(os.path.dirname(runtime.__file__), "_cache", "%016x.hsaco" % prog.key)


def _llvm(tool):
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", tool)


def kernel_resources(path):
    """{kernel: {vgpr_count, sgpr_count, private_segment_fixed_size, ...}} from the code object's notes"""
    out = subprocess.run([_llvm("llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    res = {}
    # a kernel's metadata map is sorted by key: .agpr_count first, .wavefront_size last
    for m in re.finditer(r"\.agpr_count:.*?\.wavefront_size", out, re.S):
        body = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", body).group(1)
        res[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))
                     for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                               "private_segment_fixed_size")}
    return res


def instruction_counts(path, names):
    """{kernel: (instructions, global/flat loads)} from the disassembly"""
    out = subprocess.run([_llvm("llvm-objdump"), "-d", "--no-show-raw-insn", path],
                         capture_output=True, text=True, check=True).stdout
    counts, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                counts[cur] = [0, 0, 0]
            continue
        if cur and re.match(r"^\s+[a-z_0-9]+(\s|$)", line):
            counts[cur][0] += 1
            op = line.split()[0]
            if op.startswith("global_load"):
                counts[cur][1] += 1
            elif op.startswith("flat_load"):
                counts[cur][2] += 1
    return counts


def main():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_strom_build", os.path.join(ROOT, "pg_strom_amd", "build.py"))
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)
    bm.build_library(verbose=False)
    print("star lookup kernels built FOR a mapping, gfx950, session default geometry (1024 threads: 128 VGPRs a wave)")
    print("%-30s %5s %5s %8s %7s %7s %6s" % ("kernel", "VGPR", "SGPR", "scratch", "instr", "g_load", "f_load"))
    bad = 0
    for name, agg_spec, relations in MAPPINGS:
        prog, path = build(agg_spec, relations)
        res = kernel_resources(path)
        cnt = instruction_counts(path, KERNELS)
        print("\n%s\n  %s\n  relations (keylen, reclen, narrow, columns): %r" % (name, agg_spec, relations))
        for k in KERNELS:
            r = res[k]
            print("%-30s %5d %5d %8d %7d %7d %6d" % (k, r["vgpr_count"], r["sgpr_count"],
                                                     r["private_segment_fixed_size"], *cnt[k]))
            bad += (r["private_segment_fixed_size"] != 0)
        prog.release()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
