"""the launches of hashed GpuPreAgg folds, scenario by scenario: every route through
gpupreagg_launch_hashed (csrc/gpupreagg.cpp) at the smallest size that reaches it, and every
validated STROM_GPUPREAGG_HASH_* knob at a legal and at an illegal value.  Prints the request's
num_kern_exec / num_kern_prep per fold.  Meant to run under a kernel trace

    rocprofv3 --kernel-trace --output-format csv -- python scripts/gpu_hashed_launch_trace.py

a one-element torch fill marks the start of every scenario in the trace; `--reduce trace.csv` turns a
trace into the ordered (kernel, grid, work-group, LDS bytes) list per scenario that two builds are
compared by (profiles/hashed_launch_refactor_trace.txt).  The trace's LDS column holds a kernel's
static LDS only: the dynamic bytes of the folds and the LDS scatter do not show in it."""
import csv, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P = "STROM_GPUPREAGG_HASH_"
SPEC = "(gpupreagg (key (var 1 int8)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))"
# tests/test_sum_overflow_gpu.py's hashed shape: rows x magnitude beyond 2^63, every group's sum far from it
SPEC_WIDE = "(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)) (pmax (var 2 int8)))"


def reduce_trace(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    scenario, marked = -1, False
    for r in rows:
        name = r["Kernel_Name"]
        if "gpupreagg" not in name:
            if "FillFunctor" in name and not marked:        # (zeros() and fill_(): two fills, one mark)
                scenario += 1
                print("== scenario %d" % scenario)
            marked = "FillFunctor" in name
            continue
        marked = False
        print("%s grid=%d wg=%d lds=%d" % (name.split("(")[0], int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]),
                                           int(r["Workgroup_Size_X"]), int(r["LDS_Block_Size"])))


def main():
    import torch
    from pg_strom_amd import kds, runtime
    from pg_strom_amd.gpupreagg import GpuPreAgg
    runtime.init()
    rng = np.random.default_rng(5)
    count = [0]

    def chunk(n, ngroups, fmt="column", heavy=0.0, distinct=False):
        g = (rng.permutation(n) if distinct else rng.integers(0, ngroups, n)).astype(np.int64)
        g[rng.random(n) < heavy] = 0
        return kds.build_kds(fmt, [kds.Column("int8", g * 1000003 * 65537 - 2**59),
                                   kds.Column("int4", rng.integers(-1000, 1000, n).astype(np.int32)),
                                   kds.Column("float8", rng.random(n))])

    def scenario(name, chunks, hint=0, env=(), row_maps=None, spec=SPEC):
        for k in list(os.environ):
            if k.startswith(P):
                del os.environ[k]
        for k, v in env:
            os.environ[P + k] = str(v)
        agg = GpuPreAgg(spec).begin_hashed(ngroups_hint=hint)
        agg.program.wait()
        torch.zeros(1, device="cuda").fill_(1.0)            # the scenario's mark in the trace
        torch.cuda.synchronize()
        out = []
        for i, c in enumerate(chunks):
            st, pfm = agg.fold(c, row_map=row_maps[i] if row_maps else None)
            out.append("%d:%d/%d" % (st, pfm["num_kern_exec"], pfm["num_kern_prep"]))
        print("scenario %d %-44s %-40s status:launches/prep %s  groups %d  exact folds %d"
              % (count[0], name, " ".join("%s=%s" % kv for kv in env), " ".join(out), agg.num_groups(),
                 agg.checked_folds()), flush=True)
        count[0] += 1
        agg.end()

    small = chunk(200_000, 100)
    mid = chunk(600_000, 30_000)
    parts = chunk(600_000, 50_000)
    scenario("one role", [small])
    scenario("roles, role map", [mid], 30000, [("NO_PARTS", 1)])
    scenario("roles, no role map", [mid], 30000, [("NO_PARTS", 1), ("NO_ROLEMAP", 1)])
    scenario("roles over a ROW chunk", [chunk(200_000, 3000, "row")], 3000, [("NO_PARTS", 1)])
    scenario("roles over a host row map", [mid], 30000, [("NO_PARTS", 1)], [np.arange(0, 600_000, 2, dtype=np.int32)])
    scenario("partition plan, LDS scatter", [parts], 50000, [("PARTS_MIN", 0)])
    scenario("partition plan, direct scatter", [parts], 50000, [("PARTS_MIN", 0), ("NO_LDS_SCATTER", 1)])
    scenario("heavy key", [chunk(600_000, 50_000, heavy=0.6)], 50000, [("PARTS_MIN", 0), ("UNIT_ROWS", 1024)])
    scenario("unknown group count", [chunk((4 << 20) + 1024, 1000)])
    scenario("an empty chunk between two", [small, small, small], 0, (), [None, np.zeros(0, dtype=np.int32), None])
    n = 2_000_000
    wide = kds.build_kds("column", [kds.Column("int4", rng.integers(0, 1000, n).astype(np.int32)),
                                    kds.Column("int8", rng.integers(10**13 - 10**6, 10**13, n))])
    scenario("second attempt, exact fold, exact merge", [wide, wide], spec=SPEC_WIDE)
    # the roles' knobs over a small chunk, 40 work-groups of rows (the fold's grid is a multiple of 8 x roles);
    # CHECK_PER_CU over one large enough to reach the clamp (more than 2 x 1024 x 2 x CUs rows)
    few = (chunk(40_000, 5000), 5000, ("NO_PARTS", 1))
    role = (mid, 30000, ("NO_PARTS", 1))
    plan = (parts, 50000, ("PARTS_MIN", 0))
    large = (chunk(2_200_000, 50_000), 50000, ("PARTS_MIN", 0))
    for knob, legal, illegal, (c, hint, route) in [
            ("ROLES", 4, 3, few), ("FILL", 50, None, few), ("LDS_SLOTS", 64, 100, role), ("LDS_KB", 64, None, role),
            ("PARTS", 1024, 100, plan), ("FOLD_BLOCK", 512, 300, plan), ("SCATTER_BLOCK", 256, None, plan),
            ("SCATTER_ROWS", 2, None, plan), ("CHECK_BLOCK", 256, 300, plan), ("CHECK_PER_CU", 4, None, large),
            ("UNIT_LDS_KB", 64, None, plan)]:
        for v in (legal, illegal):
            if v is not None:
                scenario("knob", [c], hint, [route, (knob, v)])
    # growth from an empty table (tests/test_gpupreagg_gpu.py: 4M distinct keys): how much turn 0
    # defers depends on which threads claim first, so the later turns differ from run to run
    grow = chunk(4_000_000, 0, distinct=True)
    scenario("growth, roles", [grow], 0, [("NO_PARTS", 1)])
    scenario("growth, partition plan, LDS scatter", [grow], 0, [("PARTS_MIN", 0)])
    scenario("growth, partition plan, direct scatter", [grow], 0, [("PARTS_MIN", 0), ("NO_LDS_SCATTER", 1)])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--reduce":
        reduce_trace(sys.argv[2])
    else:
        main()
