"""fact JOIN dim WHERE fact.c = 'MAIL' GROUP BY dim.g over one resident fact chunk, c character(10):
  (i)   the one-table lookup with WHERE bpchareq(fact.c, 'MAIL') (strom_submit_gpupreagg_lookup):
        the kernel turns c's offsets into addresses and compares the datums
  (ii)  the only plan before the lookup took text: the general join, the COLUMN projection
        carrying c (strom_hashjoin_project_column), then the plain fold of the joined chunk
  (iii) the lookup with an integer qual of the same selectivity (a < 2^31 / 7): what a request
        without text costs; run with --int-only at the parent revision too (--root PARENT_TREE),
        and hand that output in with --parent-int FILE, to show that such requests did not move
The star probe's shape (scripts/gpu_star_probe.py) with one dimension and the added column:
fact(k1 int4, a int4, b float8, c character(10)), c uniform over seven ship modes, 80 % of the keys
have a partner, 1000 groups.  5e7 rows by default: with c's offsets and datums a chunk of 1e8 rows
passes the 4 GB a chunk's length field holds.  One process, the plans alternating, warm programs,
three repetitions.  Asserts that (i)'s partial rows equal (ii)'s.  No threshold.
usage: gpu_lookup_text_probe.py [--root DIR] [--int-only] [--parent-int FILE] [nrows] [outfile]"""
import os
import sys
import time

import numpy as np

args = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
int_only, parent_int = False, None
while args and args[0].startswith("--"):
    if args[0] == "--root":
        ROOT = os.path.abspath(args[1])
        args = args[2:]
    elif args[0] == "--parent-int":
        parent_int = args[1]
        args = args[2:]
    else:
        int_only = (args[0] == "--int-only")
        args = args[1:]
sys.path.insert(0, ROOT)
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd._lib import lib  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash  # noqa: E402
from pg_strom_amd.gpupreagg import GpuPreAgg  # noqa: E402

n = int(float(args[0])) if len(args) > 0 else 50_000_000
outfile = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "lookup_text_probe.txt")
nd, ngroups, REPS = 1_000_000, 1000, 3
MODES = [b"MAIL", b"SHIP", b"TRUCK", b"AIR", b"REG AIR", b"RAIL", b"FOB"]
AGGS = "(key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"
TEXT_SPEC = "(gpupreagg (qual (bpchareq (var 4 character) (const character 'MAIL'))) " + AGGS + ")"
INT_SPEC = "(gpupreagg (qual (int4lt (var 2 int4) (param 0 int4))) " + AGGS + ")"
INT_EXT = [np.int32(2**31 // 7)]
COLUMNS = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8"), (0, 4, "character")]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def rows_of(pr):
    keys = np.where(pr.column(0)[1], 10**9, pr.column(0)[0].astype(np.int64))
    order = np.argsort(keys)
    return [keys[order]] + [pr.column(c)[0][order] for c in range(1, len(pr.targets))]


def fold_ms(pfm):
    return (pfm["time_kern_exec_ns"] - pfm["time_kern_proj_ns"]) * 1e-6


runtime.init()
rng = np.random.default_rng(13)
span = int(nd * 1.25)                           # 80 % of the fact keys have a partner
k1 = rng.integers(0, span, n, dtype=np.int64).astype(np.int32)
a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
b = rng.random(n)
# character(10): one datum per ship mode, a row's entry is its datum's address
ccol = kds.Column("character", [(m + b" " * 10)[:10] for m in MODES])
ccol.values = np.ascontiguousarray(ccol.values[rng.integers(0, len(MODES), n)])
fact = kds.build_kds("column", [kds.Column("int4", k1), kds.Column("int4", a), kds.Column("float8", b), ccol])
del k1, a, b
ds = runtime.DeviceStore.upload(fact)
nbytes = len(fact)
del fact
dk = rng.permutation(span)[:nd].astype(np.int32)
inner = kds.build_kds("row_flat", [kds.Column("int4", dk), kds.Column("int4", (dk % ngroups).astype(np.int32))])
join = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(build_multihash([(inner, [1])]))
say("lookup text probe%s: %d fact rows (a chunk of %.2f GB), 1 dimension of %d rows (key span %d), %d groups, "
    "the WHERE keeps 1 row in 7, %d repetitions" % (" (integer qual only)" if int_only else "", n, nbytes / 1e9,
                                                  nd, span, ngroups, REPS))
intq = GpuPreAgg(INT_SPEC).begin([(0, ngroups)], ext_params=INT_EXT)
if not int_only:
    look = GpuPreAgg(TEXT_SPEC).begin([(0, ngroups)])
    plain = GpuPreAgg(TEXT_SPEC).begin([(0, ngroups)])
t = {k: [] for k in ("i_wall", "i_dev", "ii_wall", "ii_fold_dev", "iii_wall", "iii_dev")}
nitems = 0
for rep in range(-1, REPS):                     # (rep -1 warms programs, the table and its slot records)
    if not int_only:
        look.reset()
        lib.strom_synchronize()
        t0 = time.perf_counter()
        st, pfm_i = look.collect(look.submit_lookup(join, ds, COLUMNS))
        t1 = time.perf_counter()
        assert st == 0
        rows_i = rows_of(look.fetch())

        plain.reset()
        lib.strom_synchronize()
        t2 = time.perf_counter()
        joined, nitems = join.join_to_column(ds, COLUMNS)
        st, pfm_ii = plain.fold(joined)
        t3 = time.perf_counter()
        assert st == 0
        joined.release()
        rows_ii = rows_of(plain.fetch())
        assert len(rows_i) == len(rows_ii) and np.array_equal(rows_i[0], rows_ii[0])
        assert np.array_equal(rows_i[1], rows_ii[1]) and np.array_equal(rows_i[2], rows_ii[2])
        assert np.allclose(rows_i[3], rows_ii[3], rtol=1e-12, atol=0)

    intq.reset()
    lib.strom_synchronize()
    t4 = time.perf_counter()
    st, pfm_iii = intq.collect(intq.submit_lookup(join, ds, COLUMNS[:3]))
    t5 = time.perf_counter()
    assert st == 0
    if rep < 0:
        continue
    if not int_only:
        t["i_wall"].append((t1 - t0) * 1e3)
        t["i_dev"].append(fold_ms(pfm_i))
        t["ii_wall"].append((t3 - t2) * 1e3)
        t["ii_fold_dev"].append(fold_ms(pfm_ii))
    t["iii_wall"].append((t5 - t4) * 1e3)
    t["iii_dev"].append(fold_ms(pfm_iii))
fmt = lambda v: "[" + " ".join("%.3f" % x for x in v) + "]"     # noqa: E731
if not int_only:
    say("  %d joined rows (%.1f %% of the fact rows), %d of the groups' rows counted by (i)"
        % (nitems, 100.0 * nitems / n, int(rows_i[1].sum())))
    say("  (i)   lookup, bpchareq(c, 'MAIL')      fold kernel %s ms   wall %s ms" % (fmt(t["i_dev"]), fmt(t["i_wall"])))
    say("  (ii)  join + column(c) + plain fold   fold kernel %s ms   wall %s ms" % (fmt(t["ii_fold_dev"]), fmt(t["ii_wall"])))
say("  (iii) lookup, integer qual, this tree fold kernel %s ms   wall %s ms" % (fmt(t["iii_dev"]), fmt(t["iii_wall"])))
if parent_int:
    for line in open(parent_int).read().splitlines():
        if line.startswith("  (iii)"):
            say(line.replace("this tree", "the parent "))
if not int_only:
    i_w, ii_w, iii_w = np.median(t["i_wall"]), np.median(t["ii_wall"]), np.median(t["iii_wall"])
    say("  (ii) / (i) wall = %.2f; (i) / (iii) wall = %.2f, fold kernel %.2f (medians)"
        % (ii_w / i_w, i_w / iii_w, np.median(t["i_dev"]) / np.median(t["iii_dev"])))
    say("  partial rows of (i) == partial rows of (ii): keys, counts and integer sums identical, float8 sums within 1e-12")
    look.end()
    plain.end()
intq.end()
join.end()
ds.release()
with open(outfile, "w") as f:
    f.write("\n".join(lines) + "\n")
