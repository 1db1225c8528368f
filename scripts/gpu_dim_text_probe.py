"""SELECT d.t, count(*), sum(a), sum(b) FROM fact JOIN d ON fact.k = d.k WHERE ... GROUP BY d.t over a resident
fact chunk, d.t a text column with few distinct values, three ways:
  (a) the coded column: strom_textdict_encode_table once per table (timed apart: its kernels from
      strom_textdict_kernel_ns, and wall), then the one-table lookup (strom_submit_gpupreagg_lookup) grouping
      by the ids
  (b) the plan that exists without it: the join, the COLUMN projection carrying the text column
      (strom_hashjoin_project_column), strom_textdict_encode of the projected chunk, the plain fold.  Its
      dictionary is kept between the repetitions: every key is known, the encode's steady state
  (c) the floor: the same lookup grouping by an int4 column of the dimension with the same cardinality
fact(k int4, a int4, b float8), a dimension of 1e6 rows over 1.25e6 key values (80 % of the fact keys have a
partner), 1000 distinct 14-byte values, a WHERE that keeps ~50 %.  One process, the plans alternating, warm
programs, three repetitions.  Asserts that (a) and (b) give the same (key bytes -> aggregates) map and that
(a)'s groups are (c)'s under word[g].  Writes profiles/dim_text_lookup_probe.txt.
usage: gpu_dim_text_probe.py [nrows] [nd] [nkeys] [outfile]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_strom_amd import kds, runtime  # noqa: E402
from pg_strom_amd._lib import lib  # noqa: E402
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash  # noqa: E402
from pg_strom_amd.gpupreagg import GpuPreAgg  # noqa: E402
from pg_strom_amd.textdict import TextDictionary, ids_to_keys  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
nd = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
NKEYS = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1000
outfile = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "dim_text_lookup_probe.txt")
REPS = 3
QUAL = "(and (int4lt (var 2 int4) (param 0 int4)) (float8gt (var 3 float8) (param 1 float8)))"
EXT = [np.int32(2**30 - 1), 0.0]                # a < 2^30 of [0, 2^31): 50 %
SPEC = "(gpupreagg (qual " + QUAL + ") (key (var 1 int4)) (nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8)))"
JOIN = "(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def fmt(v):
    return "[" + " ".join("%.3f" % x for x in v) + "]"


def groups(pr, keys):
    """{key: (nrows, sum a, sum b)}; keys[i] names partial row i"""
    c, sa, sb = pr.column(1)[0], pr.column(2)[0], pr.column(3)[0]
    return {k: (int(c[i]), int(sa[i]), float(sb[i])) for i, k in enumerate(keys)}


def same(g1, g2):
    assert set(g1) == set(g2)
    for k, (c, sa, sb) in g1.items():
        assert g2[k][0] == c and g2[k][1] == sa and np.isclose(g2[k][2], sb, rtol=1e-12, atol=0), k


runtime.init()
rng = np.random.default_rng(23)
span = int(nd * 1.25)
k = rng.integers(0, span, n, dtype=np.int64).astype(np.int32)
a = rng.integers(0, 2**31, n, dtype=np.int64).astype(np.int32)
b = rng.random(n)
fact = kds.build_kds("column", [kds.Column("int4", k), kds.Column("int4", a), kds.Column("float8", b)])
del k, a, b
ds = runtime.DeviceStore.upload(fact)
del fact
words = [b"key-%010d" % i for i in range(NKEYS)]            # 14 bytes each
say("dimension text probe: %d fact rows, a dimension of %d rows over %d key values, %d distinct %d-byte values, "
    "WHERE keeps 50 %%, %d repetitions" % (n, nd, span, NKEYS, len(words[0]), REPS))
dk = rng.permutation(span)[:nd].astype(np.int32)
g = (dk % NKEYS).astype(np.int32)
tcol = kds.Column("text", words)
tcol.values = np.ascontiguousarray(tcol.values[g])          # one datum buffer per distinct value
dim = kds.build_kds("row_flat", [kds.Column("int4", dk), kds.Column("int4", g), tcol])
km = build_multihash([(dim, [1])])
join = GpuHashJoin(JOIN).begin(km)

# the one-off encode per table: a NEW table of the same rows and a new dictionary, programs warm
enc_ns, enc_wall = [], []
for rep in range(-1, REPS):
    t_join = GpuHashJoin(JOIN).begin(km)
    d = TextDictionary("text")
    lib.strom_synchronize()
    t0 = time.perf_counter()
    d.encode_table(t_join, 2)
    t1 = time.perf_counter()
    if rep >= 0:
        enc_ns.append(d.kernel_ns())
        enc_wall.append((t1 - t0) * 1e3)
    assert d.num_keys == NKEYS
    d.release()
    t_join.end()

dic, old = TextDictionary("text"), TextDictionary("text")
coded = dic.encode_table(join, 2)
cols_a = [(1, coded + 1, "int4"), (0, 2, "int4"), (0, 3, "float8")]
cols_b = [(1, 3, "text"), (0, 2, "int4"), (0, 3, "float8")]
cols_c = [(1, 2, "int4"), (0, 2, "int4"), (0, 3, "float8")]
sa_, sb_, sc_ = (GpuPreAgg(SPEC).begin([(0, NKEYS)], ext_params=EXT) for _ in range(3))
t = {"a_wall": [], "a_dev": [], "b_wall": [], "b_parts": [], "c_wall": [], "c_dev": []}
packed = {}
for rep in range(-1, REPS):                     # (rep -1 warms programs, slot records and (b)'s dictionary)
    sa_.reset()
    lib.strom_synchronize()
    t0 = time.perf_counter()
    st, pfm_a = sa_.collect(sa_.submit_lookup(join, ds, cols_a))
    t1 = time.perf_counter()
    assert st == 0
    pr_a = sa_.fetch()

    sb_.reset()
    lib.strom_synchronize()
    t2 = time.perf_counter()
    joined, nitems = join.join_to_column(ds, cols_b)
    t3 = time.perf_counter()
    enc = old.encode(joined, [0], [1, 2])
    t4 = time.perf_counter()
    st, pfm_b = sb_.fold(enc)
    t5 = time.perf_counter()
    assert st == 0
    joined.release()
    enc.release()
    pr_b = sb_.fetch()

    sc_.reset()
    lib.strom_synchronize()
    t6 = time.perf_counter()
    st, pfm_c = sc_.collect(sc_.submit_lookup(join, ds, cols_c))
    t7 = time.perf_counter()
    assert st == 0
    pr_c = sc_.fetch()
    packed = {"a": pfm_a["num_kern_prep"], "c": pfm_c["num_kern_prep"]}

    ga = groups(pr_a, ids_to_keys(pr_a, [dic])[0])
    same(ga, groups(pr_b, ids_to_keys(pr_b, [old])[0]))
    same(ga, groups(pr_c, [None if nul else words[int(v)] for v, nul in zip(*pr_c.column(0))]))
    if rep < 0:
        continue
    t["a_wall"].append((t1 - t0) * 1e3)
    t["a_dev"].append((pfm_a["time_kern_exec_ns"] - pfm_a["time_kern_proj_ns"]) * 1e-6)
    t["b_wall"].append((t5 - t2) * 1e3)
    t["b_parts"].append(((t3 - t2) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3))
    t["c_wall"].append((t7 - t6) * 1e3)
    t["c_dev"].append((pfm_c["time_kern_exec_ns"] - pfm_c["time_kern_proj_ns"]) * 1e-6)

say("\n%d joined rows (%.1f %% of the fact rows), %d groups; packed accumulators: coded %d, floor %d"
    % (nitems, 100.0 * nitems / n, len(ga), packed["a"], packed["c"]))
say("  encode_table, once per table (%d slots): wall %s ms; kernels probe (with the offsets pass) %s, settle %s, "
    "emit %s, rebuild %s ms"
    % (span, fmt(enc_wall), fmt([x["probe"] * 1e-6 for x in enc_ns]), fmt([x["settle"] * 1e-6 for x in enc_ns]),
       fmt([x["emit"] * 1e-6 for x in enc_ns]), fmt([x["rebuild"] * 1e-6 for x in enc_ns])))
say("  (a) lookup by the coded column  fold kernel %s ms   wall %s ms" % (fmt(t["a_dev"]), fmt(t["a_wall"])))
say("  (b) join + column + encode + fold                          wall %s ms" % fmt(t["b_wall"]))
say("      of which join + projection %s, encode %s, fold %s ms"
    % tuple(fmt([p[i] for p in t["b_parts"]]) for i in range(3)))
say("  (c) floor: lookup by an int4    fold kernel %s ms   wall %s ms" % (fmt(t["c_dev"]), fmt(t["c_wall"])))
a_w, b_w, c_w = np.median(t["a_wall"]), np.median(t["b_wall"]), np.median(t["c_wall"])
a_d, c_d = np.median(t["a_dev"]), np.median(t["c_dev"])
say("  (b) / (a) wall = %.2f (medians; spread of the repetitions: (a) %.3f ms, (b) %.3f ms, (c) %.3f ms)"
    % (b_w / a_w, max(t["a_wall"]) - min(t["a_wall"]), max(t["b_wall"]) - min(t["b_wall"]),
       max(t["c_wall"]) - min(t["c_wall"])))
say("  (a) - (c): fold kernel %+.3f ms (x %.3f; spread (a) %.3f ms, (c) %.3f ms), wall %+.3f ms"
    % (a_d - c_d, a_d / c_d, max(t["a_dev"]) - min(t["a_dev"]), max(t["c_dev"]) - min(t["c_dev"]), a_w - c_w))
say("  (a) == (b) as (key bytes -> count, integer sum, float8 sum within 1e-12) maps; (a) == (c) under word[g]")
for obj in (sa_, sb_, sc_, join):
    obj.end()
dic.release()
old.release()
ds.release()
with open(outfile, "w") as f:
    f.write("\n".join(lines) + "\n")
