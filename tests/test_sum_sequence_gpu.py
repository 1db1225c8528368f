"""
Integer sums never wrap -- over a SEQUENCE of requests (the GPU cases need an MI355X: -m gpu).

A hashed session's table sums are 64 bits wide and updated by unchecked atomics; what keeps them
from wrapping is a running bound in the table head (gpupreagg_hash_head::sum_bound[2], strom_gpupreagg.h):
every fold adds rows x 2^(bits of the largest input magnitude), and while the bound stays below 2^63
nothing is checked.  The bound has two slots and a parity.  tests/test_sum_overflow_gpu.py is thorough
per chunk, but its chunks are so heavy that the bound fails at once and everything goes through the
exact fold, which measures the bound anew.  Here the chunks are sized so that the PROVEN path runs
right up to the edge, and requests that fold nothing -- an empty row map, a chunk with a row-level
CpuReCheck, a reset() -- sit between them: the bound must neither lose a chunk (a later fold would
wrap a group's sum and answer Success) nor gain one (a later chunk would be sent back for nothing).

The contract, per request: the status (0 folded, 2 = StromError_CpuReCheck: not folded) and the
table, read with fetch() and compared with Python's big integers.  Which tier reached the verdict
(checked_folds()) is not asserted.

The arithmetic the expected statuses rest on is restated with Python ints in the CPU tests of this
module (no GPU needed), so the cases check their own premise.
"""
import numpy as np
import pytest

import oracle_binding as oracle
from pg_strom_amd import kds, runtime
from pg_strom_amd.gpupreagg import GpuPreAgg
from test_sum_overflow_gpu import I64_MAX, I64_MIN, totals

gpu = pytest.mark.gpu

# HSPEC of test_sum_overflow_gpu.py with one more target: int4pl overflows for var3 = 2^31 - 1, a
# row-level CpuReCheck that has nothing to do with the int8 sum
SPEC = ("(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8))"
        " (psum (int8 (int4pl (var 3 int4) (const int4 1)))))")
NTARGETS = 4
EDGE = 1 << 63
NO_ROWS = np.zeros(0, dtype=np.int32)


class Chunk(object):
    """the rows of one request: key, int8 input, int4 input; the COLUMN image is built once"""
    def __init__(self, g, x, y):
        self.g = np.asarray(g, dtype=np.int32)
        self.x = np.asarray(x, dtype=np.int64)
        self.y = np.asarray(y, dtype=np.int32)
        self._buf = None

    @property
    def buf(self):
        if self._buf is None:
            self._buf = kds.build_kds("column", [kds.Column("int4", self.g), kds.Column("int8", self.x),
                                                 kds.Column("int4", self.y)])
        return self._buf

    def __len__(self):
        return len(self.g)

    def group_sums(self):
        """{key: [rows, sum(var2), sum(var3 + 1)]} in Python ints"""
        out = {}
        for k, v, w in zip(self.g.tolist(), self.x.tolist(), self.y.tolist()):
            a = out.setdefault(k, [0, 0, 0])
            a[0] += 1
            a[1] += v
            a[2] += w + 1
        return out

    def magbits(self):
        """bits of the largest magnitude among the int8 sum's inputs (strom_gpupreagg.h:
        gpupreagg_sum_magnitude -- v >= 0: v, v < 0: -v - 1)"""
        return max((v if v >= 0 else -v - 1).bit_length() for v in self.x.tolist())

    def bound(self, least_bits=0):
        """what a fold of this chunk adds to the table's bound: rows x 2^bits.  least_bits: the
        second sum's inputs are int4 values and may count with the bits of their TYPE"""
        return len(self) << max(self.magbits(), least_bits)


def model_add(model, chunk):
    for k, a in chunk.group_sums().items():
        m = model.setdefault(k, [0, 0, 0])
        for i in range(3):
            m[i] += a[i]


def model_crosses(model, chunk):
    """would some group's int8 sum leave int8 if the chunk joined the table?"""
    for k, a in chunk.group_sums().items():
        s = model.get(k, [0, 0, 0])[1] + a[1]
        if s > I64_MAX or s < I64_MIN:
            return True
    return False


def as_table(model):
    return {(k,): [None] + list(v) for k, v in model.items()}


def oracle_status(chunk, row_map=None):
    rc, _, _ = oracle.gpupreagg(SPEC, chunk.buf, NTARGETS, row_map=row_map)
    return rc


# ---------------------------------------------------------------------------------------------
# part 1: the chunks of the hand-made sequences
# ---------------------------------------------------------------------------------------------
def heavy_chunk(sign=1):
    """H: 3072 rows of +-(2^50 - 1) in group 7, 100 small rows over keys 100..149"""
    g = np.concatenate([np.full(3072, 7), 100 + np.arange(100) % 50])
    x = np.concatenate([np.full(3072, sign * ((1 << 50) - 1)), (np.arange(100) * 37) % 1000])
    y = np.arange(len(g)) % 10
    return Chunk(g, x, y)


def recheck_chunk():
    """R: 300 ordinary rows, one of them with var3 = 2^31 - 1 (int4pl overflows)"""
    n = 300
    g = np.where(np.arange(n) % 6 == 0, 7, 100 + np.arange(n) % 50)
    x = (np.arange(n) * 53) % 1000
    y = np.arange(n) % 10
    y[123] = (1 << 31) - 1
    return Chunk(g, x, y)


def small_chunk():
    return Chunk([7, 7, 7], [1, 1, 1], [0, 1, 2])


def growth_chunk(n=4000000):
    """G: n distinct keys (from 1000 up), values below 2^10 -- more new groups than the first
    table's fill limit takes (the same count as test_hashed_table_grows_with_the_group_count)"""
    i = np.arange(n)
    return Chunk(1000 + i, (i * 7) % 1000, i % 10)


H, HDOWN, R, S = heavy_chunk(), heavy_chunk(-1), recheck_chunk(), small_chunk()
B_H = H.bound()
S7 = H.group_sums()[7][1]


def test_premise_of_the_sequences():
    """the hand arithmetic the expected statuses rest on, in Python ints, and the oracle's
    verdict on every chunk alone (the oracle runs on the CPU)"""
    assert len(H) == 3172 and H.magbits() == 50 and B_H == 3172 << 50
    assert HDOWN.magbits() == 50 and HDOWN.bound() == B_H
    assert S7 == 3072 * ((1 << 50) - 1) == 3 * (1 << 60) - 3072
    # two H: the truthful bound stays below 2^63, and the sum fits
    assert 2 * B_H < EDGE and 2 * S7 <= I64_MAX
    # three H: the truthful bound reaches 2^63 -- and rightly so, the sum does not fit
    assert 3 * B_H >= EDGE and 3 * S7 == 9 * (1 << 60) - 9216 > I64_MAX
    # a bound that lost one H lets the third fold through unchecked: that sum wraps
    assert 3 * B_H - B_H < EDGE
    # ... and what takes group 7 back down fits on top of two H
    assert 2 * S7 + HDOWN.group_sums()[7][1] == S7
    # S on top of two H stays provable, even if the int4 sum counts with 32 bits of its type
    assert 2 * B_H + S.bound(32) < EDGE and 2 * S7 + 3 <= I64_MAX
    # the small rows of H and R never matter
    assert all(abs(v[1]) < 10**6 for k, v in H.group_sums().items() if k != 7)
    assert all(abs(v[1]) < 10**6 for v in R.group_sums().values())
    # table growth: two H and G stay provable, three H are over the edge with or without G
    G = growth_chunk(1000)           # (the bound is linear in the rows: scaled up below)
    assert G.magbits() <= 10 and 2 * B_H + (4000000 << 32) < EDGE
    assert set(G.g.tolist()).isdisjoint(H.g.tolist())
    # the oracle, chunk by chunk
    assert oracle_status(H) == 0 and oracle_status(HDOWN) == 0 and oracle_status(S) == 0
    assert oracle_status(R) == 2
    assert oracle_status(H, row_map=NO_ROWS) == 0


# sequence -> the statuses it must return.  E: H with an empty row map; '!': reset()
SEQUENCES = [
    ("HEHH", [0, 0, 0, 2]),
    ("HRHH", [0, 2, 0, 2]),
    ("HHEH", [0, 0, 0, 2]),           # the skip at the other parity
    ("HHRH", [0, 0, 2, 2]),
    ("EHHH", [0, 0, 0, 2]),           # the skip before anything is in the table
    ("RHHH", [2, 0, 0, 2]),
    ("HEHS", [0, 0, 0, 0]),           # a skipped fold must not send later chunks back either
    ("HEREHH", [0, 0, 2, 0, 0, 2]),   # several skips in a row
    ("HEH!HHH", [0, 0, 0, 0, 0, 2]),  # a reset restarts the bound, at either parity
    ("HH", [0, 0]),
    ("HHH", [0, 0, 2]),               # (no skip at all: the proof itself)
]
CHUNKS = {"H": (H, None), "E": (H, NO_ROWS), "R": (R, None), "S": (S, None)}


def model_statuses(seq):
    """the rule of the module docstring, applied by the Python model alone"""
    model, out = {}, []
    for c in seq:
        if c == "!":
            model = {}
            continue
        chunk, rmap = CHUNKS[c]
        if rmap is not None:
            out.append(0)
        elif c == "R" or model_crosses(model, chunk):
            out.append(2)
        else:
            out.append(0)
            model_add(model, chunk)
    return out


def test_premise_expected_statuses_are_the_models():
    for seq, statuses in SEQUENCES:
        assert model_statuses(seq) == statuses, seq


def fold_and_compare(agg, model, chunk, row_map, want, what):
    """one request: status, then the table against the model (updated only by a fold that
    happened)"""
    status, pfm = agg.fold(chunk.buf, row_map=row_map)
    assert status == want, "%s: status %d, expected %d" % (what, status, want)
    if status == 0 and row_map is None:
        model_add(model, chunk)
    got = totals([agg.fetch()], agg.targets)
    assert got == as_table(model), "%s: table differs from the model (group 7: %r, expected %r)" % (
        what, got.get((7,)), as_table(model).get((7,)))
    return pfm


def take_group_7_down(agg, model, what):
    """after a CpuReCheck: 'table as it was' checked by use -- the chunk that takes group 7 back
    down must be summed, exactly"""
    fold_and_compare(agg, model, HDOWN, None, 0, what + " + H negated")
    assert model[7][1] == S7


def run_sequence(seq, statuses, parts=False):
    agg = GpuPreAgg(SPEC).begin_hashed()
    model = {}
    try:
        it = iter(statuses)
        nreq = 0
        for pos, c in enumerate(seq):
            what = "%s[%d]=%s" % (seq, pos, c)
            if c == "!":
                agg.reset()
                model = {}
                assert agg.num_groups() == 0 and len(agg.fetch()) == 0
                continue
            chunk, rmap = CHUNKS[c]
            want = next(it)
            known = agg.num_groups()
            pfm = fold_and_compare(agg, model, chunk, rmap, want, what)
            nreq += 1
            if parts and known >= 1 and rmap is None:
                # gpupreagg_launch_hashed marks the partition plan: the fold was gpupreagg_hash_fold_parts
                assert pfm["num_kern_prep"] >= 1, what
            if want == 2 and c == "H":
                take_group_7_down(agg, model, what)
    finally:
        agg.end()


@gpu
@pytest.mark.parametrize("seq,statuses", SEQUENCES, ids=[s for s, _ in SEQUENCES])
def test_hashed_sequence(seq, statuses):
    run_sequence(seq, statuses)


@gpu
@pytest.mark.parametrize("seq,statuses", SEQUENCES[:4], ids=[s for s, _ in SEQUENCES[:4]])
def test_hashed_sequence_partition_plan(seq, statuses, monkeypatch):
    """the same through the partition plan's fold (gpupreagg_hash_fold_units): from the second
    request on, when the table's group count is known"""
    monkeypatch.setenv("STROM_GPUPREAGG_HASH_PARTS_MIN", "1")
    run_sequence(seq, statuses, parts=True)


@gpu
@pytest.mark.parametrize("seq", ["HEHH", "HHEH"])
def test_hashed_sequence_with_an_empty_device_row_map(seq):
    """Scan -> PreAgg without leaving HBM, and the scan's WHERE kept nothing: the row map is a
    DeviceRowMap of no rows"""
    from pg_strom_amd.gpuscan import GpuScan
    store = runtime.DeviceStore.upload(H.buf)
    scan = GpuScan("(int4lt (var 1 int4) (const int4 0))").begin()
    rowmap, res = scan.scan_to_rowmap(store)
    assert res.nitems == 0 and rowmap.nvalids == 0
    agg = GpuPreAgg(SPEC).begin_hashed()
    model = {}
    try:
        for pos, (c, want) in enumerate(zip(seq, [0, 0, 0, 2])):
            what = "%s[%d]=%s (device row map)" % (seq, pos, c)
            if c == "E":
                assert agg.fold(store, row_map=rowmap)[0] == 0, what
                assert totals([agg.fetch()], agg.targets) == as_table(model), what
            else:
                fold_and_compare(agg, model, H, None, want, what)
        take_group_7_down(agg, model, seq)
    finally:
        agg.end()
        scan.end()
        rowmap.release()
        store.release()


def table_arrays(pr):
    """fetch() of a table with millions of groups, as sorted numpy columns (one row per group)"""
    k = pr.column(0)[0].astype(np.int64)
    order = np.argsort(k, kind="stable")
    assert len(np.unique(k)) == len(k)
    return [k[order]] + [pr.column(t)[0][order].astype(np.int64) for t in (1, 2, 3)]


@gpu
def test_hashed_table_growth_in_the_middle_keeps_the_bound():
    """H, H, G, H: G brings more new groups than the table's fill limit takes -- rows are deferred,
    the table grows (hash_table_grow copies both slots of the bound) and they are folded again;
    the third H must still be sent back"""
    G = growth_chunk()
    n = len(G)
    assert G.magbits() <= 10 and 2 * B_H + G.bound(32) < EDGE and 3 * B_H >= EDGE
    agg = GpuPreAgg(SPEC).begin_hashed()
    model = {}
    try:
        fold_and_compare(agg, model, H, None, 0, "H")
        fold_and_compare(agg, model, H, None, 0, "HH")
        small = len(model)
        status, pfm = agg.fold(G.buf)
        assert status == 0
        # a second launch of the fold exists only for rows deferred at the fill limit, and the
        # host grows the table before every such launch (gpupreagg_launch_hashed, turn > 0)
        assert pfm["num_kern_exec"] >= 3, pfm
        assert agg.num_groups() == small + n

        def check_table(what):
            k, cnt, s2, s3 = table_arrays(agg.fetch())
            assert len(k) == small + n, what
            lo = k < 1000
            assert {(int(a),): [None, int(b), int(c), int(d)]
                    for a, b, c, d in zip(k[lo], cnt[lo], s2[lo], s3[lo])} == as_table(model), what
            assert np.array_equal(k[~lo], G.g.astype(np.int64)) and (cnt[~lo] == 1).all(), what
            assert np.array_equal(s2[~lo], G.x) and np.array_equal(s3[~lo], G.y.astype(np.int64) + 1), what

        check_table("HHG")
        assert agg.fold(H.buf)[0] == 2, "HHGH: the third H fits no more"
        check_table("HHGH")
        assert agg.fold(HDOWN.buf)[0] == 0
        model_add(model, HDOWN)
        assert model[7][1] == S7
        check_table("HHGH + H negated")
    finally:
        agg.end()


# ---------------------------------------------------------------------------------------------
# part 2: seeded sequences against a Python model, hashed and dense sessions
# ---------------------------------------------------------------------------------------------
NKEYS = 200                               # keys 0 .. 199: the dense session's domain
HEAVY_GROUPS = {7: 1, 11: -1}             # a group's heavy values share a sign (see the docstring
                                          # of test_sum_overflow_gpu.py)
# (chosen by running the generator and the model alone: each has a request that folds nothing directly
# before an edge-crossing, four at either parity -- test_premise_of_the_seeded_sequences keeps it so)
SEEDS = [14, 25, 41, 74, 95, 113, 128, 167]
KINDS = ["ordinary", "heavy", "empty", "recheck", "reset"]
KIND_P = [0.20, 0.40, 0.15, 0.15, 0.10]


def ordinary_rows(rng, n):
    return (rng.integers(0, NKEYS, n), rng.integers(-10**9, 10**9 + 1, n), rng.integers(0, 10, n))


def generate(seed):
    """10 to 14 requests: [(kind, Chunk or None, row map or None)]"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for _ in range(int(rng.integers(10, 15))):
        kind = KINDS[int(rng.choice(len(KINDS), p=KIND_P))]
        if kind == "reset":
            out.append((kind, None, None))
            continue
        if kind == "heavy":
            # a few thousand rows of one magnitude in one group; the chunk's sum is 2^63 / m,
            # 2 <= m < 5: two to five such chunks reach the edge
            key = int(rng.choice(list(HEAVY_GROUPS)))
            rows = int(rng.integers(1000, 3001))
            value = int(EDGE / float(rng.uniform(2.0, 5.0))) // rows
            g, x, y = ordinary_rows(rng, 200)
            keep = ~np.isin(g, list(HEAVY_GROUPS))
            g, x, y = g[keep], x[keep], y[keep]
            g = np.concatenate([np.full(rows, key), g])
            x = np.concatenate([np.full(rows, HEAVY_GROUPS[key] * value), x])
            y = np.concatenate([np.arange(rows) % 10, y])
            out.append((kind, Chunk(g, x, y), None))
            continue
        n = 300 if kind == "recheck" else int(rng.integers(1, 4001))
        g, x, y = ordinary_rows(rng, n)
        if kind == "recheck":
            y[int(rng.integers(0, n))] = (1 << 31) - 1
        out.append((kind, Chunk(g, x, y), NO_ROWS if kind == "empty" else None))
    return out


def walk(requests, hashed, chunk_status=None):
    """the model: per request the status it must return and the table afterwards.
    chunk_status(chunk, row_map): the oracle's verdict on the chunk alone (default: what the
    generator meant -- 2 for a recheck chunk, else 0)"""
    model, steps = {}, []
    for kind, chunk, rmap in requests:
        if kind == "reset":
            model = {}
            steps.append((None, {}, False))
            continue
        alone = (chunk_status(chunk, rmap) if chunk_status else (2 if kind == "recheck" else 0))
        crossing = (hashed and alone == 0 and rmap is None and model_crosses(model, chunk))
        status = 2 if (alone == 2 or crossing) else 0
        if status == 0 and rmap is None:
            model_add(model, chunk)
        steps.append((status, {k: list(v) for k, v in model.items()}, crossing))
    return steps


def skips_before_a_crossing(requests):
    """positions (counted in requests, resets left out) of a request that folds nothing -- an empty
    row map, a recheck chunk -- directly followed by a heavy chunk that takes a sum over the edge"""
    steps = walk(requests, hashed=True)
    out, nreq = [], 0
    for i, (kind, _, _) in enumerate(requests):
        if kind == "reset":
            continue
        if (kind in ("empty", "recheck") and i + 1 < len(requests) and
                requests[i + 1][0] == "heavy" and steps[i + 1][2]):
            out.append(nreq)
        nreq += 1
    return out


def test_premise_of_the_seeded_sequences():
    """the property is not vacuous: every seed has a skipped request directly followed by an
    edge-crossing, at both parities over the set; the oracle agrees with what the generator
    meant for every chunk alone; the dense model does run past int8"""
    assert len(SEEDS) >= 8
    parities = set()
    past_int8 = 0
    for seed in SEEDS:
        requests = generate(seed)
        assert 10 <= len(requests) <= 14
        at = skips_before_a_crossing(requests)
        assert at, "seed %d: no skipped request directly before an edge-crossing" % seed
        parities.update(p & 1 for p in at)
        for kind, chunk, rmap in requests:
            if kind == "reset":
                continue
            assert oracle_status(chunk, rmap) == (2 if kind == "recheck" else 0), (seed, kind)
            assert set(chunk.g.tolist()) <= set(range(NKEYS))
            if kind == "heavy":
                # the chunk alone is far from the edge: no reduction order can matter inside it
                assert all(abs(v[1]) <= EDGE // 2 + 4000 * 10**9 for v in chunk.group_sums().values())
        for _, table, _ in walk(requests, hashed=False):
            past_int8 += any(not I64_MIN <= v[1] <= I64_MAX for v in table.values())
        # every hashed table of the model is a legal one
        for _, table, _ in walk(requests, hashed=True):
            assert all(I64_MIN <= v[1] <= I64_MAX for v in table.values())
    assert parities == {0, 1}
    assert past_int8 > 0


def run_seeded(seed, hashed):
    requests = generate(seed)
    steps = walk(requests, hashed, chunk_status=oracle_status)
    assert steps == walk(requests, hashed)               # the oracle is the generator's intent
    agg = GpuPreAgg(SPEC)
    if hashed:
        agg.begin_hashed()
    else:
        agg.begin([(0, NKEYS)])
    try:
        for i, ((kind, chunk, rmap), (want, table, _)) in enumerate(zip(requests, steps)):
            what = "seed %d request %d (%s)" % (seed, i, kind)
            if kind == "reset":
                agg.reset()
            else:
                status = agg.fold(chunk.buf, row_map=rmap)[0]
                assert status == want, "%s: status %d, expected %d" % (what, status, want)
            pr = agg.fetch()
            got = totals([pr], agg.targets)
            assert got == as_table(table), "%s: table differs from the model" % what
            # every partial row is a legal int8 partial, whatever their sum
            v, isn = pr.column(2)
            assert not isn.any() and v.dtype == np.int64, what
    finally:
        agg.end()


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_sequence_hashed(seed):
    """status 2 exactly where the oracle says so for the chunk alone, or where the chunk would
    take a group's sum outside int8; the table is the model's after every request"""
    run_seeded(seed, hashed=True)


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_sequence_dense(seed):
    """the same sequences in a dense session: its table is 128 bits wide, so status 2 only where
    the oracle says so for the chunk alone, the model is exact at every step, and a total beyond
    int8 comes out as several legal int8 partial rows"""
    run_seeded(seed, hashed=False)
