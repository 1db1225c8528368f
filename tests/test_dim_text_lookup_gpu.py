"""
GROUP BY a DIMENSION's text / character(n) column, as ids (needs an MI355X: -m gpu):
strom_textdict_encode_table walks the rows of a hash table by slot (strom_textdict.h: textdict_table_*) and
leaves an int4 id per slot with the table -- a coded column -- which every fused fold then serves like
any int4 column of the relation (hashjoin_patch_dimrec_kernel puts it into the slot records).

The parent of this change has no such call: every test here fails there on the missing symbol.

Models are Python dicts over bytes plus numpy; the words are text_cases.WORDS (and generated ones where
more distinct keys are needed), character(n) through text_cases.bpchar_key; dimensions and helpers
are test_star_lookup_gpu.py's.  Bars: ids, keys, counts and integer sums equal; float8 sums within rtol
1e-12 (a group sums at most ~1e4 values of [0, 1): worst case 1e4 * 2^-53 = 1.1e-12 only if every
rounding went one way, a random walk gives 1e2 * 2^-53).

The ids of a coded column are read back through a fold: GROUP BY (fact.k, id) over a fact chunk that
holds every key of the table's range and some outside it -- one partial row per present slot, the id
NULL where the text is; an absent slot (a hole in the key range) has no partner and gives no row.
"""
import numpy as np
import pytest

import text_cases
from pg_strom_amd import kds, runtime
from pg_strom_amd._lib import lib
from pg_strom_amd.gpuhashjoin import GpuHashJoin, build_multihash
from pg_strom_amd.gpupreagg import GpuPreAgg
from pg_strom_amd.textdict import TextDictionary, group_by_dimension_text, ids_to_keys
from test_star_lookup_gpu import BAD_REQUEST, CPU_RECHECK, Dim, open_joins

pytestmark = pytest.mark.gpu

CORRUPTION = 300                                # StromError_DataStoreCorruption
WORDS = text_cases.WORDS


def many_words(n):
    """n distinct words: text_cases.WORDS first, then generated ones (a 200-byte one among them: a
    4-byte header next to the 1-byte ones)"""
    out = list(WORDS[:n])
    i = 0
    while len(out) < n:
        out.append((b"key-%05d" % i) if i != 3 else b"k" * 200)
        i += 1
    assert len(set(out)) == n
    return out


def text_dim(seed, nd, words, kind="text", holes=1.3, key_lo=-40, null_ratio=0.1, pick=None):
    """a dimension (k int4, t text | character(12)): row i holds words[pick[i]]"""
    rng = np.random.default_rng(seed)
    d = Dim(rng, nd, key_lo=key_lo, holes=holes)
    d.pick = rng.integers(0, len(words), nd) if pick is None else np.asarray(pick)
    d.words = [words[i] for i in d.pick]
    stored = d.words if kind == "text" else [(w + b" " * 12)[:max(12, len(w))] for w in d.words]
    d.tnull = rng.random(nd) < null_ratio
    d.kind = kind
    d.add(kind, stored, d.tnull)
    return d


def key_of(d, i):
    """the group key of dimension row i as the dictionary sees it; None for NULL"""
    if d.tnull[i]:
        return None
    return text_cases.bpchar_key(d.words[i]) if d.kind == "character" else d.words[i]


def lookup_rows(spec, domain, submit, ext=()):
    agg = GpuPreAgg(spec)
    try:
        agg.begin(domain, ext_params=ext)
        got = submit(agg)
        st, pfm = agg.collect(got)
        checked = agg.checked_folds()
        pr = agg.fetch()
        defines = agg.mapping_defines()
    finally:
        agg.end()
    assert st == 0
    return pr, pfm, checked, defines


def coded_ids(join, d, dic, coded):
    """{dimension key: id, None for a NULL id} of every slot that has a row, read through a fold"""
    k = np.arange(d.key_lo - 3, d.key_lo + d.span + 3, dtype=np.int32)
    ds = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", k)]))
    try:
        pr, _, _, _ = lookup_rows("(gpupreagg (key (var 1 int4)) (key (var 2 int4)) (nrows))",
                                  [(int(k[0]), len(k)), (0, max(dic.num_keys, 1))],
                                  lambda agg: agg.submit_lookup(join, ds, [(0, 1, "int4"), (1, coded + 1, "int4")]))
    finally:
        ds.release()
    (kv, kn), (iv, inull), (cnt, _) = pr.column(0), pr.column(1), pr.column(2)
    assert not kn.any() and np.all(cnt == 1)
    return {int(a): (None if nul else int(b)) for a, b, nul in zip(kv, iv, inull)}


def check_coded(join, d, dic, coded):
    """ids[] / isnull[] against the model: every present slot, and no other, has a row; its id is NULL iff
    the text is, and names the row's key under the dictionary"""
    got = coded_ids(join, d, dic, coded)
    keys = dic.keys()
    assert len(set(keys)) == len(keys) == dic.num_keys
    assert set(got) == set(int(x) for x in d.key)             # holes and keys outside the range: no row
    for i, k in enumerate(d.key):
        want, ident = key_of(d, i), got[int(k)]
        assert (ident is None) == (want is None), (i, want, ident)
        if want is not None:
            assert 0 <= ident < len(keys) and keys[ident] == want, (i, want, ident)
    return got


def encoded(d, dic):
    """(join, coded index) of a fresh table of d under dic"""
    join = open_joins([d], [1])[0]
    try:
        return join, dic.encode_table(join, 1)
    except Exception:
        join.end()
        raise


# ---------------------------------------------------------------------------------------------
# encode alone
# ---------------------------------------------------------------------------------------------
KNOBS = {"default": {}, "grid1": {"STROM_TEXTDICT_MAX_GRID": "1"},
         "block64_grid1": {"STROM_TEXTDICT_BLOCK": "64", "STROM_TEXTDICT_MAX_GRID": "1"}}


@pytest.mark.parametrize("knobs", sorted(KNOBS))
@pytest.mark.parametrize("nslots", [1, 255, 256, 257])
def test_slot_counts_around_one_block_and_grid_strides(nslots, knobs, monkeypatch):
    """1 slot, a block less one, a block, a block and one; one work-group of 256 or of 64 lanes walks the
    table in strides.  No holes: the key range is the rows.  NULLs in present rows."""
    for k, v in KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    runtime.init()
    d = text_dim(100 + nslots, nslots, WORDS, holes=1.0)
    dic = TextDictionary("text", nkeys_hint=64)
    join, coded = encoded(d, dic)
    try:
        assert join.table_info(1)["nslots"] == nslots
        assert coded == 2                                       # behind the relation's own two columns
        check_coded(join, d, dic, coded)
        assert set(dic.keys()) == {key_of(d, i) for i in range(d.nd)} - {None}
    finally:
        join.end()
        dic.release()


def test_holes_in_the_key_range_and_nulls():
    runtime.init()
    d = text_dim(211, 230, WORDS, holes=1.3, null_ratio=0.2)
    assert d.span > d.nd and d.tnull.any()
    dic = TextDictionary("text", nkeys_hint=64)
    join, coded = encoded(d, dic)
    try:
        assert join.table_info(1)["nslots"] > d.nd
        check_coded(join, d, dic, coded)
    finally:
        join.end()
        dic.release()


@pytest.mark.parametrize("shape", ["same", "distinct", "distinct_hash_bits_4"])
def test_one_key_in_every_row_and_a_key_of_its_own_in_every_row(shape, monkeypatch):
    """every row the same key: one claim, every other lane finds it under a PENDING word.  Every row a
    key of its own, in a dictionary begun WITHOUT a hint: 16 slots, so the table grows through NoSpace
    and rebuild; with TEXTDICT_HASH_BITS=4 unequal keys share tags and home slots for certain.
    1-byte and 4-byte headers (a 200-byte word, 'x' * 127 ...) and bytes >= 0x80 are among the words."""
    if shape == "distinct_hash_bits_4":
        monkeypatch.setenv("STROM_TEXTDICT_HASH_BITS", "4")
    runtime.init()
    nd = 290
    words = many_words(nd)
    assert any(len(w) == 200 for w in words) and any(max(w, default=0) >= 0x80 for w in words)
    pick = np.full(nd, 20) if shape == "same" else np.random.default_rng(5).permutation(nd)
    d = text_dim(307, nd, words, holes=1.02, null_ratio=0.0, pick=pick)
    dic = TextDictionary("text")                                # no hint: 16 slots
    if shape != "same":
        # four of the words are in the dictionary already: a rebuild then has entries to put back, so the
        # recovery shows as device time of textdict_rebuild (an empty dictionary is rebuilt by a memset)
        src = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("text", words[40:44])]))
        dic.encode(src, [0]).release()
        src.release()
        assert dic.num_keys == 4
    join, coded = encoded(d, dic)
    try:
        if shape != "same":
            assert dic.kernel_ns()["rebuild"] > 0               # NoSpace -> grow -> rebuild was taken
        got = check_coded(join, d, dic, coded)
        assert dic.num_keys == (1 if shape == "same" else nd)
        assert len(set(got.values())) == dic.num_keys
    finally:
        join.end()
        dic.release()


def test_character_ignores_trailing_blanks_and_text_does_not():
    """'a' and 'a ' are one key of a character(n) column and two of a text column"""
    runtime.init()
    words = [b"a", b"a ", b"a  ", b"ab", b"", b" "]
    for kind, nkeys in (("text", 6), ("character", 3)):
        d = text_dim(401, 60, words, kind=kind, null_ratio=0.05, pick=np.arange(60) % 6)
        dic = TextDictionary(kind)
        join, coded = encoded(d, dic)
        try:
            check_coded(join, d, dic, coded)
            assert dic.num_keys == nkeys
        finally:
            join.end()
            dic.release()


def test_keys_of_a_fact_chunk_keep_their_ids_and_a_second_call_adds_nothing():
    """a dictionary that has encoded a fact chunk first: those ids stay, the table's new keys follow;
    the second encode_table returns the same index, adds no key and launches nothing"""
    runtime.init()
    first = [WORDS[i] for i in (20, 21, 22, 3)]
    src = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("text", first * 5)]))
    d = text_dim(503, 200, WORDS)
    dic = TextDictionary("text")
    join = None
    try:
        dic.encode(src, [0]).release()
        before = dic.keys()
        assert sorted(before) == sorted(first)
        join, coded = encoded(d, dic)
        after = dic.keys()
        assert after[:len(before)] == before
        check_coded(join, d, dic, coded)
        ns = dic.kernel_ns()
        assert ns["probe"] > 0 and ns["emit"] > 0
        assert dic.encode_table(join, 1) == coded
        assert dic.keys() == after and dic.kernel_ns() == ns
        # a fact chunk encoded AFTERWARDS extends the dictionary; the coded column stays valid
        more = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("text", [b"never seen", b"MAIL"])]))
        dic.encode(more, [0]).release()
        more.release()
        assert dic.num_keys == len(after) + 1
        check_coded(join, d, dic, coded)
    finally:
        if join:
            join.end()
        src.release()
        dic.release()


def test_two_tables_under_one_dictionary_agree_on_ids():
    """supplier.nation and customer.nation as one domain"""
    runtime.init()
    d1, d2 = text_dim(601, 120, WORDS[:20]), text_dim(607, 250, WORDS[10:], key_lo=1000)
    dic = TextDictionary("text")
    j1, c1 = encoded(d1, dic)
    j2, c2 = encoded(d2, dic)
    try:
        g1, g2 = check_coded(j1, d1, dic, c1), check_coded(j2, d2, dic, c2)
        id_of = {}
        for d, g in ((d1, g1), (d2, g2)):
            for i, k in enumerate(d.key):
                if key_of(d, i) is not None:
                    assert id_of.setdefault(key_of(d, i), g[int(k)]) == g[int(k)]
        assert len(id_of) == dic.num_keys
    finally:
        j1.end()
        j2.end()
        dic.release()


@pytest.mark.parametrize("bad", ["compressed", "external"])
def test_an_unreadable_datum_in_one_row_is_the_cpus_and_nothing_stays(bad):
    runtime.init()
    rng = np.random.default_rng(701)
    nd = 100
    datums = [kds.varlena_datum(WORDS[i]) for i in rng.integers(0, len(WORDS), nd)]
    datums[57] = (np.array([(20 << 2) | 2], dtype="<u4").tobytes() + b"\0" * 16 if bad == "compressed"
                  else bytes([0x01, 18]) + b"\0" * 16)
    d = Dim(rng, nd, holes=1.2)
    d.add("text_raw", datums)
    known = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("text", [b"MAIL", b"SHIP"])]))
    fact = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", d.key.astype(np.int32))]))
    dic = TextDictionary("text")
    join = open_joins([d], [1])[0]
    try:
        dic.encode(known, [0]).release()
        with pytest.raises(runtime.StromError) as ei:
            dic.encode_table(join, 1)
        assert ei.value.errcode == CPU_RECHECK
        assert dic.num_keys == 2 and dic.keys() == [b"MAIL", b"SHIP"]
        # the index the column would have had names no column
        agg = GpuPreAgg("(gpupreagg (key (var 1 int4)) (nrows))").begin([(0, 2)])
        try:
            with pytest.raises(runtime.StromError) as ei:
                agg.collect(agg.submit_lookup(join, fact, [(1, 3, "int4")]))
            assert ei.value.errcode == CORRUPTION
        finally:
            agg.end()
        # the dictionary still works
        dic.encode(known, [0]).release()
        assert dic.num_keys == 2
    finally:
        join.end()
        known.release()
        fact.release()
        dic.release()


def test_refusals_launch_nothing():
    """BadRequest before any launch: a table that is not DIRECT with unique keys, another dictionary for
    the same column, a column outside the relation, NULL handles; a by-value column is the kernel's to
    find (DataStoreCorruption); a fold after reset() or release() of the dictionary is refused"""
    runtime.init()
    d = text_dim(801, 150, WORDS)
    rng = np.random.default_rng(803)
    dup = Dim(rng, 100)
    dup.key[1] = dup.key[0]                                     # not unique
    dup.add("text", [WORDS[i % len(WORDS)] for i in range(100)])
    wide = Dim(rng, 50)
    wide.key = wide.key * 10**7                                 # a key range no DIRECT index takes
    wide.span = int(wide.key.max() - wide.key.min()) + 1
    wide.add("text", [WORDS[i % len(WORDS)] for i in range(50)])
    fact = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", d.key.astype(np.int32))]))
    dic, other = TextDictionary("text"), TextDictionary("text")
    join, coded = encoded(d, dic)
    joins = [join]
    try:
        ns, nkeys = dic.kernel_ns(), dic.num_keys
        assert ns["probe"] > 0
        for dim in (dup, wide):
            km_join = GpuHashJoin("(gpuhashjoin (rel (hashkey (var 1 int4) 1 int4)))").begin(
                build_multihash([(dim.chunk(), [1])]))
            joins.append(km_join)
            info = km_join.table_info(1)
            assert not (info["mode"] == "direct" and info["unique"])
            for dd in (dic, other):
                assert lib.strom_textdict_encode_table(dd.handle, km_join.table, 1) == -BAD_REQUEST
        assert lib.strom_textdict_encode_table(other.handle, join.table, 1) == -BAD_REQUEST      # coded under dic
        assert lib.strom_textdict_encode_table(dic.handle, join.table, 2) == -BAD_REQUEST        # outside the relation
        assert lib.strom_textdict_encode_table(dic.handle, join.table, -1) == -BAD_REQUEST
        assert lib.strom_textdict_encode_table(None, join.table, 1) == -BAD_REQUEST
        assert lib.strom_textdict_encode_table(dic.handle, None, 1) == -BAD_REQUEST
        assert dic.kernel_ns() == ns and dic.num_keys == nkeys
        assert other.kernel_ns() == {"probe": 0, "settle": 0, "emit": 0, "rebuild": 0} and other.num_keys == 0
        # the key column is by value: the kernel says so, nothing is attached, the dictionary is as before
        assert lib.strom_textdict_encode_table(dic.handle, join.table, 0) == -CORRUPTION
        assert dic.num_keys == nkeys
        columns = [(1, coded + 1, "int4")]
        spec = "(gpupreagg (key (var 1 int4)) (nrows))"
        pr, _, _, _ = lookup_rows(spec, [(0, nkeys)], lambda agg: agg.submit_lookup(join, fact, columns))
        assert int(pr.column(1)[0].sum()) == d.nd
        # reset: the ids name keys that are gone
        dic.reset()
        for submit in (lambda agg: agg.submit_lookup(join, fact, columns),
                       lambda agg: agg.submit_lookup_star([join], fact, columns),
                       lambda agg: agg.submit_lookup_snowflake([join], [0], fact, columns)):
            agg = GpuPreAgg(spec).begin([(0, nkeys)])
            try:
                with pytest.raises(runtime.StromError) as ei:
                    submit(agg)
                assert ei.value.errcode == BAD_REQUEST
            finally:
                agg.end()
        # ... and the column may be encoded again: the same index, ids of the new epoch
        assert dic.encode_table(join, 1) == coded
        check_coded(join, d, dic, coded)
        # release: the dictionary is gone while the table lives on; its ids have no epoch at all
        dic.release()
        for submit in (lambda agg: agg.submit_lookup(join, fact, columns),
                       lambda agg: agg.submit_lookup_typed([join], ["left"], fact, columns)):
            agg = GpuPreAgg(spec).begin([(0, nkeys)])
            try:
                with pytest.raises(runtime.StromError) as ei:
                    submit(agg)
                assert ei.value.errcode == BAD_REQUEST
            finally:
                agg.end()
        # ... and another dictionary may take the column over
        assert other.encode_table(join, 1) == coded
        check_coded(join, d, other, coded)
    finally:
        for j in joins:
            j.end()
        fact.release()
        dic.release()
        other.release()


# ---------------------------------------------------------------------------------------------
# folds
# ---------------------------------------------------------------------------------------------
AGG3 = "(nrows) (psum (int8 (var 2 int4))) (psum (var 3 float8))"


class Fact(object):
    """fact(k1, k2, a int4, b float8) against up to two dimensions"""

    def __init__(self, seed, n, dims, nulls=True, a_range=(0, 2**31)):
        rng = np.random.default_rng(seed)
        self.n = n
        self.keys = [d.fact_keys(rng, n, nulls) for d in dims]
        while len(self.keys) < 2:
            self.keys.append((rng.integers(0, 100, n).astype(np.int32), np.zeros(n, dtype=bool)))
        self.a = rng.integers(a_range[0], a_range[1], n, dtype=np.int64).astype(np.int32)
        self.b = rng.random(n)
        self.an = (rng.random(n) < 0.03) if nulls else np.zeros(n, dtype=bool)
        cols = [kds.Column("int4", k, kn if nulls else None) for k, kn in self.keys]
        cols += [kds.Column("int4", self.a, self.an if nulls else None), kds.Column("float8", self.b)]
        self.store = runtime.DeviceStore.upload(kds.build_kds("column", cols))
        self.partners = [d.partner(k, kn) for d, (k, kn) in zip(dims, self.keys)]


def model(fact, sel, keyfns):
    """{(key bytes | None, ...): [nrows, sum a, sum b]} over the fact rows 'sel'"""
    out = {}
    for r in sel:
        g = out.setdefault(tuple(f(r) for f in keyfns), [0, 0, 0.0])
        g[0] += 1
        g[1] += 0 if fact.an[r] else int(fact.a[r])            # psum skips a NULL input
        g[2] += float(fact.b[r])
    return out


def folded(pr, dicts, times=1):
    """the partial rows as the model's map; the first len(dicts) targets are the id keys"""
    keycols = ids_to_keys(pr, dicts)
    n = len(dicts)
    cnt, sa, sb = pr.column(n)[0], pr.column(n + 1)[0], pr.column(n + 2)[0]
    out = {}
    for i in range(len(pr)):
        key = tuple(kc[i] for kc in keycols)
        assert key not in out
        out[key] = [int(cnt[i]) // times, int(sa[i]) // times, float(sb[i]) / times]
    return out


def same_groups(got, want):
    assert set(got) == set(want)
    for k, (c, sa, sb) in want.items():
        assert got[k][0] == c and got[k][1] == sa, k
        assert np.isclose(got[k][2], sb, rtol=1e-12, atol=0), k


_ONE = {}


def one_dim():
    """computed once, shared, left unchanged: 25 keys (the nation of a customer)"""
    if not _ONE:
        _ONE["d"] = text_dim(901, 230, WORDS[:25], null_ratio=0.08)
    return _ONE["d"]


@pytest.mark.parametrize("generic", [False, True])
def test_lookup_groups_by_the_dimensions_text_in_both_mapping_forms(generic, monkeypatch):
    """SELECT d.t, count(*), sum(a), sum(b) FROM fact JOIN d GROUP BY d.t through group_by_dimension_text;
    the narrow form is reached: a 25-key column and its NULL bit are a 2-byte record"""
    if generic:
        monkeypatch.setenv("STROM_GPUPREAGG_LOOKUP_GENERIC", "1")
    runtime.init()
    d = one_dim()
    fact = Fact(911, 6007, [d])
    join = open_joins([d], [1])[0]
    dic = TextDictionary("text")
    try:
        spec = "(gpupreagg (qual (isnotnull (var 2 int4))) (key (var 1 int4)) " + AGG3 + ")"
        pr, keys = group_by_dimension_text([fact.store], join, 1, "text", spec,
                                           [None, (0, 3, "int4"), (0, 4, "float8")], dictionary=dic)
        assert dic.num_keys == 25
        p = fact.partners[0]
        sel = np.flatnonzero((p >= 0) & ~fact.an)
        assert 0 < len(sel) < fact.n
        same_groups(folded(pr, [dic]), model(fact, sel, [lambda r: key_of(d, p[r])]))
        assert None in keys                                     # NULL text is the NULL group
        if not generic:
            columns = [(1, dic.encode_table(join, 1) + 1, "int4"), (0, 3, "int4"), (0, 4, "float8")]
            _, _, _, defines = lookup_rows(spec, [(0, 25)], lambda agg: agg.submit_lookup(join, fact.store, columns))
            assert any("#define GPUPREAGG_LOOKUP_NARROW 1" in t and "#define GPUPREAGG_LOOKUP_RECLEN 2" in t
                       for t in defines), defines
    finally:
        join.end()
        fact.store.release()
        dic.release()


def test_the_coded_column_in_the_qual():
    """WHERE d.t = 'MAIL' as an id equality, the id looked up in keys(); GROUP BY a fact column"""
    runtime.init()
    d = one_dim()
    fact = Fact(921, 5003, [d])
    join = open_joins([d], [1])[0]
    dic = TextDictionary("text")
    try:
        coded = dic.encode_table(join, 1)
        mail = dic.keys().index(b"MAIL")
        spec = ("(gpupreagg (qual (int4eq (var 4 int4) (const int4 %d))) (key (var 1 int4)) " % mail) + AGG3 + ")"
        columns = [(0, 2, "int4"), (0, 3, "int4"), (0, 4, "float8"), (1, coded + 1, "int4")]
        pr, _, _, _ = lookup_rows(spec, [(0, 100)], lambda agg: agg.submit_lookup(join, fact.store, columns))
        p = fact.partners[0]
        is_mail = np.array([key_of(d, i) == b"MAIL" for i in range(d.nd)])
        sel = np.flatnonzero((p >= 0) & is_mail[np.clip(p, 0, d.nd - 1)])
        assert 0 < len(sel)
        want = model(fact, sel, [lambda r: int(fact.keys[1][0][r])])
        got = {}
        for i in range(len(pr)):
            got[(int(pr.column(0)[0][i]),)] = [int(pr.column(1)[0][i]), int(pr.column(2)[0][i]), float(pr.column(3)[0][i])]
        same_groups(got, want)
    finally:
        join.end()
        fact.store.release()
        dic.release()


@pytest.mark.parametrize("packed", [False, True])
def test_star_of_two_dimensions_with_a_coded_column_each(packed):
    """GROUP BY d1.t, d2.t; dense accumulators, and packed ones (1e4 groups, summed outer columns without
    NULLs; num_kern_prep reports the packed path)"""
    runtime.init()
    n1, n2 = (100, 100) if packed else (12, 9)      # 1e4 groups: the packed image of two words a group fits one role
    # (every word occurs: the domain is n1 x n2 groups)
    d1 = text_dim(1001, 280, many_words(n1), null_ratio=0.0 if packed else 0.05, pick=np.arange(280) % n1)
    d2 = text_dim(1003, 260, many_words(n2)[::-1], key_lo=500, null_ratio=0.0 if packed else 0.05,
                  pick=np.arange(260) % n2)
    fact = Fact(1009, 40009 if packed else 7001, [d1, d2], nulls=not packed, a_range=(-5 * 10**5, 2**20))
    joins = open_joins([d1, d2], [1, 2])
    dic1, dic2 = TextDictionary("text"), TextDictionary("text")
    try:
        c1, c2 = dic1.encode_table(joins[0], 1), dic2.encode_table(joins[1], 1)
        assert (dic1.num_keys, dic2.num_keys) == (n1, n2)
        spec = "(gpupreagg (key (var 1 int4)) (key (var 4 int4)) " + AGG3 + ")"
        columns = [(1, c1 + 1, "int4"), (0, 3, "int4"), (0, 4, "float8"), (2, c2 + 1, "int4")]
        agg = GpuPreAgg(spec)
        try:
            agg.begin([(0, n1), (0, n2)])
            pfms = [agg.collect(agg.submit_lookup_star(joins, fact.store, columns)) for _ in range(2)]
            pr = agg.fetch()
        finally:
            agg.end()
        assert all(st == 0 for st, _ in pfms)
        assert all(pfm["num_kern_prep"] == (1 if packed else 0) for _, pfm in pfms)
        p1, p2 = fact.partners
        sel = np.flatnonzero((p1 >= 0) & (p2 >= 0))
        want = model(fact, sel, [lambda r: key_of(d1, p1[r]), lambda r: key_of(d2, p2[r])])
        same_groups(folded(pr, [dic1, dic2], times=2), want)
    finally:
        for j in joins:
            j.end()
        fact.store.release()
        dic1.release()
        dic2.release()


def test_a_left_relation_sends_partnerless_rows_and_null_text_to_the_null_group():
    runtime.init()
    d = one_dim()
    fact = Fact(1101, 6011, [d], nulls=False)
    join = open_joins([d], [1])[0]
    dic = TextDictionary("text")
    try:
        coded = dic.encode_table(join, 1)
        columns = [(1, coded + 1, "int4"), (0, 3, "int4"), (0, 4, "float8")]
        pr, _, _, _ = lookup_rows("(gpupreagg (key (var 1 int4)) " + AGG3 + ")", [(0, dic.num_keys)],
                                  lambda agg: agg.submit_lookup_typed([join], ["left"], fact.store, columns))
        p = fact.partners[0]
        nulltext = (p >= 0) & d.tnull[np.clip(p, 0, d.nd - 1)]
        assert np.count_nonzero(p < 0) > 0 and np.count_nonzero(nulltext) > 0
        got = folded(pr, [dic])
        same_groups(got, model(fact, range(fact.n), [lambda r: key_of(d, p[r]) if p[r] >= 0 else None]))
        # both kinds of row are in the NULL group, and nothing else is
        assert got[(None,)][0] == np.count_nonzero(p < 0) + np.count_nonzero(nulltext)
    finally:
        join.end()
        fact.store.release()
        dic.release()


def test_snowflake_groups_by_a_childs_coded_column():
    """fact -> d1 -> d2 GROUP BY d2.t: the coded column of the child, composed into d1's slot records"""
    runtime.init()
    rng = np.random.default_rng(1201)
    d2 = text_dim(1203, 90, WORDS[:25], key_lo=300, null_ratio=0.1)
    d1 = Dim(rng, 250, key_lo=-20)
    link, linknull = d2.fact_keys(rng, d1.nd, False)[0], rng.random(d1.nd) < 0.04
    d1.add("int4", link, linknull)
    fact = Fact(1207, 7013, [d1])
    joins = open_joins([d1, d2], [1, 2])                      # d2's program names column 2 of its parent
    dic = TextDictionary("text")
    try:
        coded = dic.encode_table(joins[1], 1)
        columns = [(2, coded + 1, "int4"), (0, 3, "int4"), (0, 4, "float8")]
        spec = "(gpupreagg (qual (isnotnull (var 2 int4))) (key (var 1 int4)) " + AGG3 + ")"
        pr, _, _, _ = lookup_rows(spec, [(0, dic.num_keys)],
                                  lambda agg: agg.submit_lookup_snowflake(joins, [0, 1], fact.store, columns,
                                                                          [None, "int4"]))
        p1 = fact.partners[0]
        i1 = np.clip(p1, 0, d1.nd - 1)
        p2 = np.where(p1 >= 0, d2.partner(link[i1], linknull[i1]), -1)
        sel = np.flatnonzero((p2 >= 0) & ~fact.an)
        assert 0 < len(sel) < np.count_nonzero(p1 >= 0)
        same_groups(folded(pr, [dic]), model(fact, sel, [lambda r: key_of(d2, p2[r])]))
    finally:
        for j in joins:
            j.end()
        fact.store.release()
        dic.release()


def test_the_plan_of_the_parent_commit_gives_the_same_groups():
    """join, COLUMN projection carrying the text column, strom_textdict_encode of the projected chunk, plain
    fold -- against encode_table and one lookup fold: equal (key bytes -> aggregates) maps"""
    runtime.init()
    d = one_dim()
    fact = Fact(1301, 6029, [d])
    join = open_joins([d], [1])[0]
    dic, old = TextDictionary("text"), TextDictionary("text")
    joined = enc = None
    try:
        coded = dic.encode_table(join, 1)
        spec = "(gpupreagg (key (var 1 int4)) " + AGG3 + ")"
        pr_new, _, _, _ = lookup_rows(spec, [(0, dic.num_keys)], lambda agg: agg.submit_lookup(
            join, fact.store, [(1, coded + 1, "int4"), (0, 3, "int4"), (0, 4, "float8")]))
        joined, nitems = join.join_to_column(fact.store, [(1, 2, "text"), (0, 3, "int4"), (0, 4, "float8")])
        enc = old.encode(joined, [0], [1, 2])
        pr_old, _, _, _ = lookup_rows(spec, [(0, old.num_keys)], lambda agg: agg.submit(enc))
        assert nitems == np.count_nonzero(fact.partners[0] >= 0)
        same_groups(folded(pr_new, [dic]), folded(pr_old, [old]))
    finally:
        for s in (joined, enc):
            if s is not None:
                s.release()
        join.end()
        fact.store.release()
        dic.release()
        old.release()


def test_the_checked_retry_is_taken_over_a_coded_group_key():
    """int8 inputs near 2^56: the range proof does not cover their sums and the chunk is folded again by the
    GPUPREAGG_CHECKED program, grouped by the coded column"""
    runtime.init()
    d = one_dim()
    n = 6007
    rng = np.random.default_rng(1401)
    k, kn = d.fact_keys(rng, n, True)
    x = (rng.integers(2**55, 2**56, n) * np.where(np.arange(n) % 2 == 0, 1, -1)).astype(np.int64)
    store = runtime.DeviceStore.upload(kds.build_kds("column", [kds.Column("int4", k, kn), kds.Column("int8", x)]))
    join = open_joins([d], [1])[0]
    dic = TextDictionary("text")
    try:
        coded = dic.encode_table(join, 1)
        pr, _, checked, _ = lookup_rows("(gpupreagg (key (var 1 int4)) (nrows) (psum (var 2 int8)))",
                                        [(0, dic.num_keys)],
                                        lambda agg: agg.submit_lookup(join, store, [(1, coded + 1, "int4"), (0, 2, "int8")]))
        assert checked >= 1
        p = d.partner(k, kn)
        want = {}
        for r in np.flatnonzero(p >= 0):
            g = want.setdefault(key_of(d, p[r]), [0, 0])
            g[0] += 1
            g[1] += int(x[r])
        keys = ids_to_keys(pr, [dic])[0]
        got = {keys[i]: [int(pr.column(1)[0][i]), int(pr.column(2)[0][i])] for i in range(len(pr))}
        assert got == want
    finally:
        join.end()
        store.release()
        dic.release()
