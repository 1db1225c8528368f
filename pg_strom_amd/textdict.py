"""
GROUP BY text / character(n): the key dictionary in front of GpuPreAgg, host side.

The reference groups by varlena keys inside gpupreagg (gpupreagg_codegen_keycomp,
gpupreagg.c:1208-1242) and hands the key datums back through pg_fixup_tupslot_varlena.
Here a dictionary of its own (strom_textdict_*, devlib/strom_textdict.h) maps the text column
of a resident COLUMN chunk to dense int4 ids; GpuPreAgg groups the encoded chunk by
(key (var K int4)) and the ids are replaced by their keys after the fetch.  group_by_text() is
the executor loop a backend would write.

Several shards (row ranges of one table, one process per GPU) each have a dictionary of their own,
and their sessions can only be merged when they call the same key by the same id: unify() builds
the union dictionary every rank builds alike (strom_keyunion_*: new keys are numbered in the order
of the key images, not in the order lanes win a slot), recode() rewrites the id columns of the
encoded chunks through the id maps, and group_by_text_sharded() is that loop with shards of one
device standing in for ranks.
"""
import ctypes
import os

import numpy as np

from ._lib import lib
from . import runtime
from .gpupreagg import GpuPreAgg, KIND_KEY, domain_of
from .kds import KDS_HEAD_FIXED

STROM_TEXTOID = 25
STROM_BPCHARNOID = 0x10000 | 1042
KINDS = {"text": STROM_TEXTOID, "character": STROM_BPCHARNOID}


def program_source(block=None, hash_bits=None):
    """the fixed program as csrc/textdict.cpp names it: the two knobs are part of its text
    (default: STROM_TEXTDICT_BLOCK / STROM_TEXTDICT_HASH_BITS of the environment)"""
    s = ""
    for name, v in (("TEXTDICT_BLOCK", block), ("TEXTDICT_HASH_BITS", hash_bits)):
        if v is None:
            v = os.environ.get("STROM_" + name) or None
        if v is not None:
            s += "#define %s %d\n" % (name, int(v))
    return s + ('#include "strom_kds.h"\n#include "strom_common.h"\n#include "strom_textlib.h"\n'
                '#include "strom_textdict.h"\n')


class TextDictionary(object):
    """keys of one text / character(n) column -> dense ids, resident on the device"""

    def __init__(self, kind, nkeys_hint=0, dindex=0):
        runtime.init()
        self.kind = kind
        err = ctypes.c_int(0)
        self.handle = lib.strom_textdict_create(KINDS[kind], int(nkeys_hint), dindex, ctypes.byref(err))
        if not self.handle:
            raise runtime.StromError(err.value, "strom_textdict_create")

    @property
    def num_keys(self):
        return lib.strom_textdict_num_keys(self.handle)

    def encode(self, store, key_cols, carry_cols=(), dicts=None):
        """store: resident COLUMN chunk (runtime.DeviceStore); key_cols / carry_cols: 0-based
        column numbers; dicts: one dictionary per key column (default: this one for each).
        Returns the encoded chunk: id columns first, then the carried columns."""
        dicts = list(dicts) if dicts is not None else [self] * len(key_cols)
        assert len(dicts) == len(key_cols)
        handles = (ctypes.c_void_p * max(len(dicts), 1))(*[d.handle for d in dicts])
        keys = (ctypes.c_int32 * max(len(key_cols), 1))(*[int(c) for c in key_cols])
        carry = (ctypes.c_int32 * max(len(carry_cols), 1))(*[int(c) for c in carry_cols])
        err = ctypes.c_int(0)
        h = lib.strom_textdict_encode(handles, keys, len(key_cols), store.handle, carry, len(carry_cols),
                                      ctypes.byref(err))
        if not h:
            raise runtime.StromError(err.value, "strom_textdict_encode")
        return runtime.DeviceStore(h, store.nitems)

    def encode_table(self, join, col):
        """text / character(n) column 'col' (0-based) of the one relation of join's hash table (DIRECT
        index, unique keys) becomes a CODED column of the table: int4 ids under this dictionary, by
        slot (strom_textdict_encode_table).  Returns its 0-based column index (>= the relation's own
        columns): the fused folds serve it like any int4 column of the relation -- mapped as
        (depth, index + 1, "int4").  A second call returns the same index.  The dictionary must
        outlive the table, unreset."""
        rc = lib.strom_textdict_encode_table(self.handle, join.table, int(col))
        if rc < 0:
            raise runtime.StromError(-rc, "strom_textdict_encode_table")
        return rc

    def image(self):
        """the keys as they lie in the dictionary: (heap bytes, offsets[id] of each complete datum) --
        what another dictionary absorbs, on this rank or on another"""
        nbytes = ctypes.c_size_t(0)
        n = lib.strom_textdict_fetch(self.handle, None, 0, None, 0, ctypes.byref(nbytes))
        if n < 0:
            raise runtime.StromError(-n, "strom_textdict_fetch")
        heap = np.zeros(max(nbytes.value, 1), dtype=np.uint8)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        n = lib.strom_textdict_fetch(self.handle, heap.ctypes.data, len(heap), offs.ctypes.data, len(offs),
                                     ctypes.byref(nbytes))
        if n < 0:
            raise runtime.StromError(-n, "strom_textdict_fetch")
        return heap[:nbytes.value].tobytes(), offs[:n].copy()

    def absorb(self, image):
        """image: (heap bytes, offsets) as image() returns it.  Its keys enter this dictionary, new ones
        numbered in image order; returns the KeyMap: id in the image -> id here"""
        heap, offs = image
        heap = np.frombuffer(bytes(heap), dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        err = ctypes.c_int(0)
        h = lib.strom_keyunion_absorb(self.handle, heap.ctypes.data if len(heap) else None, len(heap),
                                      offs.ctypes.data if len(offs) else None, len(offs), ctypes.byref(err))
        if not h:
            raise runtime.StromError(err.value, "strom_keyunion_absorb")
        return KeyMap(h, self)

    def absorb_dict(self, other):
        """absorb(other.image()) without the way over the host: both dictionaries are on one device"""
        err = ctypes.c_int(0)
        h = lib.strom_keyunion_absorb_dict(self.handle, other.handle, ctypes.byref(err))
        if not h:
            raise runtime.StromError(err.value, "strom_keyunion_absorb_dict")
        return KeyMap(h, self)

    def union_kernel_ns(self):
        """device time of the last absorb's kernels and of the last recode through one of this dictionary's
        maps (runtime perfmon on)"""
        ns = (ctypes.c_uint64 * 6)()
        lib.strom_keyunion_kernel_ns(self.handle, ns)
        return dict(zip(("probe", "ranks", "settle", "emit", "rebuild", "recode"), [int(v) for v in ns]))

    def keys(self):
        """payload bytes of every key, by id (header stripped; character(n) without its padding)"""
        nbytes = ctypes.c_size_t(0)
        n = lib.strom_textdict_fetch(self.handle, None, 0, None, 0, ctypes.byref(nbytes))
        if n < 0:
            raise runtime.StromError(-n, "strom_textdict_fetch")
        heap = np.zeros(nbytes.value + 8, dtype=np.uint8)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        n = lib.strom_textdict_fetch(self.handle, heap.ctypes.data, len(heap), offs.ctypes.data, len(offs),
                                     ctypes.byref(nbytes))
        if n < 0:
            raise runtime.StromError(-n, "strom_textdict_fetch")
        out = []
        for at in offs[:n]:
            at = int(at)
            b0 = int(heap[at])
            if b0 & 1:
                key = heap[at + 1:at + ((b0 >> 1) & 0x7f)].tobytes()
            else:
                size = int(heap[at:at + 4].view("<u4")[0]) >> 2
                key = heap[at + 4:at + size].tobytes()
            # character(n): the blanks behind the value are padding, not part of the key
            out.append(key.rstrip(b" ") if self.kind == "character" else key)
        return out

    def kernel_ns(self):
        """device time of the last encode's kernels (runtime perfmon on): probe, settle, emit, rebuild"""
        ns = (ctypes.c_uint64 * 4)()
        lib.strom_textdict_kernel_ns(self.handle, ns)
        return dict(zip(("probe", "settle", "emit", "rebuild"), [int(v) for v in ns]))

    def program_key(self):
        """key of the device program the last encode ran (0: none yet)"""
        return lib.strom_textdict_program(self.handle)

    def reset(self):
        lib.strom_textdict_reset(self.handle)

    def release(self):
        if self.handle:
            lib.strom_textdict_release(self.handle)
            self.handle = None


class KeyMap(object):
    """device-resident id map of one absorb: id under the absorbed image -> id under 'dictionary'.
    Release it before the dictionary."""

    def __init__(self, handle, dictionary):
        self.handle = handle
        self.dictionary = dictionary

    def __len__(self):
        return lib.strom_keymap_size(self.handle)

    def ids(self):
        out = np.zeros(max(len(self), 1), dtype=np.int32)
        rc = lib.strom_keymap_fetch(self.handle, out.ctypes.data, len(out))
        if rc != 0:
            raise runtime.StromError(rc, "strom_keymap_fetch")
        return out[:len(self)]

    def release(self):
        if self.handle:
            lib.strom_keymap_release(self.handle)
            self.handle = None


def recode(enc, cols, maps):
    """the int4 id columns 'cols' (0-based) of the encoded chunk 'enc' through 'maps', in place"""
    assert len(cols) == len(maps)
    colidx = (ctypes.c_int32 * max(len(cols), 1))(*[int(c) for c in cols])
    handles = (ctypes.c_void_p * max(len(maps), 1))(*[m.handle for m in maps])
    rc = lib.strom_keyunion_recode(enc.handle, colidx, handles, len(cols))
    if rc != 0:
        raise runtime.StromError(rc, "strom_keyunion_recode")


def unify(dicts, dindex=0):
    """(G, maps): a fresh dictionary that has absorbed each of 'dicts' in order, and per dictionary the
    map of its ids to G's.  Ranks that absorb the same dictionaries' images in the same order
    (G.absorb(image) for the images of parallel.allgather_key_images) get the same G."""
    union = TextDictionary(dicts[0].kind, nkeys_hint=min(sum(d.num_keys for d in dicts), 1 << 28), dindex=dindex)
    maps = []
    try:
        for d in dicts:
            maps.append(union.absorb_dict(d))
    except Exception:
        for m in maps:
            m.release()
        union.release()
        raise
    return union, maps


def group_by_text_sharded(shards, text_keys, spec, carry_cols, hashed=False, int_keys=()):
    """GROUP BY over text / character(n) keys of a table that lies in shards, one session per shard:
    the multi-rank loop, with shards of ONE device standing in for ranks (real ranks exchange their
    key images with parallel.allgather_key_images and absorb them in rank order instead of calling
    unify(); the session merge is then strom_gpupreagg_allreduce / _reduce_scatter).

    shards     [[resident COLUMN chunks of shard r]]; the other arguments as group_by_text's
    Returns (PartialRows of the merged sessions, key columns) as group_by_text does.
    """
    key_cols = [c for c, _ in text_keys]
    own = [[TextDictionary(kind) for _, kind in text_keys] for _ in shards]
    unions, maps = [], []               # per text key: G, [KeyMap of shard r]
    encoded = [[] for _ in shards]
    sessions = []
    try:
        # 1. every shard under dictionaries of its own
        for r, chunks in enumerate(shards):
            for chunk in chunks:
                encoded[r].append(own[r][0].encode(chunk, key_cols, carry_cols, own[r]))
        # 2. one union dictionary per text key, the shards' keys in rank order
        for k in range(len(text_keys)):
            g, m = unify([own[r][k] for r in range(len(shards))])
            unions.append(g)
            maps.append(m)
        # 3. the id columns into the common numbering
        for r in range(len(shards)):
            for enc in encoded[r]:
                recode(enc, list(range(len(text_keys))), [maps[k][r] for k in range(len(text_keys))])
        # 4. one session per shard over the common domain
        domain = None
        if not hashed:
            domain = [(0, g.num_keys) for g in unions]
            if int_keys:
                ncols = len(key_cols) + len(carry_cols)
                domain += domain_of([_chunk_head(e, ncols) for es in encoded for e in es], list(int_keys))
        for r in range(len(shards)):
            agg = GpuPreAgg(spec)
            sessions.append(agg)
            if hashed:
                agg.begin_hashed()
            else:
                assert len(domain) == sum(1 for k, _ in agg.targets if k == KIND_KEY), \
                    "every key target needs a domain: text_keys + int_keys"
                agg.begin(domain)
            for enc in encoded[r]:
                status, _ = agg.fold(enc)
                if status != 0:
                    raise runtime.StromError(status, "GpuPreAgg fold")
        # 5. the merge the ranks would run as a collective
        if hashed:
            GpuPreAgg.exchange_local(sessions, gather_after=True)
        else:
            for other in sessions[1:]:
                sessions[0].merge_from(other)
        pr = sessions[0].fetch()
        return pr, ids_to_keys(pr, unions)
    finally:
        for agg in sessions:
            agg.end()
        for es in encoded:
            for e in es:
                e.release()
        for ms in maps:
            for m in ms:
                m.release()
        for d in unions + [d for ds in own for d in ds]:
            d.release()


def group_by_text(chunks, text_keys, spec, carry_cols, hashed=False, row_maps=None, dicts=None, int_keys=()):
    """GROUP BY over text / character(n) keys, the loop a backend would write.

    chunks     resident COLUMN chunks (runtime.DeviceStore) of one table
    text_keys  [(0-based column, "text" | "character")]: they become columns 1..n of the encoded
               chunk, int4 ids
    carry_cols 0-based fixed-width columns of the source: columns n+1.. of the encoded chunk
    spec       GpuPreAgg IR over the ENCODED chunk, its first len(text_keys) keys being
               (key (var i int4)) for i = 1..n
    int_keys   0-based columns of the ENCODED chunk that are further (integer) group keys, in target
               order: a dense session takes their domain from the chunks' zone maps
    row_maps   per chunk, None or a runtime.DeviceRowMap / row array of a scan over the SOURCE
               chunk: rows and their order are the same in the encoded chunk
    Returns (PartialRows, key columns): key columns[i] is a list with the key bytes of every
    partial row (None for the NULL group) for text key i.
    """
    own = dicts is None
    if own:
        dicts = [TextDictionary(kind) for _, kind in text_keys]
    key_cols = [c for c, _ in text_keys]
    row_maps = row_maps if row_maps is not None else [None] * len(chunks)
    agg = GpuPreAgg(spec)
    nkeys = sum(1 for k, _ in agg.targets if k == KIND_KEY)
    encoded = []
    try:
        if hashed:
            # no second pass: each chunk is folded as soon as it is encoded
            agg.begin_hashed()
            for chunk, rm in zip(chunks, row_maps):
                enc = dicts[0].encode(chunk, key_cols, carry_cols, dicts)
                encoded.append(enc)
                status, _ = agg.fold(enc, row_map=rm)
                if status != 0:
                    raise runtime.StromError(status, "GpuPreAgg fold")
        else:
            # a dense session's ids must be known before it begins: encode everything first
            for chunk in chunks:
                encoded.append(dicts[0].encode(chunk, key_cols, carry_cols, dicts))
            domain = [(0, d.num_keys) for d in dicts]
            if int_keys:
                # further keys are plain columns of the encoded chunk: their zone maps, read from
                # the column directory alone
                domain += domain_of([_chunk_head(e, len(key_cols) + len(carry_cols)) for e in encoded],
                                    list(int_keys))
            assert len(domain) == nkeys, "every key target needs a domain: text_keys + int_keys"
            agg.begin(domain)
            for enc, rm in zip(encoded, row_maps):
                status, _ = agg.fold(enc, row_map=rm)
                if status != 0:
                    raise runtime.StromError(status, "GpuPreAgg fold")
        pr = agg.fetch()
        return pr, ids_to_keys(pr, dicts)
    finally:
        agg.end()
        for e in encoded:
            e.release()
        if own:
            for d in dicts:
                d.release()


def group_by_dimension_text(chunks, join, text_col, kind, spec, columns, dictionary=None):
    """SELECT dim.t, agg(..) FROM fact JOIN dim GROUP BY dim.t, the loop a backend would write: the
    dimension's text column is encoded ONCE, at table time, and every chunk is one lookup fold.

    chunks     resident COLUMN chunks of the fact table
    join       a begun GpuHashJoin whose table is the dimension (one relation, DIRECT, unique keys)
    text_col   0-based text / character(n) column of the dimension; kind "text" | "character"
    spec       GpuPreAgg IR whose FIRST key is (key (var K int4)), K the virtual column of the ids
    columns    the mapping as submit_lookup takes it, with None in the place of that virtual column:
               it becomes (1, coded index + 1, "int4")
    Returns (PartialRows, [keys of the id column: bytes, None for the NULL group])."""
    own = dictionary is None
    d = TextDictionary(kind) if own else dictionary
    agg = GpuPreAgg(spec)
    try:
        coded = d.encode_table(join, text_col)
        columns = [(1, coded + 1, "int4") if c is None else c for c in columns]
        agg.begin([(0, max(d.num_keys, 1))])
        for chunk in chunks:
            status, _ = agg.collect(agg.submit_lookup(join, chunk, columns))
            if status != 0:
                raise runtime.StromError(status, "GpuPreAgg lookup fold")
        pr = agg.fetch()
        return pr, ids_to_keys(pr, [d])[0]
    finally:
        agg.end()
        if own:
            d.release()


def ids_to_keys(pr, dicts):
    """the id key columns 0..len(dicts)-1 of partial rows -> their keys (None: the NULL group)"""
    key_resnos = [i for i, (k, _) in enumerate(pr.targets) if k == KIND_KEY][:len(dicts)]
    out = []
    for resno, d in zip(key_resnos, dicts):
        keys = d.keys()
        ids, isnull = pr.column(resno)
        out.append([None if nul else keys[int(i)] for i, nul in zip(ids, isnull)])
    return out


def _chunk_head(store, ncols):
    """head, colmeta and column directory of a resident COLUMN chunk (no column data)"""
    n = ((KDS_HEAD_FIXED + 8 * ncols + 15) & ~15) + 32 * ncols
    out = np.zeros((n + 7) // 8, dtype=np.uint64).view(np.uint8)[:n]
    rc = lib.strom_dstore_download(store.handle, out.ctypes.data, n)
    if rc != 0:
        raise runtime.StromError(rc, "strom_dstore_download")
    return out
