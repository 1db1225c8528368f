"""
Multi-GPU merge of GpuPreAgg partial tables (one process per GPU,
torch.distributed; backend "nccl" is RCCL on ROCm, xGMI between the GPUs of
a node; "gloo" for the CPU rehearsal in tests/).

The reference has no collective anywhere: one
backend merges partial rows in PostgreSQL's Agg node.  Here every rank
folds its row range into a resident table with an identical dense layout
(strom_gpupreagg.h: section 0 = u32 flags per group, section 1+a = 8-byte
values of aggregate a), so the merge is an all-reduce on the table itself,
one collective per section:

    nrows               SUM on int64     exact, order independent
    psum(int8)          128 bits wide in the table {low word, high word}: never wraps
                        (strom_gpupreagg.h, "integer sums never wrap") and neither may the
                        merge -- three carry-free limbs (low 32 bits | next 32 bits | high
                        word), each a SUM on int64, recombined with carries afterwards
    psum(float8)        SUM on float64   tolerance: summation order
    pmin / pmax         MIN / MAX on int64 (float keys are order-preserving
                        u64; the sign bit is flipped so that signed MIN/MAX
                        orders them)
    flags               OR, done as a SUM over unpacked bits (NCCL has no BOR)

Entries a rank never touched hold 0; for MIN/MAX they are replaced by the
identity before the collective.  With ~1e4 groups a section is 80 KB: the
collectives are latency bound, which is why they are few and whole-section.
"""
import ctypes

import numpy as np

KIND_KEY, KIND_NROWS, KIND_PSUM, KIND_PMIN, KIND_PMAX = 1, 2, 3, 4, 5
FLOAT_OIDS = (700, 701)
SIGN = np.int64(-2**63)


def align(v, a):
    return (v + a - 1) // a * a


class TableLayout(object):
    """byte layout of the resident table for `ngroups` dense ids"""

    def __init__(self, targets, ngroups):
        self.targets = list(targets)
        self.ngroups = ngroups
        self.aggs = [(i, k, oid) for i, (k, oid) in enumerate(self.targets) if k != KIND_KEY]
        self.flags_bytes = align(4 * ngroups, 256)
        self.vals_bytes = align(8 * ngroups, 256)
        # integer sums have a second section: their high word (gpupreagg_table_offset)
        self.intsums = [a for a, (_, k, oid) in enumerate(self.aggs) if k == KIND_PSUM and oid not in FLOAT_OIDS]
        self.nbytes = self.flags_bytes + self.vals_bytes * (len(self.aggs) + len(self.intsums))

    def vals_offset(self, a):
        return self.flags_bytes + self.vals_bytes * a

    def hi_offset(self, a):
        return self.flags_bytes + self.vals_bytes * (len(self.aggs) + self.intsums.index(a))

    def int_sum(self, tbl, a, gid):
        """the 128-bit sum of aggregate a in group gid as a Python int (numpy table bytes)"""
        n = self.ngroups
        lo = int(tbl[self.vals_offset(a):self.vals_offset(a) + 8 * n].view(np.uint64)[gid])
        hi = int(tbl[self.hi_offset(a):self.hi_offset(a) + 8 * n].view(np.int64)[gid])
        return (hi << 64) + lo


class RcclComm(object):
    """an RCCL communicator owned by libstrom_hip.so (strom_rccl_comm_init_rank): what
    strom_gpupreagg_allreduce() / _census_allreduce() merge over.  The unique id is
    made by rank 0 and handed to the others through torch.distributed's store-backed
    object broadcast (any channel would do: it is 128 bytes); torch is only the
    rendezvous, the collectives themselves are issued by the C library."""

    def __init__(self, rank, world, dindex=0, group=None, uid=None):
        from ._lib import lib
        self.lib = lib
        self.rank, self.world = rank, world
        nbytes = lib.strom_rccl_unique_id_bytes()
        if uid is None:
            import torch.distributed as dist
            box = [None]
            if rank == 0:
                buf = ctypes.create_string_buffer(nbytes)
                rc = lib.strom_rccl_get_unique_id(buf, nbytes)
                if rc != 0:
                    raise RuntimeError("strom_rccl_get_unique_id: %d" % rc)
                box[0] = buf.raw
            if world > 1:
                dist.broadcast_object_list(box, src=0, group=group)
            uid = box[0]
        handle = ctypes.c_void_p()
        rc = lib.strom_rccl_comm_init_rank(ctypes.byref(handle), world, uid, len(uid), rank, dindex)
        if rc != 0:
            raise RuntimeError("strom_rccl_comm_init_rank: %d" % rc)
        self.handle = handle

    def destroy(self):
        if self.handle:
            self.lib.strom_rccl_comm_destroy(self.handle)
            self.handle = None


def allreduce_table(table, layout, group=None):
    """in-place all-reduce of a table held in a torch uint8 tensor -- the torch
    statement of strom_gpupreagg_allreduce() (csrc/parallel.cpp), kept for the gloo
    rehearsal on CPU (tests/test_parallel_cpu.py) and as the check the C path is
    compared with on the GPU"""
    import torch
    import torch.distributed as dist
    n = layout.ngroups
    flags = table[:4 * n].view(torch.int32)
    nbits = len(layout.aggs) + 1
    shifts = torch.arange(nbits, device=table.device, dtype=torch.int32)
    bits = ((flags[:, None] >> shifts[None, :]) & 1).to(torch.int32)
    for a, (_, kind, oid) in enumerate(layout.aggs):
        off = layout.vals_offset(a)
        vals = table[off:off + 8 * n]
        has = bits[:, a + 1] != 0
        if kind == KIND_NROWS:
            v = vals.view(torch.int64)
            dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
        elif kind == KIND_PSUM and oid not in FLOAT_OIDS:
            # {lo, hi} -> limbs that cannot wrap under SUM, and back (strom_merge.h)
            lo = vals.view(torch.int64)
            hoff = layout.hi_offset(a)
            hi = table[hoff:hoff + 8 * n].view(torch.int64)
            lo.mul_(has.to(torch.int64))
            hi.mul_(has.to(torch.int64))
            l0 = lo & 0xffffffff
            l1 = (lo >> 32) & 0xffffffff            # (arithmetic shift, then the low 32 bits: logical)
            for limb in (l0, l1, hi):
                dist.all_reduce(limb, op=dist.ReduceOp.SUM, group=group)
            t = l1 + (l0 >> 32)
            lo.copy_((l0 & 0xffffffff) | (t << 32))
            hi.add_(t >> 32)
        elif kind == KIND_PSUM:
            v = vals.view(torch.float64)
            v.copy_(torch.where(has, v, torch.zeros_like(v)))
            dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
        else:
            v = vals.view(torch.int64)
            isfloat = oid in FLOAT_OIDS
            is_min = (kind == KIND_PMIN)
            w = v ^ int(SIGN) if isfloat else v.clone()   # unsigned order -> signed order
            ident = torch.iinfo(torch.int64).max if is_min else torch.iinfo(torch.int64).min
            w = torch.where(has, w, torch.full_like(w, ident))
            dist.all_reduce(w, op=dist.ReduceOp.MIN if is_min else dist.ReduceOp.MAX, group=group)
            v.copy_(w ^ int(SIGN) if isfloat else w)
    dist.all_reduce(bits, op=dist.ReduceOp.SUM, group=group)
    merged = ((bits > 0).to(torch.int32) << shifts[None, :]).sum(dim=1).to(torch.int32)
    flags.copy_(merged)
    return table


# ---- numpy helpers (tests, CPU rehearsal, decoding on the host) ------------
def pack_rows(layout, domain, values, isnull):
    """partial rows (uint64 images [n, ntargets], bool isnull) -> table bytes.
    domain: [(min, range)] per key; float partials are float64 images."""
    tbl = np.zeros(layout.nbytes, dtype=np.uint8)
    flags = tbl[:4 * layout.ngroups].view(np.uint32)
    keys = [i for i, (k, _) in enumerate(layout.targets) if k == KIND_KEY]
    for r in range(len(values)):
        gid, stride = 0, 1
        for (mn, rng), t in zip(domain, keys):
            off = rng if isnull[r, t] else int(values[r, t].view(np.int64)) - mn
            gid += off * stride
            stride *= rng + 1
        flags[gid] |= 1
        for a, (t, kind, oid) in enumerate(layout.aggs):
            vals = tbl[layout.vals_offset(a):layout.vals_offset(a) + 8 * layout.ngroups].view(np.uint64)
            if kind == KIND_NROWS:
                vals[gid] += values[r, t]
                continue
            if isnull[r, t]:
                continue
            had = bool(flags[gid] & (2 << a))
            x = values[r, t]
            if kind == KIND_PSUM:
                if oid in FLOAT_OIDS:
                    cur = vals[gid:gid + 1].view(np.float64)
                    cur[0] = (cur[0] if had else 0.0) + x.view(np.float64)
                else:
                    total = (layout.int_sum(tbl, a, gid) if had else 0) + int(x.view(np.int64))
                    vals[gid] = np.uint64(total & 0xFFFFFFFFFFFFFFFF)
                    hoff = layout.hi_offset(a)
                    tbl[hoff:hoff + 8 * layout.ngroups].view(np.int64)[gid] = total >> 64
            else:
                if oid in FLOAT_OIDS:
                    x = f64_ordered(x.view(np.float64))
                    cmp_new, cmp_old = int(x), int(vals[gid])
                else:
                    cmp_new, cmp_old = int(x.view(np.int64)), int(vals[gid:gid + 1].view(np.int64)[0])
                if not had or (cmp_new < cmp_old if kind == KIND_PMIN else cmp_new > cmp_old):
                    vals[gid] = x
            flags[gid] |= np.uint32(2 << a)
    return tbl


def f64_ordered(d):
    bits = np.array([d], dtype=np.float64).view(np.uint64)[0]
    if np.isnan(d):
        bits = np.uint64(0x7ff8000000000000)
    if bits & np.uint64(1 << 63):
        return np.uint64(~bits & np.uint64(0xFFFFFFFFFFFFFFFF))
    return np.uint64(bits | np.uint64(1 << 63))


def f64_unordered(k):
    k = np.uint64(k)
    bits = (k & np.uint64(0x7FFFFFFFFFFFFFFF)) if (k & np.uint64(1 << 63)) else np.uint64(~k & np.uint64(0xFFFFFFFFFFFFFFFF))
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def unpack_rows(layout, domain, tbl):
    """table bytes -> (values uint64 [n, ntargets], isnull), one row per seen group"""
    flags = tbl[:4 * layout.ngroups].view(np.uint32)
    keys = [i for i, (k, _) in enumerate(layout.targets) if k == KIND_KEY]
    gids = np.nonzero(flags & 1)[0]
    nt = len(layout.targets)
    values = np.zeros((len(gids), nt), dtype=np.uint64)
    isnull = np.zeros((len(gids), nt), dtype=bool)
    for r, gid in enumerate(gids):
        rest = int(gid)
        for (mn, rng), t in zip(domain, keys):
            off = rest % (rng + 1)
            rest //= (rng + 1)
            if off == rng:
                isnull[r, t] = True
            else:
                values[r, t] = np.array([mn + off], dtype=np.int64).view(np.uint64)[0]
        for a, (t, kind, oid) in enumerate(layout.aggs):
            vals = tbl[layout.vals_offset(a):layout.vals_offset(a) + 8 * layout.ngroups].view(np.uint64)
            if kind == KIND_NROWS:
                values[r, t] = vals[gid]
            elif not (flags[gid] & (2 << a)):
                isnull[r, t] = True
            elif kind != KIND_PSUM and oid in FLOAT_OIDS:
                values[r, t] = np.array([f64_unordered(vals[gid])], dtype=np.float64).view(np.uint64)[0]
            elif kind == KIND_PSUM and oid not in FLOAT_OIDS:
                total = layout.int_sum(tbl, a, gid)
                if not -2**63 <= total < 2**63:
                    raise OverflowError("sum of group %d does not fit one partial row: use TableLayout.int_sum" % gid)
                values[r, t] = np.uint64(total & 0xFFFFFFFFFFFFFFFF)
            else:
                values[r, t] = vals[gid]
    return values, isnull


def allreduce_census(bitmap, group=None, device=None):
    """union of the ranks' census bitmaps (uint32 words, one bit per dense
    id): every rank then compacts to the SAME table slots, which is what makes
    allreduce_table() a plain element-wise collective (SURVEY.md section 8e:
    "agree on dense group slots").  NCCL/RCCL has no bitwise OR, so the bits
    travel unpacked as bytes under MAX; the map is small (<= 2^26 bits)."""
    import torch
    import torch.distributed as dist
    bits = np.unpackbits(np.ascontiguousarray(bitmap, dtype=np.uint32).view(np.uint8), bitorder="little")
    t = torch.from_numpy(bits.copy())
    if device is not None:
        t = t.to(device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    merged = np.packbits(t.cpu().numpy(), bitorder="little").view(np.uint32)
    return merged


# ---------------------------------------------------------------------------
# hashed GROUP BY sessions (strom_gpupreagg_create_hashed): no common table
# layout across ranks -- every rank's table has its own slots -- so the merge
# is what the reference's Agg node does with partial rows of several chunks:
# gather them and combine rows of equal keys (pg_strom--1.0.sql:247-401).
# ---------------------------------------------------------------------------
def merge_partial_rows(targets, parts):
    """parts: [(values uint64 [n, ntargets], isnull bool [n, ntargets])] with floats as
    float8 images (the oracle's / partial_rows_as_raw8's convention).  Returns the
    combined (values, isnull), one row per distinct key (NULL keys are one group)."""
    nt = len(targets)
    values = np.concatenate([np.asarray(v, dtype=np.uint64).reshape(-1, nt) for v, _ in parts])
    isnull = np.concatenate([np.asarray(n, dtype=bool).reshape(-1, nt) for _, n in parts])
    keys = [t for t, (kind, _) in enumerate(targets) if kind == KIND_KEY]
    if len(values) == 0:
        return values, isnull
    if keys:
        ident = np.stack([np.where(isnull[:, t], np.uint64(0), values[:, t]) for t in keys] +
                         [isnull[:, t].astype(np.uint64) for t in keys], axis=1)
        _, first, inv = np.unique(ident, axis=0, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
    else:
        first, inv = np.zeros(1, dtype=np.int64), np.zeros(len(values), dtype=np.int64)
    ng = len(first)
    out_v = np.zeros((ng, nt), dtype=np.uint64)
    out_n = np.ones((ng, nt), dtype=bool)
    for t, (kind, oid) in enumerate(targets):
        col, nul = values[:, t], isnull[:, t]
        if kind == KIND_KEY:
            out_v[:, t], out_n[:, t] = col[first], nul[first]
            continue
        isflt = oid in FLOAT_OIDS
        x = col.view(np.float64) if isflt else col.view(np.int64)
        ok = ~nul
        has = np.zeros(ng, dtype=bool)
        np.logical_or.at(has, inv[ok], True)
        if kind in (KIND_NROWS, KIND_PSUM):
            acc = np.zeros(ng, dtype=x.dtype)
            np.add.at(acc, inv[ok], x[ok])
            if kind == KIND_NROWS:
                has[:] = True
        elif kind == KIND_PMIN:
            # PostgreSQL orders NaN above every number (float8_cmp_internal): the minimum
            # of {NaN, 1.0} is 1.0, NaN only if nothing else is there -> fmin, seeded with NaN
            acc = np.full(ng, np.nan if isflt else np.iinfo(np.int64).max, dtype=x.dtype)
            (np.fmin if isflt else np.minimum).at(acc, inv[ok], x[ok])
        else:
            # ... and the maximum is NaN as soon as one input is: np.maximum propagates it
            acc = np.full(ng, -np.inf if isflt else np.iinfo(np.int64).min, dtype=x.dtype)
            np.maximum.at(acc, inv[ok], x[ok])
        out_v[:, t] = np.where(has, acc.view(np.uint64), np.uint64(0))
        out_n[:, t] = ~has
    return out_v, out_n


def owner_of_partial_rows(targets, values, isnull, world):
    """the rank a partial row's group belongs to: a function of the key alone (csrc/parallel.cpp:
    hashed_exchange; the device hashes the key images, this restatement their bytes -- any
    function every rank agrees on does)"""
    import zlib
    values = np.asarray(values, dtype=np.uint64)
    keys = [t for t, (kind, _) in enumerate(targets) if kind == KIND_KEY]
    ident = np.stack([np.where(isnull[:, t], np.uint64(0), values[:, t]) for t in keys] +
                     [isnull[:, t].astype(np.uint64) for t in keys], axis=1) if keys else np.zeros((len(values), 1), np.uint64)
    return np.array([zlib.crc32(row.tobytes()) % world for row in ident], dtype=np.int64)


def integer_sum_bound(targets, values, isnull):
    """largest |integer psum| of these partial rows, plus one (0: none) -- what the ranks exchange
    before they add their sums up (gpupreagg_hash_sum_refresh)"""
    most = 0
    for t, (kind, oid) in enumerate(targets):
        if kind == KIND_PSUM and oid not in FLOAT_OIDS:
            v = np.asarray(values, dtype=np.uint64)[:, t].view(np.int64)[~isnull[:, t]]
            if len(v):
                most = max(most, int(np.abs(v.astype(object)).max()))
    return most + 1 if most else 0


def reduce_scatter_partial_rows(targets, values, isnull, group=None):
    """hash-partitioned merge of the ranks' partial rows: every rank ends up with the merged rows
    of the groups it owns (strom_gpupreagg_reduce_scatter).  Raises StromError(CpuReCheck) on
    EVERY rank when the ranks' integer sums could leave int8 together."""
    import torch.distributed as dist
    from .runtime import StromError
    world, me = dist.get_world_size(group), dist.get_rank(group)
    values, isnull = np.ascontiguousarray(values, dtype=np.uint64), np.ascontiguousarray(isnull, dtype=bool)
    owner = owner_of_partial_rows(targets, values, isnull, world)
    outgoing = [(values[owner == r], isnull[owner == r]) for r in range(world)]
    everybody = [None] * world
    dist.all_gather_object(everybody, (integer_sum_bound(targets, values, isnull), outgoing), group=group)
    bounds = [b for b, _ in everybody]
    if sum(1 for b in bounds if b) > 1 and sum(bounds) >= 2**63:
        raise StromError(2, "hash-partitioned merge: integer sums may leave int8")
    return merge_partial_rows(targets, [parts[me] for _, parts in everybody])


def gather_partial_rows(targets, values, isnull, group=None):
    """all ranks' partial rows, combined by key on every rank (the payload is the
    groups, not the rows: an object all-gather is enough)"""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    parts = [None] * world
    dist.all_gather_object(parts, (np.ascontiguousarray(values), np.ascontiguousarray(isnull)), group=group)
    return merge_partial_rows(targets, parts)


# ---------------------------------------------------------------------------
# GROUP BY text: the ranks' key dictionaries number their keys independently.  Before the first
# fold every rank learns every rank's key image and absorbs them in rank order
# (textdict.TextDictionary.absorb): the union dictionaries then agree id for id, and the merges
# above apply to sessions over text ids as they do to any fixed-width key.
# ---------------------------------------------------------------------------
def allgather_key_images(image, group=None):
    """image: (heap bytes, offsets) of this rank's dictionary (TextDictionary.image()).  Returns
    every rank's image, in rank order, on every rank."""
    import torch.distributed as dist
    heap, offsets = image
    images = [None] * dist.get_world_size(group)
    dist.all_gather_object(images, (bytes(heap), np.ascontiguousarray(offsets, dtype=np.uint64)), group=group)
    return images
