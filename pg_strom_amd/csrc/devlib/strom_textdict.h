/*
 * strom_textdict.h -- a dictionary of text / character(n) group keys on the device
 *
 * Stands where the varlena case of gpupreagg_codegen_keycomp stands (gpupreagg.c:1208-1242: any
 * type with a comparison function may be a group key, bpchar and text included).  GpuPreAgg here
 * groups by fixed-width key images; this fixed-function program, run IN FRONT of it, maps a text /
 * character(n) column of a resident COLUMN chunk to dense int4 ids, which GpuPreAgg then groups by
 * on its dense path.  The keys come back by id after the fetch (strom_textdict_fetch).
 *
 * State of a dictionary, all in HBM (textdict.cpp owns it):
 *   slots[nslots]   open addressing, linear probing, nslots a power of two; one 64-bit word each:
 *                     0                                   empty
 *                     OCCUPIED | PENDING | tag | row      claimed by THIS launch for row 'row' of the chunk
 *                     OCCUPIED |           tag | id       key 'id', settled by an earlier launch
 *                   tag: 30 bits of the hash that do not take part in the home slot
 *   entries[id]     {hash, offset of the datum in the heap}
 *   heap            one complete varlena datum per key, header included (the first row seen);
 *                   every datum starts on a 4-byte boundary
 *
 * NO LANE EVER WAITS FOR ANOTHER LANE.  An insert with a payload usually needs a "claimed, not
 * yet readable" state that others spin on.  Not here: a PENDING word names a row of the source
 * chunk, whose bytes have been in memory since before the launch and are never written; a settled
 * word names bytes a finished launch wrote.  Whatever a lane finds in a slot, the bytes it has to
 * compare with are readable at once.  The only words lanes of one launch exchange are the slot
 * words themselves (relaxed agent-scope atomics: performed at the coherence point, nothing else
 * is published through them).  Every loop is bounded by the slot count: slots only ever go from
 * empty to occupied during a probe, so a lost compare-and-swap looks at the winner's word and
 * moves on.  A probe whose claims take the table past half full sets ctl->toofull at once, and a
 * walk of more than 16 steps looks at that word every 64 and leaves with NoSpace when it is set:
 * a table too small for its chunk costs a short launch, not rows x slots steps.  The word is not
 * the status: a row error of the same launch keeps its priority and reaches the host first.
 *
 * Four kernels, four launches, the launch boundaries are the only ordering:
 *   textdict_probe    one row per lane: find or claim the row's slot
 *   textdict_settle   one new key per lane: id, heap bytes, entry, PENDING -> settled
 *   textdict_emit     one row per lane: the slot's id into the int4 column of the encoded chunk
 *   textdict_rebuild  one key per lane: entries -> a cleared slot array (growth, and the way back
 *                     from a failed probe: the entries are what a probe never touches)
 */
#ifndef STROM_TEXTDICT_DEVICE_H
#define STROM_TEXTDICT_DEVICE_H

#include "strom_ctl.h"

#ifndef TEXTDICT_BLOCK
#define TEXTDICT_BLOCK		256
#endif
/* the hash is cut to this many bits before tag and home slot are taken from it: the tests build
 * with 4, so that different keys share tags and home slots for certain */
#ifndef TEXTDICT_HASH_BITS
#define TEXTDICT_HASH_BITS	64
#endif
static_assert(TEXTDICT_BLOCK >= 64 && TEXTDICT_BLOCK <= 1024 && TEXTDICT_BLOCK % 64 == 0, "TEXTDICT_BLOCK: whole waves");
static_assert(TEXTDICT_HASH_BITS >= 1 && TEXTDICT_HASH_BITS <= 64, "TEXTDICT_HASH_BITS");

#define TEXTDICT_OCCUPIED	(1UL << 63)
#define TEXTDICT_PENDING	(1UL << 62)
#define TEXTDICT_TAG_MASK	0x3fffffff00000000UL
#define TEXTDICT_NO_SLOT	(~0u)

typedef __attribute__((address_space(1))) cl_ulong *textdict_slot_p;

STROM_DEVICE cl_ulong
textdict_hash(cl_ulong datum, bool blank_padded)
{
	cl_ulong	h = strom_varlena_hash(datum, blank_padded);
#if TEXTDICT_HASH_BITS < 64
	h &= (1UL << TEXTDICT_HASH_BITS) - 1;
#endif
	return h;
}

/* hash bits 34..63 (the home slot takes the low ones; nslots <= 2^31) */
STROM_DEVICE cl_ulong
textdict_tag(cl_ulong h)
{
	return TEXTDICT_OCCUPIED | ((h >> 2) & TEXTDICT_TAG_MASK);
}

STROM_DEVICE const cl_uchar *
textdict_key_bytes(cl_ulong datum, bool blank_padded, cl_int *p_len)
{
	cl_int		len;
	const cl_uchar *p = strom_varlena_payload(datum, &len);

	if (blank_padded)
		while (len > 0 && p[len - 1] == ' ')
			len--;
	*p_len = len;
	return p;
}

STROM_DEVICE cl_ulong
textdict_load_slot(const cl_ulong *slots, cl_uint s)
{
	return __hip_atomic_load((textdict_slot_p)(slots + s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

STROM_DEVICE cl_uint
textdict_wave_sum(cl_uint v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1)
		v += __shfl_xor(v, off, STROM_WAVE);
	return v;
}

/*
 * the call's status, usual priority: a significant code sticks, the first one wins; CpuReCheck
 * gives way to it.  One lane per wave, at most two compare-and-swaps, no loop.
 */
STROM_DEVICE void
textdict_writeback_status(cl_int *status, cl_int own_errcode)
{
	strom_lanemask_t major = __ballot(StromErrorIsSignificant(own_errcode));
	strom_lanemask_t bad = (major != 0 ? major : __ballot(own_errcode != StromError_Success));

	if (bad != 0)
	{
		int		leader = __ffsll((long long)bad) - 1;

		if ((int)strom_lane_id() == leader)
		{
			cl_int	old = atomicCAS(status, StromError_Success, own_errcode);
			if (old == StromError_CpuReCheck && StromErrorIsSignificant(own_errcode))
				atomicCAS(status, StromError_CpuReCheck, own_errcode);
		}
	}
}

/*
 * the key datum of 'row', checked the way pg_text_from_column / pg_text_from_addr check it: the
 * offset lies inside the chunk, so does the datum by its own length, and its header is one the
 * device reads in place.  Returns the datum's address, 0 with *p_isnull for a NULL key, 0 with an
 * error raised otherwise.
 */
STROM_DEVICE cl_ulong
textdict_row_datum(cl_int *errcode, const kern_data_store *src, const cl_ulong *values,
				   const cl_uint *notnull, cl_uint row, bool *p_isnull, cl_uint *p_size)
{
	cl_ulong	off = values[row];
	cl_ulong	length = src->length;

	*p_isnull = (off == 0 || (notnull && ((notnull[row >> 5] >> (row & 31)) & 1) == 0));
	if (*p_isnull)
		return 0;
	*p_isnull = false;
	if (off >= length)
	{
		STROM_SET_ERROR(errcode, StromError_DataStoreCorruption);
		return 0;
	}
	const char *addr = (const char *)src + off;
	cl_uchar	b0 = ((const cl_uchar *)addr)[0];
	/* the rest of a 2-byte external tag or a 4-byte header lies inside the chunk as well */
	if (off + (b0 == 0x01 ? 2 : ((b0 & 0x01) ? 1 : 4)) > length)
	{
		STROM_SET_ERROR(errcode, StromError_DataStoreCorruption);
		return 0;
	}
	cl_uint		size = strom_varsize_any(addr);
	if (off + size > length || size < ((b0 & 0x01) ? 1u : 4u))
	{
		STROM_SET_ERROR(errcode, StromError_DataStoreCorruption);
		return 0;
	}
	/* 1-byte external tag, or a 4-byte header with the "compressed" bit */
	if (b0 == 0x01 || (b0 & 0x03) == 0x02)
	{
		STROM_SET_ERROR(errcode, StromError_CpuReCheck);
		return 0;
	}
	*p_size = size;
	return (cl_ulong)addr;
}

/* ---------------------------------------------------------------- *
 * probe: the hot kernel.  Steady state (every key known): hash, one slot, one entry, one compare.
 * ---------------------------------------------------------------- */
extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_probe(const kern_data_store *__restrict__ src, textdict_args a)
{
	cl_ulong   *slots = (cl_ulong *)a.slots;
	const textdict_entry *entries = (const textdict_entry *)a.entries;
	const char *heap = (const char *)a.heap;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	cl_uint	   *row_slot = (cl_uint *)a.row_slot;
	textdict_newkey *newkeys = (textdict_newkey *)a.newkeys;
	const kern_coldir *cd = KERN_DATA_STORE_COLDIR(src) + a.colidx;
	const cl_ulong *values = (const cl_ulong *)((const char *)src + cd->values_off);
	const cl_uint *notnull = (cd->nulls_off ? (const cl_uint *)((const char *)src + cd->nulls_off) : NULL);
	const cl_uint nrows = src->nitems;
	const cl_uint mask = a.nslots - 1;
	const bool	blank_padded = (a.blank_padded != 0);
	const bool	byval = (src->colmeta[a.colidx].attlen >= 0);	/* the chunk lies: never followed as an offset */
	cl_int		errcode = StromError_Success;

	/* blockDim is whole waves and 'base' is the block's: every lane of a wave takes every turn */
	for (cl_uint base = blockIdx.x * blockDim.x; base < nrows; base += gridDim.x * blockDim.x)
	{
		cl_uint		row = base + threadIdx.x;
		cl_uint		myslot = TEXTDICT_NO_SLOT;
		cl_uint		size = 0;
		bool		isnull = false;
		bool		won = false;
		cl_int		rowerr = StromError_Success;
		cl_ulong	datum = 0;

		if (row < nrows)
		{
			if (byval)
				rowerr = StromError_DataStoreCorruption;
			else
				datum = textdict_row_datum(&rowerr, src, values, notnull, row, &isnull, &size);
		}
		if (datum != 0)
		{
			cl_int		len;
			const cl_uchar *key = textdict_key_bytes(datum, blank_padded, &len);
			cl_ulong	h = textdict_hash(datum, blank_padded);
			cl_ulong	tag = textdict_tag(h);
			cl_uint		s = (cl_uint)h & mask;
			bool		placed = false;

			for (cl_uint step = 0; step < a.nslots; step++, s = (s + 1) & mask)
			{
				cl_ulong	w = textdict_load_slot(slots, s);

				/* a long walk asks whether the table is lost already (see the claims below): a look,
				 * not a wait -- whatever it sees, the lane goes on or leaves */
				if ((step & 63) == 16 &&
					__hip_atomic_load(&ctl->toofull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
					break;
				if (w == 0)
				{
					cl_ulong	mine = tag | TEXTDICT_PENDING | row;

					if (__hip_atomic_compare_exchange_strong((textdict_slot_p)(slots + s), &w, mine,
															 __ATOMIC_RELAXED, __ATOMIC_RELAXED,
															 __HIP_MEMORY_SCOPE_AGENT))
					{
						won = placed = true;
						break;
					}
					/* lost: 'w' is the winner's word, looked at like any occupied slot */
				}
				if ((w & (TEXTDICT_OCCUPIED | TEXTDICT_TAG_MASK)) != tag)
					continue;
				cl_ulong	other = 0;
				if (w & TEXTDICT_PENDING)
				{
					/* a row of this chunk, checked by the lane that claimed the slot */
					cl_uint		orow = (cl_uint)w;
					if (orow < nrows)
						other = (cl_ulong)((const char *)src + values[orow]);
				}
				else if ((cl_uint)w < a.nkeys)
					other = (cl_ulong)(heap + entries[(cl_uint)w].off);
				if (other == 0)
				{
					rowerr = StromError_SanityCheckViolation;	/* a word no launch writes */
					break;
				}
				cl_int		olen;
				const cl_uchar *okey = textdict_key_bytes(other, blank_padded, &olen);
				if (strom_bytes_equal(key, len, okey, olen))
				{
					placed = true;
					break;
				}
			}
			if (placed)
				myslot = s;
			else if (rowerr == StromError_Success)
				rowerr = StromError_DataStoreNoSpace;
		}
		if (row < nrows)
			row_slot[row] = myslot;
		/* the claims of a wave: one add for their count, one for their bytes */
		strom_lanemask_t winners = __ballot(won);
		if (winners != 0)
		{
			cl_uint		bytes = textdict_wave_sum(won ? (cl_uint)STROM_INTALIGN(size) : 0u);
			int			leader = __ffsll((long long)winners) - 1;
			cl_uint		k0 = 0;

			if ((int)strom_lane_id() == leader)
			{
				k0 = atomicAdd(&ctl->nnew, (cl_uint)__popcll(winners));
				atomicAdd((unsigned long long *)&ctl->heap_need, (unsigned long long)bytes);
			}
			k0 = __shfl(k0, leader, STROM_WAVE);
			/* past half full the table is too small for this chunk: say so NOW, so that the walks of
			 * a filling table end at their next look instead of after nslots steps each; the host
			 * grows the table and probes again, unless a row error ends the call first */
			if ((int)strom_lane_id() == leader &&
				2 * ((cl_ulong)a.nkeys + k0 + (cl_uint)__popcll(winners)) > (cl_ulong)a.nslots)
				__hip_atomic_store(&ctl->toofull, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (won)
			{
				cl_uint		k = k0 + strom_mbcnt(winners);
				if (k < nrows)		/* a row wins once at most */
				{
					newkeys[k].slot = myslot;
					newkeys[k].row = row;
				}
			}
		}
		strom_lanemask_t nulls = __ballot(row < nrows && isnull);
		if (nulls != 0 && strom_lane_id() == 0)
			atomicAdd(&ctl->nnull, (cl_uint)__popcll(nulls));
		STROM_SET_ERROR(&errcode, rowerr);
	}
	textdict_writeback_status(&ctl->status, errcode);
}

/* ---------------------------------------------------------------- *
 * settle: the keys a probe claimed become entries
 * ---------------------------------------------------------------- */
struct __attribute__((packed)) textdict_unaligned_u64 { cl_ulong v; };

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_settle(const kern_data_store *__restrict__ src, textdict_args a)
{
	cl_ulong   *slots = (cl_ulong *)a.slots;
	textdict_entry *entries = (textdict_entry *)a.entries;
	char	   *heap = (char *)a.heap;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	const textdict_newkey *newkeys = (const textdict_newkey *)a.newkeys;
	const kern_coldir *cd = KERN_DATA_STORE_COLDIR(src) + a.colidx;
	const cl_ulong *values = (const cl_ulong *)((const char *)src + cd->values_off);
	const cl_uint nrows = src->nitems;
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < a.nnew; base += gridDim.x * blockDim.x)
	{
		cl_uint		k = base + threadIdx.x;
		bool		valid = (k < a.nnew);
		cl_uint		slot = 0, row = 0, size = 0, asize = 0;
		const char *from = NULL;

		if (valid)
		{
			slot = newkeys[k].slot;
			row = newkeys[k].row;
			if (slot >= a.nslots || row >= nrows)
			{
				errcode = StromError_SanityCheckViolation;
				valid = false;
			}
		}
		if (valid)
		{
			from = (const char *)src + values[row];		/* checked by the probe that claimed the slot */
			size = strom_varsize_any(from);
			asize = (cl_uint)STROM_INTALIGN(size);
		}
		/* a wave's share of the heap with one add: inclusive prefix sum over the lanes */
		cl_uint		lane = strom_lane_id();
		cl_uint		upto = asize;
#pragma unroll
		for (int d = 1; d < STROM_WAVE; d <<= 1)
		{
			cl_uint o = __shfl_up(upto, d, STROM_WAVE);
			if (lane >= (cl_uint)d)
				upto += o;
		}
		cl_uint		total = __shfl(upto, STROM_WAVE - 1, STROM_WAVE);
		cl_ulong	wave_at = 0;
		if (lane == 0 && total != 0)
			wave_at = atomicAdd((unsigned long long *)&ctl->heap_cursor, (unsigned long long)total);
		wave_at = __shfl(wave_at, 0, STROM_WAVE);
		if (!valid)
			continue;
		cl_ulong	at = a.heap_usage + wave_at + (upto - asize);
		if (at + asize > a.heap_size)
		{
			errcode = StromError_SanityCheckViolation;		/* the host sized the heap by heap_need */
			continue;
		}
		char	   *to = heap + at;
		cl_uint		i = 0;
		for (; i + 8 <= size; i += 8)
			((__attribute__((address_space(1))) textdict_unaligned_u64 *)(to + i))->v = strom_load_u64((const cl_uchar *)from + i);
		for (; i < size; i++)
			to[i] = from[i];
		cl_uint		id = a.nkeys + k;
		cl_ulong	h = textdict_hash((cl_ulong)from, a.blank_padded != 0);
		entries[id].hash = h;
		entries[id].off = at;
		__hip_atomic_store((textdict_slot_p)(slots + slot), textdict_tag(h) | id,
						   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	textdict_writeback_status(&ctl->status, errcode);
}

/* ---------------------------------------------------------------- *
 * emit: ids and notnull bits of the encoded chunk's key column
 * ---------------------------------------------------------------- */
extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_emit(const kern_data_store *__restrict__ src, textdict_args a)
{
	const cl_ulong *slots = (const cl_ulong *)a.slots;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	const cl_uint *row_slot = (const cl_uint *)a.row_slot;
	cl_int	   *out = (cl_int *)a.out_values;
	cl_uint	   *out_notnull = (cl_uint *)a.out_notnull;
	const cl_uint nrows = src->nitems;
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < nrows; base += gridDim.x * blockDim.x)
	{
		cl_uint		row = base + threadIdx.x;
		bool		notnull = false;

		if (row < nrows)
		{
			cl_uint		s = row_slot[row];
			cl_int		id = 0;

			if (s != TEXTDICT_NO_SLOT)
			{
				cl_ulong	w = (s < a.nslots ? slots[s] : 0UL);
				if ((w & TEXTDICT_OCCUPIED) == 0 || (w & TEXTDICT_PENDING) != 0 || (cl_uint)w >= a.nkeys)
					errcode = StromError_SanityCheckViolation;
				else
				{
					id = (cl_int)(cl_uint)w;
					notnull = true;
				}
			}
			out[row] = id;
		}
		/* 64 rows of a wave are two bitmap words (row is wave-aligned: blockDim is whole waves) */
		strom_lanemask_t bits = __ballot(notnull);
		cl_uint		lane = strom_lane_id();
		if ((lane & 31) == 0 && row < nrows)
			out_notnull[row >> 5] = (cl_uint)(bits >> lane);
	}
	textdict_writeback_status(&ctl->status, errcode);
}

/* ---------------------------------------------------------------- *
 * rebuild: every key into a cleared slot array (the keys differ: nothing to compare)
 * ---------------------------------------------------------------- */
extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_rebuild(textdict_args a)
{
	cl_ulong   *slots = (cl_ulong *)a.slots;
	const textdict_entry *entries = (const textdict_entry *)a.entries;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	const cl_uint mask = a.nslots - 1;
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < a.nkeys; base += gridDim.x * blockDim.x)
	{
		cl_uint		id = base + threadIdx.x;

		if (id < a.nkeys)
		{
			cl_ulong	h = entries[id].hash;
			cl_ulong	mine = textdict_tag(h) | id;
			cl_uint		s = (cl_uint)h & mask;
			bool		placed = false;

			for (cl_uint step = 0; step < a.nslots && !placed; step++, s = (s + 1) & mask)
			{
				cl_ulong	w = textdict_load_slot(slots, s);
				if (w == 0)
					placed = __hip_atomic_compare_exchange_strong((textdict_slot_p)(slots + s), &w, mine,
																  __ATOMIC_RELAXED, __ATOMIC_RELAXED,
																  __HIP_MEMORY_SCOPE_AGENT);
			}
			if (!placed)
				errcode = StromError_DataStoreNoSpace;
		}
	}
	textdict_writeback_status(&ctl->status, errcode);
}

#endif	/* STROM_TEXTDICT_DEVICE_H */
