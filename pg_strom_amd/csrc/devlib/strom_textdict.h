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
 *
 * textdict_table_* are the same three steps over the rows of a HASH TABLE, by slot: a dimension's text
 * column becomes int4 ids kept with the table (a coded column), which the fused folds serve like any
 * int4 column of the relation.
 *
 * The last part of the file (keyunion_*) lets a dictionary absorb the keys of other dictionaries
 * with ids that do not depend on timing, and rewrites encoded id columns through the id maps that
 * come of it: what sessions of several shards need before their tables can be merged.
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

/* ================================================================ *
 * a DIMENSION's text column as a coded column: the dictionary walks the rows of a hash table (one
 * relation, DIRECT index, unique keys: what hashjoin_build_dimrec_kernel walks) by SLOT and leaves
 * ids[slot] / isnull[slot], the form hashjoin_build_dimcol_kernel writes.  The fused folds then
 * serve the ids like any int4 column of the relation; no text datum enters a slot record.
 *
 *   textdict_table_offsets  one slot per lane: slot array -> kern_hashentry -> kern_get_datum_tuple,
 *                           the datum checked as textdict_row_datum checks a row's; its offset from
 *                           the table image into datum_off[slot], 0 for an absent slot or a NULL
 *   textdict_table_probe    the walk of textdict_probe written out a third time (see keyunion_probe
 *                           for why not one definition); a PENDING word names a SLOT INDEX of the
 *                           table, and "index -> address" is one load from datum_off[], as it is one
 *                           load from a chunk's values[].  The table image and datum_off[] are
 *                           complete before the launch and never written during it: whatever a lane
 *                           finds in a slot of the dictionary, the bytes to compare are readable at
 *                           once.  No lane waits for another.  Many slots carry the same key (1e6
 *                           customers, 25 nations): "found under a PENDING or settled word"
 *   textdict_table_settle   textdict_settle with the datum read through datum_off[]
 *   textdict_table_emit     ids[slot] (int4), isnull[slot] (one byte); id 0 with isnull 1 for an
 *                           absent slot and for a NULL datum alike
 * ================================================================ */
STROM_DEVICE cl_ulong
textdict_table_datum(const textdict_table_args &t, cl_uint slot)
{
	cl_ulong	off = ((const cl_ulong *)t.datum_off)[slot];

	return off != 0 ? t.kmhash + off : 0UL;
}

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_table_offsets(textdict_table_args t, textdict_args a)
{
	const kern_multihash *kmhash = (const kern_multihash *)t.kmhash;
	const hashjoin_index *hjidx = (const hashjoin_index *)t.hjidx;
	const kern_hashtable *kht = KERN_HASHTABLE(kmhash, 0);
	const hashjoin_index_rel *ir = &hjidx->rel[0];
	const cl_uint *slots = (const cl_uint *)((const char *)hjidx + ir->slots_off);
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	cl_ulong   *datum_off = (cl_ulong *)t.datum_off;
	const cl_uint nslots = t.tbl_nslots;
	const cl_ulong length = kht->length;
	const cl_ulong kht_at = (cl_ulong)((const char *)kht - (const char *)kmhash);
	/* not a varlena column (the table lies, or the caller does): never followed as a datum */
	const bool	badcol = (t.colidx < 0 || t.colidx >= (cl_int)kht->ncols || kht->colmeta[t.colidx].attlen != -1 ||
						  ir->nslots != nslots);
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < nslots; base += gridDim.x * blockDim.x)
	{
		cl_uint		slot = base + threadIdx.x;
		cl_ulong	at = 0;
		cl_int		rowerr = StromError_Success;
		cl_uint		off = (slot < nslots && !badcol ? slots[slot] : 0u);

		if (slot < nslots && badcol)
			rowerr = StromError_DataStoreCorruption;
		else if (off != 0)
		{
			/* the entry and its tuple inside the table, then the datum by its own length */
			const kern_hashentry *ent = (const kern_hashentry *)((const char *)kht + off);
			const char *addr = NULL;

			if ((cl_ulong)off + offsetof(kern_hashentry, htup) + HEAPTUPLE_HEADER_FIXED > length ||
				ent->t_len < HEAPTUPLE_HEADER_FIXED ||
				(cl_ulong)off + offsetof(kern_hashentry, htup) + ent->t_len > length)
				rowerr = StromError_DataStoreCorruption;
			else
				addr = kern_get_datum_tuple(kht->colmeta, &ent->htup, (cl_uint)t.colidx);
			if (addr != NULL)
			{
				cl_ulong	doff = (cl_ulong)(addr - (const char *)kht);
				cl_uchar	b0 = (doff < length ? ((const cl_uchar *)addr)[0] : 0);

				/* (the rest of a 2-byte external tag or a 4-byte header lies inside the table as well) */
				if (doff >= length || doff + (b0 == 0x01 ? 2 : ((b0 & 0x01) ? 1 : 4)) > length)
					rowerr = StromError_DataStoreCorruption;
				else
				{
					cl_uint		size = strom_varsize_any(addr);

					if (doff + size > length || size < ((b0 & 0x01) ? 1u : 4u))
						rowerr = StromError_DataStoreCorruption;
					else if (b0 == 0x01 || (b0 & 0x03) == 0x02)
						rowerr = StromError_CpuReCheck;		/* external, or compressed */
					else
						at = kht_at + doff;
				}
			}
		}
		if (slot < nslots)
			datum_off[slot] = at;
		STROM_SET_ERROR(&errcode, rowerr);
	}
	textdict_writeback_status(&ctl->status, errcode);
}

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_table_probe(textdict_table_args t, textdict_args a)
{
	cl_ulong   *slots = (cl_ulong *)a.slots;
	const textdict_entry *entries = (const textdict_entry *)a.entries;
	const char *heap = (const char *)a.heap;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	cl_uint	   *row_slot = (cl_uint *)a.row_slot;
	textdict_newkey *newkeys = (textdict_newkey *)a.newkeys;
	const cl_uint nrows = t.tbl_nslots;
	const cl_uint mask = a.nslots - 1;
	const bool	blank_padded = (a.blank_padded != 0);
	cl_int		errcode = StromError_Success;

	/* blockDim is whole waves and 'base' is the block's: every lane of a wave takes every turn */
	for (cl_uint base = blockIdx.x * blockDim.x; base < nrows; base += gridDim.x * blockDim.x)
	{
		cl_uint		row = base + threadIdx.x;			/* a slot of the TABLE */
		cl_uint		myslot = TEXTDICT_NO_SLOT;			/* a slot of the DICTIONARY */
		cl_uint		size = 0;
		bool		won = false;
		cl_int		rowerr = StromError_Success;
		cl_ulong	datum = (row < nrows ? textdict_table_datum(t, row) : 0UL);

		if (datum != 0)
		{
			cl_int		len;
			const cl_uchar *key = textdict_key_bytes(datum, blank_padded, &len);
			cl_ulong	h = textdict_hash(datum, blank_padded);
			cl_ulong	tag = textdict_tag(h);
			cl_uint		s = (cl_uint)h & mask;
			bool		placed = false;

			size = strom_varsize_any((const char *)datum);
			for (cl_uint step = 0; step < a.nslots; step++, s = (s + 1) & mask)
			{
				cl_ulong	w = textdict_load_slot(slots, s);

				/* a look, not a wait (see textdict_probe) */
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
					/* a slot of this table, checked by textdict_table_offsets before this launch */
					if ((cl_uint)w < nrows)
						other = textdict_table_datum(t, (cl_uint)w);
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
			/* past half full: say so NOW (see textdict_probe) */
			if ((int)strom_lane_id() == leader &&
				2 * ((cl_ulong)a.nkeys + k0 + (cl_uint)__popcll(winners)) > (cl_ulong)a.nslots)
				__hip_atomic_store(&ctl->toofull, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (won)
			{
				cl_uint		k = k0 + strom_mbcnt(winners);
				if (k < nrows)		/* a slot wins once at most */
				{
					newkeys[k].slot = myslot;
					newkeys[k].row = row;
				}
			}
		}
		STROM_SET_ERROR(&errcode, rowerr);
	}
	textdict_writeback_status(&ctl->status, errcode);
}

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_table_settle(textdict_table_args t, textdict_args a)
{
	cl_ulong   *slots = (cl_ulong *)a.slots;
	textdict_entry *entries = (textdict_entry *)a.entries;
	char	   *heap = (char *)a.heap;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	const textdict_newkey *newkeys = (const textdict_newkey *)a.newkeys;
	const cl_uint nrows = t.tbl_nslots;
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
			from = (const char *)textdict_table_datum(t, row);	/* checked by textdict_table_offsets */
			if (from == NULL)
			{
				errcode = StromError_SanityCheckViolation;		/* a slot without a datum claims nothing */
				valid = false;
			}
		}
		if (valid)
		{
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

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
textdict_table_emit(textdict_table_args t, textdict_args a)
{
	const cl_ulong *slots = (const cl_ulong *)a.slots;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	const cl_uint *row_slot = (const cl_uint *)a.row_slot;
	cl_int	   *out_ids = (cl_int *)t.out_ids;
	cl_uchar   *out_isnull = (cl_uchar *)t.out_isnull;
	const cl_uint nrows = t.tbl_nslots;
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < nrows; base += gridDim.x * blockDim.x)
	{
		cl_uint		row = base + threadIdx.x;

		if (row < nrows)
		{
			cl_uint		s = row_slot[row];
			cl_int		id = 0;
			bool		isnull = true;

			if (s != TEXTDICT_NO_SLOT)
			{
				cl_ulong	w = (s < a.nslots ? slots[s] : 0UL);
				if ((w & TEXTDICT_OCCUPIED) == 0 || (w & TEXTDICT_PENDING) != 0 || (cl_uint)w >= a.nkeys)
					errcode = StromError_SanityCheckViolation;
				else
				{
					id = (cl_int)(cl_uint)w;
					isnull = false;
				}
			}
			out_ids[row] = id;
			out_isnull[row] = (isnull ? 1 : 0);
		}
	}
	textdict_writeback_status(&ctl->status, errcode);
}

/* ================================================================ *
 * union of dictionaries: the keys of an IMAGE (heap bytes + offsets, what strom_textdict_fetch
 * hands out, or another dictionary's heap and entries) enter this dictionary, and every image
 * key learns its id here.  New keys are numbered in IMAGE ORDER -- key i of the image, if the
 * dictionary does not hold it and no j < i of the image equals it, becomes id K + (number of
 * such keys before i) -- so that dictionaries that absorb the same images in the same order are
 * identical, whatever the timing of their lanes.
 *
 *   keyunion_probe    one image key per lane: find or claim its slot.  The walk of textdict_probe
 *                     written out a second time (one templated definition for both cost
 *                     textdict_probe two VGPRs and this kernel four: DESIGN 3.8); a PENDING
 *                     word names an index of the image.  A lane that finds its key
 *                     under a PENDING word with a higher index lowers the word to its own index
 *                     (one 64-bit atomic min: tag and flag bits are equal, the index decides), so
 *                     after the launch a claimed slot names the LOWEST index of its key.  A lane
 *                     records its slot only; nothing depends on who claimed.
 *   keyunion_count    key i is new iff its slot holds PENDING | i; per tile of TEXTDICT_BLOCK
 *                     image keys: how many, and the heap bytes of their datums
 *   keyunion_offsets  one work-group: exclusive sums over the tiles, the totals behind the last
 *   keyunion_settle   the new key of rank r (tile offset + rank inside the tile): id K + r, heap
 *                     bytes, entry, PENDING -> tag | id, as textdict_settle does
 *   keyunion_emit     map[i] = the id in key i's slot
 *   keyunion_recode   ids[row] = map[ids[row]] over an id column of an encoded chunk, in place
 *
 * No lane waits for another here either: the ranks are three launches (count, offsets, settle),
 * not a look-back scan; inside a tile the sums go through LDS between two work-group barriers,
 * which every lane of the work-group reaches (tiles are handed out per work-group).
 * ================================================================ */

/* key i of the image, checked against the image the way textdict_row_datum checks a row against
 * its chunk; a header the device does not read in place has no business in a key image */
STROM_DEVICE cl_ulong
keyunion_image_offset(const keyunion_args &a, cl_uint i)
{
	return *(const cl_ulong *)((const char *)a.img_offsets + (size_t)i * a.img_stride);
}

STROM_DEVICE cl_ulong
keyunion_image_datum(cl_int *errcode, const keyunion_args &a, cl_uint i)
{
	cl_ulong	off = keyunion_image_offset(a, i);
	cl_ulong	length = a.img_heaplen;

	if (off >= length)
	{
		STROM_SET_ERROR(errcode, StromError_DataStoreCorruption);
		return 0;
	}
	const char *addr = (const char *)a.img_heap + off;
	cl_uchar	b0 = ((const cl_uchar *)addr)[0];
	if (b0 == 0x01 || (b0 & 0x03) == 0x02 || off + ((b0 & 0x01) ? 1 : 4) > length)
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
	return (cl_ulong)addr;
}

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
keyunion_probe(keyunion_args a)
{
	cl_ulong   *slots = (cl_ulong *)a.slots;
	const textdict_entry *entries = (const textdict_entry *)a.entries;
	const char *heap = (const char *)a.heap;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	cl_uint	   *key_slot = (cl_uint *)a.key_slot;
	const cl_uint nimg = a.nimg;
	const cl_uint mask = a.nslots - 1;
	const bool	blank_padded = (a.blank_padded != 0);
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < nimg; base += gridDim.x * blockDim.x)
	{
		cl_uint		i = base + threadIdx.x;
		cl_uint		myslot = TEXTDICT_NO_SLOT;
		bool		won = false;
		cl_int		rowerr = StromError_Success;
		cl_ulong	datum = (i < nimg ? keyunion_image_datum(&rowerr, a, i) : 0);

		if (datum != 0)
		{
			cl_int		len;
			const cl_uchar *key = textdict_key_bytes(datum, blank_padded, &len);
			cl_ulong	h = textdict_hash(datum, blank_padded);
			cl_ulong	tag = textdict_tag(h);
			cl_ulong	mine = tag | TEXTDICT_PENDING | i;
			cl_uint		s = (cl_uint)h & mask;
			bool		placed = false;

			for (cl_uint step = 0; step < a.nslots; step++, s = (s + 1) & mask)
			{
				cl_ulong	w = textdict_load_slot(slots, s);

				/* a look, not a wait (see textdict_probe) */
				if ((step & 63) == 16 &&
					__hip_atomic_load(&ctl->toofull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
					break;
				if (w == 0)
				{
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
					/* a key of this image, checked by the lane that claimed the slot (or lowered its word) */
					if ((cl_uint)w < nimg)
						other = (cl_ulong)((const char *)a.img_heap + keyunion_image_offset(a, (cl_uint)w));
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
					/* my key, claimed under a later index: the word differs from mine in the index
					 * alone, the smaller one stays whoever comes last */
					if ((w & TEXTDICT_PENDING) != 0 && (cl_uint)w > i)
						(void)__hip_atomic_fetch_min((textdict_slot_p)(slots + s), mine,
													 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					placed = true;
					break;
				}
			}
			if (placed)
				myslot = s;
			else if (rowerr == StromError_Success)
				rowerr = StromError_DataStoreNoSpace;
		}
		if (i < nimg)
			key_slot[i] = myslot;
		/* a claim is a new key, whichever index ends up in its word: count them for the host's
		 * growth decisions, and say at once when the table is lost (see textdict_probe) */
		strom_lanemask_t winners = __ballot(won);
		if (winners != 0)
		{
			int			leader = __ffsll((long long)winners) - 1;

			if ((int)strom_lane_id() == leader)
			{
				cl_uint		k0 = atomicAdd(&ctl->nnew, (cl_uint)__popcll(winners));
				if (2 * ((cl_ulong)a.nkeys + k0 + (cl_uint)__popcll(winners)) > (cl_ulong)a.nslots)
					__hip_atomic_store(&ctl->toofull, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
		}
		STROM_SET_ERROR(&errcode, rowerr);
	}
	textdict_writeback_status(&ctl->status, errcode);
}

/* is image key i new, and how much heap does its datum take?  (slots as the probe left them) */
STROM_DEVICE bool
keyunion_is_new(cl_int *errcode, const keyunion_args &a, cl_uint i, cl_uint *p_slot, cl_uint *p_size)
{
	cl_uint		s = ((const cl_uint *)a.key_slot)[i];

	if (s >= a.nslots)
	{
		*errcode = StromError_SanityCheckViolation;		/* a failed key ends the absorb before this launch */
		return false;
	}
	cl_ulong	w = textdict_load_slot((const cl_ulong *)a.slots, s);
	if ((w & TEXTDICT_PENDING) == 0 || (cl_uint)w != i)
		return false;
	*p_slot = s;
	*p_size = strom_varsize_any((const char *)a.img_heap + keyunion_image_offset(a, i));	/* checked by the probe */
	return true;
}

/*
 * exclusive sums of (count, bytes) over the lanes of a work-group in thread order, and the totals.
 * Every lane of the work-group calls it.
 */
STROM_DEVICE void
keyunion_block_sums(cl_uint count, cl_ulong bytes, cl_uint *p_count_before, cl_ulong *p_bytes_before,
					cl_uint *p_count_total, cl_ulong *p_bytes_total)
{
	__shared__ cl_uint	wave_count[TEXTDICT_BLOCK / STROM_WAVE];
	__shared__ cl_ulong	wave_bytes[TEXTDICT_BLOCK / STROM_WAVE];
	cl_uint		lane = strom_lane_id();
	cl_uint		wave = threadIdx.x / STROM_WAVE;
	cl_uint		csum = count;
	cl_ulong	bsum = bytes;

#pragma unroll
	for (int d = 1; d < STROM_WAVE; d <<= 1)
	{
		cl_uint		oc = __shfl_up(csum, d, STROM_WAVE);
		cl_ulong	ob = (cl_ulong)__shfl_up((unsigned long long)bsum, d, STROM_WAVE);
		if (lane >= (cl_uint)d)
		{
			csum += oc;
			bsum += ob;
		}
	}
	if (lane == STROM_WAVE - 1)
	{
		wave_count[wave] = csum;
		wave_bytes[wave] = bsum;
	}
	__syncthreads();
	cl_uint		cbefore = csum - count, ctotal = 0;
	cl_ulong	bbefore = bsum - bytes, btotal = 0;
	for (cl_uint w = 0; w < blockDim.x / STROM_WAVE; w++)
	{
		if (w < wave)
		{
			cbefore += wave_count[w];
			bbefore += wave_bytes[w];
		}
		ctotal += wave_count[w];
		btotal += wave_bytes[w];
	}
	__syncthreads();							/* the arrays are free for the next call */
	*p_count_before = cbefore;
	*p_bytes_before = bbefore;
	*p_count_total = ctotal;
	*p_bytes_total = btotal;
}

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
keyunion_count(keyunion_args a)
{
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	keyunion_tile *tiles = (keyunion_tile *)a.tiles;
	cl_int		errcode = StromError_Success;

	for (cl_uint t = blockIdx.x; t < a.ntiles; t += gridDim.x)
	{
		cl_uint		i = t * blockDim.x + threadIdx.x;
		cl_uint		slot = 0, size = 0, rank, count;
		cl_ulong	before, bytes;
		bool		isnew = (i < a.nimg && keyunion_is_new(&errcode, a, i, &slot, &size));

		keyunion_block_sums(isnew ? 1u : 0u, (cl_ulong)STROM_INTALIGN(size), &rank, &before, &count, &bytes);
		if (threadIdx.x == 0)
		{
			tiles[t].bytes = bytes;
			tiles[t].count = count;
			tiles[t].__pad = 0;
		}
	}
	textdict_writeback_status(&ctl->status, errcode);
}

/* one work-group (the host launches no more): tiles[] of counts -> tiles[] of offsets, strip by
 * strip with the sums so far carried along; tiles[ntiles] = the totals */
extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
keyunion_offsets(keyunion_args a)
{
	keyunion_tile *tiles = (keyunion_tile *)a.tiles;
	cl_uint		carry_count = 0;
	cl_ulong	carry_bytes = 0;

	if (blockIdx.x != 0)
		return;
	for (cl_uint base = 0; base < a.ntiles; base += blockDim.x)
	{
		cl_uint		t = base + threadIdx.x;
		cl_uint		count = (t < a.ntiles ? tiles[t].count : 0u), cbefore, ctotal;
		cl_ulong	bytes = (t < a.ntiles ? tiles[t].bytes : 0UL), bbefore, btotal;

		keyunion_block_sums(count, bytes, &cbefore, &bbefore, &ctotal, &btotal);
		if (t < a.ntiles)
		{
			tiles[t].count = carry_count + cbefore;
			tiles[t].bytes = carry_bytes + bbefore;
		}
		carry_count += ctotal;
		carry_bytes += btotal;
	}
	if (threadIdx.x == 0)
	{
		tiles[a.ntiles].count = carry_count;
		tiles[a.ntiles].bytes = carry_bytes;
		tiles[a.ntiles].__pad = 0;
	}
}

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
keyunion_settle(keyunion_args a)
{
	cl_ulong   *slots = (cl_ulong *)a.slots;
	textdict_entry *entries = (textdict_entry *)a.entries;
	char	   *heap = (char *)a.heap;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	const keyunion_tile *tiles = (const keyunion_tile *)a.tiles;
	const cl_uint nnew = tiles[a.ntiles].count;
	cl_int		errcode = StromError_Success;

	for (cl_uint t = blockIdx.x; t < a.ntiles; t += gridDim.x)
	{
		cl_uint		i = t * blockDim.x + threadIdx.x;
		cl_uint		slot = 0, size = 0, rank, count;
		cl_ulong	before, bytes;
		bool		isnew = (i < a.nimg && keyunion_is_new(&errcode, a, i, &slot, &size));
		cl_uint		asize = (cl_uint)STROM_INTALIGN(size);

		keyunion_block_sums(isnew ? 1u : 0u, (cl_ulong)asize, &rank, &before, &count, &bytes);
		if (!isnew)
			continue;
		cl_uint		r = tiles[t].count + rank;
		cl_ulong	at = a.heap_usage + tiles[t].bytes + before;
		if (r >= nnew || at + asize > a.heap_size)
		{
			errcode = StromError_SanityCheckViolation;		/* the host sized entries and heap by the totals */
			continue;
		}
		const char *from = (const char *)a.img_heap + keyunion_image_offset(a, i);
		char	   *to = heap + at;
		cl_uint		n = 0;
		for (; n + 8 <= size; n += 8)
			((__attribute__((address_space(1))) textdict_unaligned_u64 *)(to + n))->v = strom_load_u64((const cl_uchar *)from + n);
		for (; n < size; n++)
			to[n] = from[n];
		cl_uint		id = a.nkeys + r;
		cl_ulong	h = textdict_hash((cl_ulong)from, a.blank_padded != 0);
		entries[id].hash = h;
		entries[id].off = at;
		/* only lane i looks for PENDING | i in this slot: the others of this launch find a word
		 * that is not theirs before and after this store */
		__hip_atomic_store((textdict_slot_p)(slots + slot), textdict_tag(h) | id,
						   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	textdict_writeback_status(&ctl->status, errcode);
}

extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
keyunion_emit(keyunion_args a)
{
	const cl_ulong *slots = (const cl_ulong *)a.slots;
	const cl_uint *key_slot = (const cl_uint *)a.key_slot;
	textdict_ctl *ctl = (textdict_ctl *)a.ctl;
	cl_int	   *map = (cl_int *)a.map;
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < a.nimg; base += gridDim.x * blockDim.x)
	{
		cl_uint		i = base + threadIdx.x;

		if (i < a.nimg)
		{
			cl_uint		s = key_slot[i];
			cl_ulong	w = (s < a.nslots ? slots[s] : 0UL);
			cl_int		id = 0;

			if ((w & TEXTDICT_OCCUPIED) == 0 || (w & TEXTDICT_PENDING) != 0 || (cl_uint)w >= a.nkeys)
				errcode = StromError_SanityCheckViolation;
			else
				id = (cl_int)(cl_uint)w;
			map[i] = id;
		}
	}
	textdict_writeback_status(&ctl->status, errcode);
}

/* ids under one dictionary -> ids under another, in place; a NULL row's id becomes 0 without a
 * look at the map (the dictionary the chunk was encoded under may hold no key at all) */
extern "C" __global__ void __launch_bounds__(TEXTDICT_BLOCK)
keyunion_recode(kern_data_store *chunk, keyunion_recode_args a)
{
	const kern_coldir *cd = KERN_DATA_STORE_COLDIR(chunk) + a.colidx;
	cl_int	   *ids = (cl_int *)((char *)chunk + cd->values_off);
	const cl_uint *notnull = (cd->nulls_off ? (const cl_uint *)((const char *)chunk + cd->nulls_off) : NULL);
	const cl_int *map = (const cl_int *)a.map;
	const cl_uint nrows = chunk->nitems;
	cl_int		errcode = StromError_Success;

	for (cl_uint base = blockIdx.x * blockDim.x; base < nrows; base += gridDim.x * blockDim.x)
	{
		cl_uint		row = base + threadIdx.x;

		if (row < nrows)
		{
			cl_int		id = 0;

			if (!notnull || ((notnull[row >> 5] >> (row & 31)) & 1) != 0)
			{
				cl_uint		old = (cl_uint)ids[row];
				if (old < a.mapsize)
					id = map[old];
				else
					errcode = StromError_DataStoreCorruption;
			}
			ids[row] = id;
		}
	}
	textdict_writeback_status((cl_int *)a.status, errcode);
}

#endif	/* STROM_TEXTDICT_DEVICE_H */
