/*
 * strom_ctl.h -- what the runtime and its own kernels agree on besides the wire format
 * (strom_kds.h), defined ONCE: the control blocks a .cpp file fills and a kernel takes as an
 * argument (or the host reads back), the records the two exchange, the bounds of their arrays
 * and the layout functions both evaluate.  g++ compiles it into the library
 * ("devlib/strom_ctl.h", after strom_kds.h), hiprtc into every program (strom_gpupreagg.h,
 * strom_hashjoin.h and strom_merge.h include it).  The rule: a block the host writes or reads
 * is defined here and nowhere else.  Plain C++ only -- PODs over the cl_* types, bounds, a few
 * inline functions; no kernel, nothing that depends on generated code (a kernel passes its
 * GPUPREAGG_NKEYS / GPUPREAGG_NAGGS where the host passes its vector sizes).
 *
 * Every struct's size is pinned, with the figure of the separate host copy it replaced; both
 * compilers evaluate the pins, g++ when the library is built, hiprtc whenever a program is.
 * The program cache keys code objects by a digest that covers this file: a stale code object
 * never meets a newer layout.
 */
#ifndef STROM_CTL_H
#define STROM_CTL_H

#if defined(__HIPCC_RTC__)
#define STROM_CTL_FN	static __device__ __forceinline__ constexpr
#else
#define STROM_CTL_FN	static inline constexpr
#endif

/* ---------------------------------------------------------------------- *
 * GpuPreAgg, dense ids
 * ---------------------------------------------------------------------- */
#define GPUPREAGG_MAXKEYS		8		/* == STROM_PREAGG_MAXKEYS of strom_hip.h (runtime.h) */

/* geometry of a session: how the dense ids are laid over LDS, slabs and the table */
struct gpupreagg_dense_ctl {
	cl_uint		ngroups;			/* dense ids in the whole domain */
	cl_uint		nsplits;			/* work-group roles over the id range */
	cl_uint		groups_per_split;
	cl_uint		nrep;				/* LDS replicas, power of two */
	cl_uint		nslabs;				/* == gridDim.x */
	cl_uint		nkeys;
	cl_ulong	slab_bytes;
	cl_long		key_min[GPUPREAGG_MAXKEYS];
	cl_uint		key_range[GPUPREAGG_MAXKEYS];	/* max-min+1; NULL slot == key_range */
	cl_uint		key_stride[GPUPREAGG_MAXKEYS];
	/* compaction (strom_gpupreagg_compact): dense id -> slot of the ids that
	 * actually occur, ~0 = absent; 0 = ids are used as they are */
	cl_ulong	remap;				/* device address of cl_uint[dense_ngroups] */
	cl_uint		dense_ngroups;		/* product of (key_range + 1) */
	cl_uint		merge_ws;			/* stripes of the slab merge (power of two <= 64), 0 = derive */
};
static_assert(sizeof(gpupreagg_dense_ctl) == 176, "gpupreagg_dense_ctl");

/*
 * the per-chunk words of kern_gpupreagg the range proof of the integer sums reads ("integer sums
 * never wrap", strom_gpupreagg.h), written by the host per request.  In the 8 padding bytes: the
 * bit count B of the largest input magnitude -- preset with what is known statically, raised by
 * the folds (atomic max) -- and the rows ONE work-group folds at most; sortbuf_len -- the
 * reference's sort buffer length, no use here -- carries the rows of the whole request.
 */
#define KERN_GPUPREAGG_SUM_MAGBITS(kgp)		((cl_uint *)((kgp)->__padding))
#define KERN_GPUPREAGG_WG_ROWS(kgp)			(*(const cl_uint *)((kgp)->__padding + 4) & 0x7fffffffu)
/* top bit of that word: the host has bounded the sums of PLAIN columns (GPUPREAGG_SUMBITS_<a> 65) and
 * of expressions over decimal columns (66: GPUPREAGG_SUMBOUND_<a>, a formula over the columns' zone
 * maps from the code generator) by the chunk's zone maps -- the fold need not measure them */
#define KERN_GPUPREAGG_ZONE_BOUNDED(kgp)	((*(const cl_uint *)((kgp)->__padding + 4) >> 31) != 0)
#define KERN_GPUPREAGG_FOLD_NROWS(kgp)		((cl_uint)(kgp)->sortbuf_len)
/* ... as the host writes them into the request's staging image (wg_rows saturates) */
#if !defined(__HIPCC_RTC__)
static inline void
kern_gpupreagg_set_chunk_words(kern_gpupreagg *kgp, cl_uint fold_nrows, cl_uint magbits,
							   cl_ulong wg_rows, bool zone_bounded)
{
	cl_uint		words[2] = { magbits, (cl_uint)(wg_rows < 0x7fffffffUL ? wg_rows : 0x7fffffffUL) |
									  (zone_bounded ? 0x80000000u : 0u) };
	kgp->sortbuf_len = (cl_int)fold_nrows;
	__builtin_memcpy(kgp->__padding, words, sizeof(words));
}
#endif

/*
 * Per-group flags: bit 0 = a row of this group passed the qual ("seen"), bit 1+a = aggregate a
 * received a non-NULL input.  One word per (group, replica), as narrow as the aggregates allow
 * (gpupreagg_flags_t on the device).
 */
STROM_CTL_FN cl_uint
gpupreagg_flag_width(cl_uint naggs)
{
	return naggs <= 7 ? 1 : (naggs <= 15 ? 2 : 4);
}

/*
 * LDS / slab image for G groups and REP replicas, sections 16-byte aligned:
 *   section 0        flags[G*REP]
 *   section 1+a      values of aggregate a: u32[G*REP] (NROWS: bit a of nrows_mask) or 8 bytes[G*REP]
 *   section 1+naggs  total size
 * OFF is cl_uint on the device -- the image lives in LDS (<= 160 KB) or in a slab of the same
 * shape -- and size_t on the host, which also asks about images that turn out too large.
 */
template <typename OFF>
STROM_CTL_FN OFF
gpupreagg_image_offset_of(int sec, OFF G, OFF REP, int naggs, cl_uint nrows_mask)
{
	OFF		off = 0;

	if (sec == 0) return off;
	off += ((OFF)gpupreagg_flag_width(naggs) * G * REP + 15) & ~(OFF)15;
	for (int a = 0; a < naggs; a++)
	{
		if (sec == 1 + a) return off;
		off += ((OFF)(((nrows_mask >> a) & 1u) != 0 ? 4 : 8) * G * REP + 15) & ~(OFF)15;
	}
	return off;
}

/*
 * resident table for N groups, 256-byte aligned sections:
 *   section 0          flags as u32[N]
 *   section 1+a        8-byte values[N] (NROWS widened to i64)
 *   section 1+naggs+j  the j-th INTEGER sum's high word, i64[N]: such a sum is
 *                      128 bits wide in the table (low word in its section 1+a,
 *                      two's complement), so a total over any number of chunks
 *                      cannot wrap ("integer sums never wrap", strom_gpupreagg.h)
 */
STROM_CTL_FN size_t
gpupreagg_table_offset(int sec, cl_uint N)
{
	size_t	flags = STROM_TYPEALIGN(256, sizeof(cl_uint) * (size_t)N);
	size_t	vals = STROM_TYPEALIGN(256, 8 * (size_t)N);

	return sec == 0 ? 0 : flags + vals * (size_t)(sec - 1);
}

/* packed accumulators of one launch (strom_gpupreagg.h: gpupreagg_packed_column) */
#define GPUPREAGG_PACK_MAXAGGS	32
struct gpupreagg_pack_ctl {
	cl_uint		count_shift;					/* count field: bits count_shift .. 63 */
	cl_uint		nwords;							/* 1 (the packed word) + float8 sums */
	cl_uint		spill_at;						/* 0, or: a group whose count field reaches this moves to the slab */
	cl_uint		count_limit;					/* spill_at != 0: the count field's largest value */
	cl_uint		shift[GPUPREAGG_PACK_MAXAGGS];	/* kind 2: position of the field in word 0 */
	cl_uint		word[GPUPREAGG_PACK_MAXAGGS];	/* kind 3: the aggregate's own word */
	cl_ulong	mask[GPUPREAGG_PACK_MAXAGGS];	/* kind 2: field mask (after the shift) */
	cl_ulong	vmax[GPUPREAGG_PACK_MAXAGGS];	/* kind 2: max - min of the column (zone map) */
	cl_long		bias[GPUPREAGG_PACK_MAXAGGS];	/* kind 2: min of the column */
};
static_assert(sizeof(gpupreagg_pack_ctl) == 1040, "gpupreagg_pack_ctl");

/* the virtual joined relation of gpupreagg_dense_joined / _lookup: where its columns come from */
#define GPUPREAGG_JOINED_MAXCOLS	64
struct gpupreagg_joined_map {
	cl_uint		ncols;
	cl_int		key_col;			/* outer column (0-based) that is the join key */
	cl_int		key_attlen;
	cl_uint		nslots;
	cl_long		key_min;
	struct {
		cl_int		depth;
		cl_int		col;
		cl_ulong	dimvalues;		/* depth 1: device arrays by slot */
		cl_ulong	dimisnull;
	} c[GPUPREAGG_JOINED_MAXCOLS];
	/* gpupreagg_dense_lookup: packed slot records (hashjoin_build_dimrec_kernel); an inner
	 * column i then has c[i].dimvalues = byte offset of its value in the record and
	 * c[i].dimisnull = its bit in the record's flags word */
	cl_ulong	recs;
	cl_uint		reclen;
	/* NARROW records (hashjoin_dimrec_narrow_kernel, lookup only): reclen 2 or 4, the word is
	 * presence | NULL bits | (value - nmin) fields; inner column i = nmin[i] + field */
	cl_uint		narrow;
	cl_uint		nshift[GPUPREAGG_JOINED_MAXCOLS];
	cl_uint		nmask[GPUPREAGG_JOINED_MAXCOLS];
	cl_long		nmin[GPUPREAGG_JOINED_MAXCOLS];
	/* a TRACKED lookup (RIGHT / FULL: GPUPREAGG_LOOKUP_TRACK) and gpupreagg_dense_lookup_unmatched: the
	 * session's matched flags of this table, one byte per slot (0 unmatched, 1 matched); 0 otherwise */
	cl_ulong	matches;
	/* gpupreagg_dense_lookup_unmatched: the work-groups of a role that walk the slots (the others
	 * only store their empty slab); 0: all of them */
	cl_uint		unmatched_wgs;
	cl_uint		__pad;
};
static_assert(sizeof(gpupreagg_joined_map) == 2616, "gpupreagg_joined_map");

/*
 * the virtual joined relation of gpupreagg_dense_lookup_star / _packed_lookup_star: a star of
 * relations 1 .. nrels, each a DIRECT unique-key table probed by an outer column of its own; a
 * virtual column of depth d comes from relation d's slot record.  What is a fact of the mapping
 * (the relation count, per relation the record length and form, the key's width and which columns
 * it serves) is ALSO compiled into the program (GPUPREAGG_STAR_*): the kernel reads the rest here.
 */
#define GPUPREAGG_STAR_MAXRELS		4		/* == STROM_LOOKUP_STAR_MAXRELS of strom_hip.h */
#define GPUPREAGG_STAR_MAXRECLEN	16		/* one relation's slot record, two relations and more */
#define GPUPREAGG_STAR_MAXRECBYTES	32		/* ... and all relations' records of a row together */
struct gpupreagg_star_map {
	cl_uint		ncols;
	cl_uint		nrels;
	struct {
		cl_int		key_col;		/* outer column (0-based) that is this relation's join key */
		cl_int		key_attlen;		/* 4 or 8 */
		cl_uint		nslots;
		cl_uint		reclen;			/* 2 / 4 (narrow), 8 or 16 */
		cl_long		key_min;
		cl_ulong	recs;			/* device address of the slot records */
		cl_uint		narrow;
		cl_uint		__pad;
	} rel[GPUPREAGG_STAR_MAXRELS];
	struct {
		cl_int		depth;			/* 0: outer column 'col'; d: column 'col' of relation d */
		cl_int		col;
		cl_uint		recoff;			/* standard records: byte offset of the value in the record */
		cl_uint		nullbit;		/* its bit in the record's flags word */
		cl_uint		nshift;			/* narrow records: value = nmin + ((word >> nshift) & nmask) */
		cl_uint		nmask;
		cl_long		nmin;
	} c[GPUPREAGG_JOINED_MAXCOLS];
	/* the matched flags of the TRACKED relation (GPUPREAGG_STAR_TRACK_REL), one byte per slot of it; 0: none */
	cl_ulong	matches;
};
static_assert(sizeof(gpupreagg_star_map) == 2224, "gpupreagg_star_map");

/* key range of one chunk (gpupreagg_keyrange), read back by the host */
struct gpupreagg_keyrange_t {
	cl_long		kmin[GPUPREAGG_MAXKEYS];
	cl_long		kmax[GPUPREAGG_MAXKEYS];
	cl_uint		nvalues[GPUPREAGG_MAXKEYS];		/* != 0: the key had a non-NULL value */
	cl_uint		nrows;							/* != 0: a row passed the qual */
	cl_uint		__pad;
};
static_assert(sizeof(gpupreagg_keyrange_t) == 168, "gpupreagg_keyrange_t");

/* ---------------------------------------------------------------------- *
 * GpuPreAgg, hashed GROUP BY: the table is a head, then one record per slot
 *
 *   +0   state  u32     0 empty, 1 being claimed, 2 ready
 *   +4   knull  u32     bit k: key k is NULL
 *   +8   flags  u32     bit 0 seen, bit 1+a aggregate a has a value
 *   +16  keys[nkeys]    u64 images
 *        vals[naggs]    8 bytes each (NROWS widened to i64, float min/max as
 *                       order-preserving keys, like the dense table)
 *
 * records start GPUPREAGG_HASH_HEAD bytes into the table, one every
 * GPUPREAGG_HASH_STRIDE_OF bytes: a probe touches one cache line.
 * ---------------------------------------------------------------------- */
#define GPUPREAGG_HASH_HEAD			256
#define GPUPREAGG_HASH_REC_KEYS		16
#define HASH_REC_STATE(rec)			((cl_uint *)(rec))
#define HASH_REC_KNULL(rec)			((cl_uint *)((rec) + 4))
#define HASH_REC_FLAGS(rec)			((cl_uint *)((rec) + 8))
#define HASH_REC_KEYS(rec)			((cl_ulong *)((rec) + GPUPREAGG_HASH_REC_KEYS))
#define GPUPREAGG_HASH_RECLEN_OF(nkeys, naggs)	(GPUPREAGG_HASH_REC_KEYS + 8 * ((nkeys) + (naggs)))
#define GPUPREAGG_HASH_STRIDE_OF(nkeys, naggs)											\
	(GPUPREAGG_HASH_RECLEN_OF(nkeys, naggs) <= 32 ? 32 :								\
	 GPUPREAGG_HASH_RECLEN_OF(nkeys, naggs) <= 64 ? 64 :								\
	 ((GPUPREAGG_HASH_RECLEN_OF(nkeys, naggs) + 127) / 128 * 128))

struct gpupreagg_hash_head {
	cl_uint		capacity;			/* power of two */
	cl_uint		nkeys;
	cl_uint		ngroups;			/* slots claimed so far */
	cl_uint		overflow;			/* set when a probe found no free slot */
	cl_uint		stride;				/* GPUPREAGG_HASH_STRIDE_OF, written by the host and by gpupreagg_hash_init */
	cl_uint		naggs;
	cl_uint		__pad[2];
	/*
	 * integer sums never wrap ("integer sums never wrap", strom_gpupreagg.h -- here for a table whose
	 * accumulators are 64 bits wide and are updated by atomics all over the chip): an upper
	 * bound of |any partial sum in this table|, the sum over the folded chunks of
	 * rows x 2^(bits of the largest input magnitude).  While it stays below 2^63 nothing can have
	 * wrapped and nothing is checked.  Two slots: the fold of turn k reads slot k & 1 and
	 * (its first work-group) writes the other, which the fold of turn k + 1 reads -- no
	 * work-group of a launch reads what another one of it writes.  The host counts a turn
	 * where it queues the first launch of a request's fold, and every such launch writes
	 * the other slot, whether it folds (gpupreagg_hash_sum_account) or not (.._sum_carry).
	 */
	cl_ulong	sum_bound[2];
};
static_assert(sizeof(gpupreagg_hash_head) == 48 && sizeof(gpupreagg_hash_head) <= GPUPREAGG_HASH_HEAD,
			  "gpupreagg_hash_head");
static_assert(offsetof(gpupreagg_hash_head, sum_bound) == 32, "gpupreagg_hash_head.sum_bound");

/*
 * the work-group's LDS table in front of the global one (gpupreagg_hash_lds): after the dense
 * kernels' image for its slots, per slot a state word, the NULL bits and the key images; then, with
 * hash roles, GPUPREAGG_HASH_QUEUE queued row numbers per wave (a power of two, >= 64 * (UNROLL + 1))
 */
#define GPUPREAGG_HASH_LDS_ENTRY(nkeys)		(2 * sizeof(cl_uint) + sizeof(cl_ulong) * (nkeys))
#define GPUPREAGG_HASH_QUEUE				256

/*
 * the groups of a table packed for the host or for another table (gpupreagg_hash_export /
 * _export_parts -> fetch, gpupreagg_hash_import): records of this head, then keys[nkeys] and
 * vals[naggs], 8 bytes each
 */
struct gpupreagg_export_rec {
	cl_uint		knull;
	cl_uint		flags;
	cl_ulong	body[1];			/* really keys[nkeys], vals[naggs] */
};
#define GPUPREAGG_EXPORT_RECLEN(nkeys, naggs)	(offsetof(gpupreagg_export_rec, body) + 8 * ((nkeys) + (naggs)))
static_assert(offsetof(gpupreagg_export_rec, flags) == 4 && offsetof(gpupreagg_export_rec, body) == 8,
			  "gpupreagg_export_rec");

/* the partition plan of a hashed fold (gpupreagg_hash_part_*) */
struct gpupreagg_part_ctl {
	cl_uint		nparts;				/* power of two, <= GPUPREAGG_PART_MAX */
	cl_uint		pshift;
	cl_uint		unit_rows;
	cl_uint		nunits;				/* by gpupreagg_hash_part_plan */
	cl_uint		nrecords;
	cl_uint		deferred;			/* by the claim pass */
	cl_uint		max_units;
	cl_uint		reclen;				/* the host's record length (it sized the buffer): checked by the kernels */
};
static_assert(sizeof(gpupreagg_part_ctl) == 32, "gpupreagg_part_ctl");

/* ---------------------------------------------------------------------- *
 * GpuPreAgg: the fixed-function program (strom_merge.h)
 * ---------------------------------------------------------------------- */
#define PREAGG_MERGE_MAXAGGS	31		/* a flags word: "seen" and one bit per aggregate */
typedef struct {
	cl_uint		ngroups;
	cl_uint		naggs;
	cl_uint		op[PREAGG_MERGE_MAXAGGS];
	cl_uint		__pad;
	cl_ulong	vals_off[PREAGG_MERGE_MAXAGGS];		/* byte offset of section 1+a in the table */
	cl_ulong	hi_off[PREAGG_MERGE_MAXAGGS];		/* op 1: byte offset of the sum's high-word section */
	cl_uint		mid_idx[PREAGG_MERGE_MAXAGGS];		/* op 1: which ngroups-long lane of 'mid' takes bits 32..63 */
	cl_uint		__pad2;
} preagg_merge_spec;
static_assert(sizeof(preagg_merge_spec) == 760, "preagg_merge_spec");

/* preagg_dense_export_rows: the columns of a partial row (kinds: strom_merge.h) */
#define PREAGG_EXPORT_MAXCOLS	64
typedef struct {
	cl_uint		ngroups;
	cl_uint		ncols;
	cl_uint		stride;
	cl_uint		nkeys;
	cl_long		key_min[GPUPREAGG_MAXKEYS];
	cl_uint		key_range[GPUPREAGG_MAXKEYS];
	cl_uint		key_stride[GPUPREAGG_MAXKEYS];
	struct {
		cl_uint		kind;
		cl_uint		len;			/* bytes of the datum */
		cl_uint		which;			/* key number, or the aggregate's has-value bit (1 + a) */
		cl_uint		float4;
		cl_ulong	vals_off;
		cl_ulong	hi_off;
	} col[PREAGG_EXPORT_MAXCOLS];
} preagg_export_spec;
static_assert(sizeof(preagg_export_spec) == 2192, "preagg_export_spec");

/* ---------------------------------------------------------------------- *
 * GpuHashJoin: the probe index and the slot records made from it
 * ---------------------------------------------------------------------- */
#define HASHJOIN_MAXRELS		8

#define HASHJOIN_MODE_HASH		0
#define HASHJOIN_MODE_DIRECT	1
#define HASHJOIN_MODE_KEYED		2

struct hashjoin_index_rel {
	cl_uint		mode;
	cl_uint		nslots;			/* HASH / KEYED: power of two; DIRECT: key range */
	cl_long		key_min;
	cl_uint		unique;			/* no chain longer than one entry */
	cl_uint		slots_off;		/* bytes from the index base to cl_uint slots[] */
	cl_uint		nentries;
	/*
	 * DIRECT + unique keys: the same slots in THREE bytes each -- (entry offset >> 3; entries are
	 * LONGALIGNed, KERN_HASHENTRY_SIZE_BY_TLEN) -- when the table is below 2^27 bytes; 0 = none.
	 * A slot array is probed at random by every CU of an XCD: what counts is whether it fits that
	 * XCD's 4 MB L2 next to the stream.  1.25e6 key values (BASELINE configs[2]) are 5.0 MB as
	 * cl_uint -- one probe in three went to HBM for a 64-byte line -- and 3.75 MB like this.
	 * Made by hashjoin_narrow_slots_kernel, read by gpuhashjoin_main_fast_narrow.
	 */
	cl_uint		slots3_off;
};
struct hashjoin_index {
	cl_uint		nrels;
	/*
	 * RIGHT / FULL joins: the relation whose entries the probe kernels flag (0: none; it is the
	 * program's HASHJOIN_TRACK_DEPTH) and its flag area behind the slot arrays: ONE BYTE per 32-byte
	 * granule of that relation's kern_hashtable, addressed by (entry offset >> 5) -- an entry is at
	 * least 40 bytes long, so at most one starts in a granule.  0x80: an entry starts here, at
	 * 8 x (the low two bits) into the granule (set once, by the index build); 0x40: it was matched
	 * (set by the probes, cleared by strom_hashjoin_table_reset_matches).  track_len is a multiple
	 * of 16 (strom_hashjoin.h: HASHJOIN_FLAG_*).
	 */
	cl_uint		track_depth;
	cl_uint		track_off;		/* bytes from the index base */
	cl_uint		track_len;		/* bytes == granules covered */
	hashjoin_index_rel rel[HASHJOIN_MAXRELS];
};
struct hashjoin_build_stats {
	cl_long		key_min;
	cl_long		key_max;
	cl_uint		nentries;
	cl_uint		intlike;
};
static_assert(sizeof(hashjoin_index_rel) == 32, "hashjoin_index_rel");
static_assert(sizeof(hashjoin_index) == 272, "hashjoin_index");
static_assert(sizeof(hashjoin_build_stats) == 24, "hashjoin_build_stats");

/* inner columns by slot, packed (hashjoin_build_dimrec_kernel), their ranges
 * (hashjoin_dimrec_minmax_kernel) and the narrow form (hashjoin_dimrec_narrow_kernel) */
#define HASHJOIN_DIMREC_MAXCOLS	16
#define HASHJOIN_DIMREC_CODED	(-2)	/* a coded column of the table (int4 ids of a text column, by slot) */
struct hashjoin_dimrec_spec {
	cl_uint		ncols;
	cl_uint		reclen;
	struct {
		cl_int		col;			/* inner column, 0-based; HASHJOIN_DIMREC_CODED: no column of the tuple, the
									 * field is laid out NULL and filled by hashjoin_patch_dimrec_kernel */
		cl_int		attlen;
		cl_uint		offset;			/* of the value inside the record */
		cl_uint		__pad;
	} c[HASHJOIN_DIMREC_MAXCOLS];
};
struct hashjoin_dimrec_range {
	cl_long		vmin[HASHJOIN_DIMREC_MAXCOLS];
	cl_long		vmax[HASHJOIN_DIMREC_MAXCOLS];
	cl_uint		nvalues[HASHJOIN_DIMREC_MAXCOLS];
};
struct hashjoin_dimrec_narrow_spec {
	cl_uint		ncols;
	cl_uint		reclen;				/* 2 or 4 */
	cl_uint		shift[HASHJOIN_DIMREC_MAXCOLS];
	cl_uint		mask[HASHJOIN_DIMREC_MAXCOLS];
	cl_long		vmin[HASHJOIN_DIMREC_MAXCOLS];
};
/*
 * a snowflake flattened at table time (hashjoin_compose_dimrec_kernel): the child relation's standard
 * records joined into the parent's, over the PARENT's slots.  The parent's records hold the link
 * column, the child's key; an output column is a parent's or a child's, copied with its NULL bit
 * (output column i has bit 1 + i, as in every standard record).
 */
struct hashjoin_compose_spec {
	cl_uint		ncols;				/* of the output */
	cl_uint		reclen;
	cl_uint		parent_reclen;
	cl_uint		child_reclen;
	cl_int		link_attlen;		/* 4 or 8 */
	cl_uint		link_offset;		/* the link column in the parent's record ... */
	cl_uint		link_nullbit;		/* ... and its bit in that record's flags word */
	cl_uint		__pad;
	struct {
		cl_uint		from_child;		/* 0: the parent's record, 1: the child's */
		cl_int		attlen;
		cl_uint		src_offset;
		cl_uint		src_nullbit;
		cl_uint		offset;			/* of the value inside the output record */
		cl_uint		__pad;
	} c[HASHJOIN_DIMREC_MAXCOLS];
};
static_assert(sizeof(hashjoin_compose_spec) == 416, "hashjoin_compose_spec");
static_assert(sizeof(hashjoin_dimrec_spec) == 264, "hashjoin_dimrec_spec");
static_assert(sizeof(hashjoin_dimrec_range) == 320, "hashjoin_dimrec_range");
static_assert(sizeof(hashjoin_dimrec_narrow_spec) == 264, "hashjoin_dimrec_narrow_spec");

/* ---------------------------------------------------------------------- *
 * text key dictionary (strom_textdict.h, textdict.cpp)
 * ---------------------------------------------------------------------- */
/* the words one encode call exchanges with the host: zeroed before every probe */
struct textdict_ctl {
	cl_int		status;				/* probe: worst row error, NoSpace included */
	cl_uint		nnew;				/* probe: keys claimed by this call */
	cl_uint		nnull;				/* probe: rows whose key is NULL */
	cl_uint		toofull;			/* probe: the claims took the table past half full (a word of its own:
									 * 'status' keeps the row errors' priority) */
	cl_ulong	heap_need;			/* probe: bytes of the new keys' datums, each rounded up to 4 */
	cl_ulong	heap_cursor;		/* settle: bytes handed out so far, on top of heap_usage */
};
/* entries[id]: where key 'id' lies in the dictionary heap, and its (masked) hash */
struct textdict_entry {
	cl_ulong	hash;
	cl_ulong	off;
};
/* newkeys[k]: the slot a probe claimed and the row of this chunk whose datum it stands for */
struct textdict_newkey {
	cl_uint		slot;
	cl_uint		row;
};
/* the kernels' argument (device addresses as cl_ulong: one layout for both compilers) */
struct textdict_args {
	cl_ulong	slots;				/* cl_ulong[nslots] */
	cl_ulong	entries;			/* textdict_entry[>= nkeys + nnew] */
	cl_ulong	heap;				/* char[heap_size] */
	cl_ulong	ctl;				/* textdict_ctl */
	cl_ulong	row_slot;			/* cl_uint[nrows]: the row's slot, ~0 = NULL or failed row */
	cl_ulong	newkeys;			/* textdict_newkey[nrows] */
	cl_ulong	heap_usage;			/* bytes of the heap in use before this call */
	cl_ulong	heap_size;
	cl_ulong	out_values;			/* emit: cl_int[nrows] of the encoded chunk */
	cl_ulong	out_notnull;		/* emit: its notnull bitmap */
	cl_uint		nslots;				/* power of two */
	cl_uint		nkeys;				/* keys before this call; rebuild: all keys */
	cl_uint		nnew;				/* settle */
	cl_uint		colidx;				/* the key column of the source chunk */
	cl_uint		blank_padded;		/* character(n): trailing blanks do not count */
	cl_uint		__pad;
};
static_assert(sizeof(textdict_ctl) == 32, "textdict_ctl");
static_assert(sizeof(textdict_entry) == 16, "textdict_entry");
static_assert(sizeof(textdict_newkey) == 8, "textdict_newkey");
static_assert(sizeof(textdict_args) == 104, "textdict_args");
/* a text column of a hash table's one relation (DIRECT index, unique keys) under the dictionary, by SLOT
 * of the table (textdict_table_*): the second argument of those kernels, next to a textdict_args whose
 * row_slot / newkeys are tbl_nslots long and whose "rows" are the table's slots */
struct textdict_table_args {
	cl_ulong	kmhash;				/* the table's kern_multihash image: read-only for the whole call */
	cl_ulong	hjidx;				/* its hashjoin_index */
	cl_ulong	datum_off;			/* cl_ulong[tbl_nslots]: the slot's checked datum, bytes from kmhash;
									 * 0 = no row in the slot, or a NULL column */
	cl_ulong	out_ids;			/* emit: cl_int[tbl_nslots] */
	cl_ulong	out_isnull;			/* emit: cl_uchar[tbl_nslots], 1 = absent slot or NULL datum (id 0) */
	cl_uint		tbl_nslots;			/* hashjoin_index_rel.nslots, <= 2^31 */
	cl_int		colidx;				/* the relation's column, attlen -1 */
};
static_assert(sizeof(textdict_table_args) == 48, "textdict_table_args");

/* ---------------------------------------------------------------------- *
 * union of key dictionaries (strom_textdict.h: keyunion_*, textdict.cpp)
 * ---------------------------------------------------------------------- */
/* one absorb: the keys of an image -- complete varlena datums in img_heap, key i at the offset read
 * from img_offsets + i * img_stride -- enter the dictionary {slots, entries, heap}; the image is
 * read-only for the whole absorb.  The call's status and claim count go through the dictionary's
 * textdict_ctl (status, nnew, toofull; the other words are not used). */
struct keyunion_args {
	cl_ulong	slots;				/* the absorbing dictionary's, as in textdict_args */
	cl_ulong	entries;
	cl_ulong	heap;
	cl_ulong	ctl;
	cl_ulong	img_heap;			/* const char[img_heaplen] */
	cl_ulong	img_offsets;		/* the first of nimg cl_ulong offsets into img_heap, img_stride bytes apart:
									 * 8 = an offsets array, 16 = the 'off' words of a dictionary's entries[] */
	cl_ulong	img_heaplen;
	cl_ulong	key_slot;			/* cl_uint[nimg]: the slot of image key i, ~0 = failed key */
	cl_ulong	tiles;				/* keyunion_tile[ntiles + 1], a tile being TEXTDICT_BLOCK image keys in a row:
									 * count: its new keys; offsets: the new keys before it, [ntiles] = all */
	cl_ulong	map;				/* emit: cl_int[nimg], id of image key i under the dictionary */
	cl_ulong	heap_usage;			/* bytes of the heap in use before this call */
	cl_ulong	heap_size;
	cl_uint		img_stride;
	cl_uint		nimg;
	cl_uint		ntiles;
	cl_uint		nslots;				/* power of two */
	cl_uint		nkeys;				/* keys before this call; emit: after it */
	cl_uint		blank_padded;
};
/* new keys of a tile (or before it), and the heap bytes of their datums, each rounded up to 4 */
struct keyunion_tile {
	cl_ulong	bytes;
	cl_uint		count;
	cl_uint		__pad;
};
/* recode: ids[row] = map[ids[row]] over the int4 column 'colidx' of a COLUMN chunk */
struct keyunion_recode_args {
	cl_ulong	map;				/* const cl_int[mapsize] */
	cl_ulong	status;				/* cl_int: worst row error */
	cl_uint		mapsize;
	cl_uint		colidx;
};
static_assert(sizeof(keyunion_args) == 120, "keyunion_args");
static_assert(sizeof(keyunion_tile) == 16, "keyunion_tile");
static_assert(sizeof(keyunion_recode_args) == 24, "keyunion_recode_args");

#endif	/* STROM_CTL_H */
