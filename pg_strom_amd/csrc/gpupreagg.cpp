/*
 * gpupreagg.cpp -- host side of GpuPreAgg
 *
 * Role in the reference: clserv_process_gpupreagg (gpupreagg.c:3849-4240)
 * and clserv_respond_gpupreagg (3009-3194): send the chunk, run
 * preparation -> (set_rindex | bitonic sort) -> reduction, read back the
 * partial rows; plus pgstrom_create_gpupreagg (2329-2416) which sizes the
 * buffers.  Here a request folds its chunk into a per-GPU table that stays
 * in HBM (see strom_hip.h) using strom_gpupreagg.h's dense-id kernels; the
 * geometry decisions -- how many LDS replicas, how many id-range roles,
 * how many work-groups -- are made below from the group domain, which is
 * the job clserv_compute_workgroup_size + the sort-size heuristics
 * (gpupreagg.c:4105-4141) do in the reference.
 */
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <cstdio>
#include <algorithm>

#include "runtime.h"

using namespace strom;

/* a scratch session of a hashed one, its program built with GPUPREAGG_CHECKED (defined below) */
static strom_gpupreagg *gpupreagg_exact_child(strom_gpupreagg *sess, int *p_errcode);

namespace {

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}	/* namespace */

struct strom_gpupreagg {
	strom_devprog_key	key = 0;
	Program			   *prog = nullptr;
	Device			   *dev = nullptr;
	std::vector<strom_preagg_target> targets;
	std::vector<int>	agg_resno, key_resno;
	std::vector<char>	kparams;			/* kern_parambuf image */
	bool				has_domain = false;
	gpupreagg_dense_ctl			ctl;
	size_t				lds_bytes = 0;
	size_t				table_bytes = 0;
	char			   *table = nullptr;	/* resident table (device) */
	bool				table_owned = false;
	char			   *d_ctl = nullptr;	/* device copy of ctl */
	char			   *d_slabs = nullptr;
	int					block = 1024, quads = 2;
	/* compaction of the dense ids that occur (census -> compact) */
	char			   *d_census = nullptr;	/* bitmap over dense ids (device) */
	char			   *d_remap = nullptr;
	std::vector<cl_uint> present;			/* table slot -> dense id */
	size_t				nfolds = 0;
	/* hashed GROUP BY (strom_gpupreagg_create_hashed) */
	bool				hashed = false;
	char			   *htab = nullptr;
	size_t				htab_bytes = 0;
	cl_uint				hash_capacity = 0;
	cl_ulong			groups_upper = 0;	/* groups known at the last read-back + rows folded since */
	std::atomic<cl_uint> groups_known{0};	/* groups at the last read-back (or the caller's hint) */
	int					reg_groups = 0;		/* 1: register accumulators, 2: lane-private LDS, 0: LDS atomics */
	/* packed accumulators (gpupreagg_packed_column): what the generated code says
	 * about every aggregate, and the launch geometry per role count */
	/* a partial accumulated in the 64-bit numeric form (compare-and-swap in LDS,
	 * checked merge): LDS-atomics kernel only, one replica, no RCCL SUM */
	bool				numeric_aggs = false;
	bool				packable = false;
	std::vector<int>	pack_kind, pack_attno;
	struct packed_geom {
		gpupreagg_dense_ctl	ctl;
		char	   *d_ctl = nullptr;
		char	   *d_slabs = nullptr;		/* two buffers of nslabs * slab_bytes (see slab_turn) */
		size_t		lds_bytes = 0;
	};
	/*
	 * Fold k+1 runs while merge k adds its slabs to the table (resident chunks: the
	 * merge has a stream of its own): slabs are double-buffered, slab_turn picks the
	 * buffer, merge_ev[b] is recorded behind the merge that last read buffer b --
	 * the next fold into b waits for it, and so does the next merge (the table is
	 * read-modify-written in request order)
	 */
	unsigned			slab_turn = 0;
	hipEvent_t			merge_ev[2] = {nullptr, nullptr};
	bool				merge_ev_used[2] = {false, false};
	std::mutex			launch_lock;
	std::map<cl_uint, packed_geom> packed;		/* by number of roles */
	size_t				packed_static_lds = ~(size_t)0;
	std::mutex			lock;
	/*
	 * integer sums never wrap (strom_gpupreagg.h): per aggregate the static magnitude bound
	 * the code generator found (GPUPREAGG_SUMBITS_<a>: 0 not an integer sum, 1..63 bits, 64
	 * none), the OR of the static bounds (preset in every request's kern_gpupreagg) and the
	 * aggregates whose sums are 128 bits wide in the resident table.  (A chunk whose range proof
	 * failed is folded by the program built with GPUPREAGG_CHECKED: checked_program)
	 */
	std::vector<int>	sumbits;
	std::vector<std::string> sumbound;	/* sumbits 66: the code generator's bound formula (eval_sum_bound) */
	cl_uint				static_magbits = 0;		/* the largest static bound, in bits */
	bool				sums_measured = false;	/* an integer sum without a static bound */
	std::vector<int>	intsum_of;			/* aggregate -> index among the integer sums, or -1 */
	int					nintsums = 0;
	std::atomic<cl_uint> checked_folds{0};	/* (reported: chunks that took the checked program) */
	cl_uint				sum_turn = 0;		/* hashed: folds queued so far; its parity is the next fold's (gpupreagg_hash_sum_account) */
	/* the session's source built behind a define block -- FOR a column mapping (lookup_mapping_program,
	 * star_mapping_program), with GPUPREAGG_CHECKED (checked_program) -- by that block */
	std::map<std::string, std::pair<strom_devprog_key, Program *>> lookup_programs;	/* (program_with_defines) */
	/*
	 * the matched flags of the TRACKED relation of this session's lookup folds (RIGHT / FULL joins:
	 * strom_submit_gpupreagg_lookup_tracked): one byte per slot of that table, 0 unmatched, 1 matched.  The
	 * slot records belong to the table and are shared between sessions; what matched is a fact of one query,
	 * so the flags are the session's -- made (zeroed) by its first tracked request or its unmatched call,
	 * bound to (table, tracked position, slots) from then on, freed with the session.  (under 'lock')
	 */
	char			   *d_matches = nullptr;
	size_t				matches_len = 0;			/* == the table's nslots */
	uint64_t			matches_serial = 0;			/* the table (hashjoin_table_null_key_entries) */
	int					matches_pos = 0;			/* the tracked relation, 1-based */
	bool				unmatched_done = false;		/* the unmatched pass ran: no fold, no second pass before a reset */
	char			   *d_export_spec = nullptr;	/* preagg_export_spec of this table (fetch on the device) */
	/* the program's text / character(n) variables: { attno, type oid } (its STROM_KVARLENA_LIST) */
	std::vector<std::pair<int, int>> varlena_vars;

	/* the LDS / slab image of this session's aggregates (strom_ctl.h): section 0 = flags,
	 * 1+a = values of aggregate a, 1+naggs = total */
	size_t image_offset(int sec, cl_uint G, cl_uint REP) const
	{
		cl_uint	nrows_mask = 0;
		for (size_t a = 0; a < agg_resno.size() && a < 32; a++)		/* (a flags word has a bit for 31) */
			if (targets[agg_resno[a]].kind == STROM_PREAGG_NROWS)
				nrows_mask |= 1u << a;
		return gpupreagg_image_offset_of<size_t>(sec, G, REP, (int)agg_resno.size(), nrows_mask);
	}
	int nsections() const { return 1 + (int)agg_resno.size(); }
	/* the table has one more section per integer sum: its high word (section 1 + naggs + j) */
	int table_sections() const { return nsections() + nintsums; }
	size_t table_hi_offset(int a, cl_uint N) const { return gpupreagg_table_offset(nsections() + intsum_of[a], N); }
	bool is_intsum(int a) const { return intsum_of[a] >= 0; }
};

namespace {

/* everything queued for the session's table has landed: folds (streams[0]) and
 * the merges that run behind them on the merge stream */
hipError_t
session_quiesce(strom_gpupreagg *sess)
{
	hipError_t rc = hipStreamSynchronize(sess->dev->streams[0]);
	if (rc == hipSuccess && sess->dev->merge_stream)
		rc = hipStreamSynchronize(sess->dev->merge_stream);
	return rc;
}

/* bytes of a fixed-width value of this type: the one width table of this file.  (A column mapping
 * may name a type by its negative oid -- strom_hip.h: "that type, no zone map needed".) */
int
type_length(int type_oid)
{
	switch (type_oid < 0 ? -type_oid : type_oid)
	{
		case STROM_BOOLOID: case STROM_BPCHAROID:	return 1;
		case STROM_INT2OID:							return 2;
		case STROM_INT4OID: case STROM_FLOAT4OID: case STROM_DATEOID:	return 4;
		default:									return 8;
	}
}

bool
type_is_float(int type_oid)
{
	return type_oid == STROM_FLOAT4OID || type_oid == STROM_FLOAT8OID;
}

/*
 * geometry for a domain: how the dense ids are laid over LDS
 */
int	setup_layout(strom_gpupreagg *sess);

int
setup_geometry(strom_gpupreagg *sess, const strom_preagg_domain *dom)
{
	gpupreagg_dense_ctl  &ctl = sess->ctl;

	if (dom->nkeys != (int)sess->key_resno.size() || dom->nkeys > STROM_PREAGG_MAXKEYS)
		return StromError_BadRequestMessage;
	memset(&ctl, 0, sizeof(ctl));
	ctl.nkeys = dom->nkeys;
	cl_ulong	ngroups = 1;
	for (int k = 0; k < dom->nkeys; k++)
	{
		ctl.key_min[k] = dom->key_min[k];
		ctl.key_range[k] = dom->key_range[k];
		ctl.key_stride[k] = (cl_uint)ngroups;
		ngroups *= (cl_ulong)dom->key_range[k] + 1;		/* + NULL slot */
		if (ngroups > (1UL << 26))
			return StromError_DataStoreOutOfRange;		/* too sparse for dense ids */
	}
	ctl.ngroups = (cl_uint)ngroups;
	ctl.dense_ngroups = (cl_uint)ngroups;
	ctl.remap = 0;
	sess->present.clear();
	return setup_layout(sess);
}

/*
 * how ctl.ngroups table slots are laid over LDS
 */
int
setup_layout(strom_gpupreagg *sess)
{
	Device	   *dev = sess->dev;
	gpupreagg_dense_ctl  &ctl = sess->ctl;
	size_t		lds_budget = std::min<size_t>(dev->prop.sharedMemPerBlock, 160 * 1024) - 8192;	/* static LDS: remap stage, scan scratch */

	if (const char *v = getenv("STROM_GPUPREAGG_LDS_BUDGET"))
		lds_budget = (size_t)atol(v);
	size_t	one = sess->image_offset(sess->nsections(), ctl.ngroups, 1);
	if (one <= lds_budget)
	{
		ctl.nsplits = 1;
		ctl.groups_per_split = ctl.ngroups;
		/* replicas: as many as fit, power of two, at most one per lane of
		 * a wave -- a wave's 64 lanes then never share an address */
		cl_uint rep = 1;
		while (rep < 64 &&
			   sess->image_offset(sess->nsections(), ctl.ngroups, rep * 2) <= lds_budget / 2)
			rep *= 2;
		ctl.nrep = rep;
	}
	else
	{
		cl_uint nsplits = (cl_uint)((one + lds_budget - 1) / lds_budget);
		for (;;)
		{
			cl_uint G = (ctl.ngroups + nsplits - 1) / nsplits;
			if (sess->image_offset(sess->nsections(), G, 1) <= lds_budget)
			{
				ctl.groups_per_split = G;
				break;
			}
			nsplits++;
		}
		ctl.nsplits = nsplits;
		ctl.nrep = 1;
		if (nsplits > 64)
			return StromError_DataStoreOutOfRange;
	}
	if (const char *v = getenv("STROM_GPUPREAGG_NREP"))
		ctl.nrep = std::max(1, atoi(v));
	if (sess->numeric_aggs)
		ctl.nrep = 1;			/* replicas are folded with plain merges: no error path there */
	/*
	 * a handful of groups: no LDS atomics at all.  One group (no GROUP BY):
	 * register accumulators (gpupreagg_reg1_column); up to 32: lane-private
	 * LDS accumulators (gpupreagg_priv_column) when [group][thread] arrays
	 * for a 256-thread work-group fit the budget.
	 */
	sess->reg_groups = 0;
	size_t	priv_bytes = 0;
	if (ctl.nsplits == 1 && ctl.ngroups <= 32 && !sess->numeric_aggs && !getenv("STROM_GPUPREAGG_NO_REG"))
	{
		size_t	priv_budget = 64 * 1024;
		if (const char *v = getenv("STROM_GPUPREAGG_PRIV_LDS"))
			priv_budget = (size_t)atol(v);
		size_t	per_entry = 0;
		for (int resno : sess->agg_resno)
			per_entry += (sess->targets[resno].kind == STROM_PREAGG_NROWS ? 4 : 8);
		priv_bytes = sess->image_offset(sess->nsections(), ctl.ngroups, 1) +
			(size_t)ctl.ngroups * 256 * per_entry;
		/* (lane-private accumulators cost a ds_read + ds_write per aggregate and row, LDS atomics
		 * one ds_add: with Q1's nine aggregates over three groups the private form is the slower
		 * one -- 765 against 749 us per 1e8 rows, profiles/r03_q1_lds_offsets.txt -- so it is
		 * kept for the narrow aggregates it was built for) */
		size_t	priv_entry_max = 32;
		if (const char *v = getenv("STROM_GPUPREAGG_PRIV_ENTRY"))
			priv_entry_max = (size_t)atol(v);
		if (ctl.ngroups == 1)
			sess->reg_groups = 1;
		else if (priv_bytes <= priv_budget && per_entry <= priv_entry_max)
			sess->reg_groups = 2;
		if (sess->reg_groups)
			ctl.nrep = 1;
	}
	sess->lds_bytes = sess->image_offset(sess->nsections(), ctl.groups_per_split, ctl.nrep);
	if (sess->reg_groups == 2)
		sess->lds_bytes = priv_bytes;
	ctl.slab_bytes = STROM_TYPEALIGN(256, sess->image_offset(sess->nsections(), ctl.groups_per_split, 1));
	sess->table_bytes = gpupreagg_table_offset(sess->table_sections(), ctl.ngroups);
	/* work-groups: fill the CUs at the occupancy LDS allows */
	size_t	per_cu = std::max<size_t>(1, std::min<size_t>((size_t)dev->prop.sharedMemPerBlock / (sess->lds_bytes + 4608),	/* + static LDS */
														  2048 / sess->block));
	if (const char *v = getenv("STROM_GPUPREAGG_BLOCKS_PER_CU"))
		per_cu = std::max(1, atoi(v));
	size_t	wgs = (size_t)dev->prop.multiProcessorCount * per_cu;
	wgs = std::max<size_t>(ctl.nsplits, wgs - wgs % ctl.nsplits);
	/* several roles per tile: a multiple of 8 XCDs x nsplits lets the kernel
	 * keep the roles of one tile stream on one XCD (shared L2) */
	if (ctl.nsplits > 1 && wgs >= 8 * (size_t)ctl.nsplits)
		wgs -= wgs % (8 * (size_t)ctl.nsplits);
	if (sess->reg_groups)								/* 256-thread work-groups */
	{
		size_t	fit = std::max<size_t>(1, std::min<size_t>(8, (size_t)(160 * 1024) /
															(sess->lds_bytes + 4608)));
		if (const char *v = getenv("STROM_GPUPREAGG_BLOCKS_PER_CU"))
			fit = std::max(1, atoi(v));
		wgs = (size_t)dev->prop.multiProcessorCount * fit;
	}
	ctl.nslabs = (cl_uint)wgs;
	ctl.merge_ws = 0;
	if (const char *v = getenv("STROM_GPUPREAGG_MERGE_WS"))
	{
		int		w = atoi(v);
		if (w >= 1 && w <= 64 && (w & (w - 1)) == 0)
			ctl.merge_ws = (cl_uint)w;
	}
	sess->has_domain = true;
	return 0;
}

int
alloc_session_buffers(strom_gpupreagg *sess)
{
	Device *dev = sess->dev;
	(void)hipSetDevice(dev->hip_id);
	if (!sess->table)
	{
		sess->table = (char *)dev->pool.alloc(sess->table_bytes);
		if (!sess->table)
			return StromError_OutOfMemory;
		sess->table_owned = true;
		if (hipMemset(sess->table, 0, sess->table_bytes) != hipSuccess)
			return StromError_HipInternal;
	}
	sess->d_ctl = (char *)dev->pool.alloc(sizeof(gpupreagg_dense_ctl));
	sess->d_slabs = (char *)dev->pool.alloc(2 * (size_t)sess->ctl.nslabs * sess->ctl.slab_bytes);
	if (!sess->d_ctl || !sess->d_slabs)
		return StromError_OutOfMemory;
	if (hipMemcpy(sess->d_ctl, &sess->ctl, sizeof(gpupreagg_dense_ctl), hipMemcpyHostToDevice) != hipSuccess)
		return StromError_HipInternal;
	return 0;
}

int
bits_for(cl_ulong v)			/* bits needed to hold values 0..v */
{
	int		n = 0;
	while (v) { n++; v >>= 1; }
	return n;
}

/*
 * Packed accumulators for THIS chunk?  (strom_gpupreagg.h explains the
 * layout.)  Yes when the generated code says every aggregate is count(*) or
 * psum of a plain column, no input column has a NULL bitmap in the chunk,
 * the integer columns' zone maps and the rows one work-group folds bound
 * all fields to one 64-bit word, and the packed image needs FEWER id-range
 * roles than the standard one (each role visits every row).
 * Returns the geometry to launch with, or NULL.
 */
strom_gpupreagg::packed_geom *
packed_plan(strom_gpupreagg *sess, hipFunction_t fn_packed, const kern_coldir *coldir, cl_uint ncols,
			cl_uint nitems, gpupreagg_pack_ctl *pk)
{
	Device	   *dev = sess->dev;
	gpupreagg_dense_ctl  &std_ctl = sess->ctl;

	if (!sess->packable || !fn_packed || !coldir || std_ctl.remap != 0 || std_ctl.nsplits < 2 ||
		getenv("STROM_GPUPREAGG_NO_PACKED"))
		return nullptr;
	if (sess->packed_static_lds == ~(size_t)0)
	{
		int		v = 0;
		if (hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn_packed) != hipSuccess || v < 0)
			v = 8192;
		sess->packed_static_lds = (size_t)v;
	}
	size_t		lds_max = std::min<size_t>(dev->prop.sharedMemPerBlock, 160 * 1024);
	if (sess->packed_static_lds + 1024 >= lds_max)
		return nullptr;
	size_t		lds_budget = lds_max - sess->packed_static_lds - 256;
	cl_uint		naggs = (cl_uint)sess->agg_resno.size();
	cl_uint		nwords = 1;
	memset(pk, 0, sizeof(*pk));
	for (cl_uint a = 0; a < naggs; a++)
	{
		int		kind = sess->pack_kind[a];
		if (kind == 1)
			continue;
		int		col = sess->pack_attno[a] - 1;
		if (col < 0 || col >= (int)ncols || coldir[col].nulls_off != 0)
			return nullptr;					/* a NULL input needs the has-value flags */
		if (kind == 3)
			pk->word[a] = nwords++;
		else if (!(coldir[col].stat_flags & KDS_COLSTAT_MINMAX) || (coldir[col].stat_flags & KDS_COLSTAT_ISFLOAT) ||
				 coldir[col].maxval < coldir[col].minval)
			return nullptr;					/* no zone map to bound the sum with */
	}
	/* roles and work-groups of the packed image */
	size_t		per_group = 8 * (size_t)nwords;
	cl_uint		nsplits = 1;
	cl_uint		G = std_ctl.ngroups;
	while ((size_t)nwords * align16(8 * (size_t)G) > lds_budget)
	{
		nsplits++;
		G = (std_ctl.ngroups + nsplits - 1) / nsplits;
	}
	(void)per_group;
	if (nsplits >= std_ctl.nsplits)
		return nullptr;						/* nothing gained */
	size_t		wgs = (size_t)dev->prop.multiProcessorCount;		/* the image takes a CU's LDS */
	wgs = std::max<size_t>(nsplits, wgs - wgs % nsplits);
	if (nsplits > 1 && wgs >= 8 * (size_t)nsplits)
		wgs -= wgs % (8 * (size_t)nsplits);
	/* field widths: rows one work-group can fold in this chunk, zone-map ranges */
	size_t		tile_rows = (size_t)sess->block * 4 * sess->quads;
	size_t		ntiles = ((size_t)nitems + tile_rows - 1) / tile_rows;
	size_t		wgs_per_split = wgs / nsplits;
	cl_ulong	rows_per_wg = (cl_ulong)((ntiles + wgs_per_split - 1) / wgs_per_split) * tile_rows;
	/*
	 * count field: wide enough for every row the work-group may fold -- or, when the sums do not
	 * leave that much room, NARROW: the fold then adds with the returning atomic and moves a group
	 * to the slab when its count reaches a quarter of the field (strom_gpupreagg.h:
	 * gpupreagg_packed_spill; three quarters of the field are the margin for the adds in flight, so
	 * the field must hold a few tiles' worth of rows).  Uniform keys never get there: 1e4 groups
	 * share the 4e5 rows of a work-group.  (Round 2 flushed the whole table every few tiles
	 * instead -- "epochs": 0.7 GB of extra slab traffic per 1e8 rows and two barriers in the tile
	 * loop, whatever the key distribution.)
	 */
	int			vbits = 0, nsums = 0;
	for (cl_uint a = 0; a < naggs; a++)
	{
		if (sess->pack_kind[a] != 2)
			continue;
		int			col = sess->pack_attno[a] - 1;
		vbits += bits_for((cl_ulong)coldir[col].maxval - (cl_ulong)coldir[col].minval);
		nsums++;
	}
	if (vbits >= 64)
		return nullptr;
	int			cbits = bits_for(rows_per_wg);
	cl_uint		spill_at = 0, count_limit = 0;
	const char *cap = getenv("STROM_GPUPREAGG_PACK_COUNT_BITS");	/* tests: narrow fields on small inputs */
	int			cap_bits = (cap ? atoi(cap) : 0);
	if (vbits + (nsums + 1) * cbits > 64 || (cap_bits > 0 && cap_bits < cbits))
	{
		cbits = (64 - vbits) / (nsums + 1);
		if (cap_bits > 0)
			cbits = std::min(cbits, cap_bits);
		/* 2^cbits rows: at least 4 tiles (a quarter to get there, three for the adds in flight) */
		if (cbits > 31 || (1UL << cbits) < 4 * tile_rows || getenv("STROM_GPUPREAGG_NO_SPILL"))
			return nullptr;
		spill_at = 1u << (cbits - 2);
		count_limit = (1u << cbits) - 1;
	}
	pk->spill_at = spill_at;
	pk->count_limit = count_limit;
	int			pos = 0;
	for (cl_uint a = 0; a < naggs; a++)
	{
		if (sess->pack_kind[a] != 2)
			continue;
		int			col = sess->pack_attno[a] - 1;
		cl_ulong	vrange = (cl_ulong)coldir[col].maxval - (cl_ulong)coldir[col].minval;
		int			width = cbits + bits_for(vrange);
		if (pos + width > 64)
			return nullptr;
		pk->shift[a] = (cl_uint)pos;
		pk->mask[a] = (width >= 64 ? ~0UL : ((1UL << width) - 1));
		pk->vmax[a] = vrange;
		pk->bias[a] = coldir[col].minval;
		pos += width;
	}
	if (pos + cbits > 64)
		return nullptr;
	pk->count_shift = (cl_uint)pos;
	pk->nwords = nwords;
	/* geometry of this role count: control block + slabs, made once */
	std::lock_guard<std::mutex> g(sess->lock);
	auto	it = sess->packed.find(nsplits);
	if (it == sess->packed.end())
	{
		strom_gpupreagg::packed_geom geom;
		geom.ctl = std_ctl;
		geom.ctl.nsplits = nsplits;
		geom.ctl.groups_per_split = G;
		geom.ctl.nrep = 1;
		geom.ctl.nslabs = (cl_uint)wgs;
		geom.ctl.slab_bytes = STROM_TYPEALIGN(256, sess->image_offset(sess->nsections(), G, 1));
		geom.lds_bytes = (size_t)nwords * align16(8 * (size_t)G);
		(void)hipSetDevice(dev->hip_id);
		geom.d_ctl = (char *)dev->pool.alloc(sizeof(gpupreagg_dense_ctl));
		geom.d_slabs = (char *)dev->pool.alloc(2 * (size_t)geom.ctl.nslabs * geom.ctl.slab_bytes);
		if (!geom.d_ctl || !geom.d_slabs ||
			hipMemcpy(geom.d_ctl, &geom.ctl, sizeof(gpupreagg_dense_ctl), hipMemcpyHostToDevice) != hipSuccess)
		{
			if (geom.d_ctl) dev->pool.release(geom.d_ctl);
			if (geom.d_slabs) dev->pool.release(geom.d_slabs);
			return nullptr;
		}
		it = sess->packed.insert({nsplits, geom}).first;
	}
	return &it->second;
}

#define REQ_CHECK_OR(call, what, failed)										\
	do {																	\
		hipError_t __rc = (call);											\
		if (__rc != hipSuccess)												\
		{																	\
			task_fail(task, hip_errcode(__rc, what));						\
			return failed;													\
		}																	\
	} while (0)
#define REQ_CHECK(call, what)	REQ_CHECK_OR(call, what, )

/* where a request's rows come from: that decides the fold kernel, its arguments and the control
 * block it reads (fold_kernels, queue_fold_and_merge, map_column_source) */
enum preagg_kind {
	PREAGG_PLAIN,			/* the chunk's rows, or a row map's */
	PREAGG_JOINED,			/* a finished GpuHashJoin's result pairs (strom_submit_gpupreagg_joined) */
	PREAGG_LOOKUP,			/* the chunk's rows, the join a lookup in the aggregate's pass (..._lookup) */
	PREAGG_STAR,			/* ... a lookup in every relation of a star (..._lookup_star) */
	PREAGG_UNMATCHED,		/* no chunk: the unmatched slots of a tracked relation (..._lookup_unmatched) */
};

struct preagg_request {
	strom_gpupreagg	   *sess = nullptr;
	const kern_data_store *kds = nullptr;
	strom_dstore	   *kds_dev = nullptr;
	const kern_row_map *krowmap = nullptr;
	strom_rowmap	   *rowmap_dev = nullptr;	/* device-resident row map (chained operators) */
	uint32_t			format = 0;
	uint32_t			nrows = 0;
	preagg_kind			kind = PREAGG_PLAIN;
	/* joined: the join's result pairs */
	const void		   *joined_results = nullptr;	/* device kern_resultbuf */
	void			   *joined_buffer = nullptr;	/* the join's device image, owned by this request now */
	/* the program to fold with when it is not the session's own: the one built for this column
	 * mapping (lookup, star), or the checked one of a retry (checked_program) */
	Program			   *prog = nullptr;
	/* joined, lookup, unmatched: a gpupreagg_joined_map; star: a gpupreagg_star_map (write_joined_map / write_star_map) */
	std::shared_ptr<std::vector<char>> map;
	/* the define block 'prog' was built with, for checked_program to build again behind GPUPREAGG_CHECKED: a star's,
	 * and a TYPED one-table lookup's.  EMPTY for an inner one-table lookup, on purpose: its checked retry folds with
	 * the session's own source (the run-time form of the kernel), as it always did -- lookup_mapping_program fills
	 * this only where a join type is named, and checked_program relies on that. */
	std::string			mapping_defs;
	/* hashed, exact fold (gpupreagg_hashed_exact): 'sess' is a scratch session of this one */
	strom_gpupreagg	   *exact_parent = nullptr;
};

/* bits of the largest magnitude a zone map allows (strom_gpupreagg.h: gpupreagg_sum_magnitude) */
cl_uint
zone_magbits(const kern_coldir &cd)
{
	cl_long		lo = cd.minval, hi = cd.maxval;
	return (cl_uint)bits_for((cl_ulong)(lo ^ (lo >> 63)) | (cl_ulong)(hi ^ (hi >> 63)));
}

/*
 * bits of the largest magnitude a summed EXPRESSION can take in this chunk: the code generator's
 * formula (codegen_preagg.cpp: sum_bound_formula -- reverse Polish over magnitudes: cN column N's
 * zone map, nN a numeric image column's integer-part bounds, kV a constant, + and *, eK a rescale by
 * 10^K) over the chunk's zone maps.  -1: a column
 * without a zone map, or a malformed formula -- the fold measures the rows then.
 */
int
eval_sum_bound(const std::string &formula, const kern_coldir *cd, cl_uint ncd)
{
	std::vector<unsigned __int128> st;
	const unsigned __int128 CAP = (unsigned __int128)1 << 100;		/* saturate well above 2^64 */
	const char *p = formula.c_str();
	while (*p)
	{
		while (*p == ' ')
			p++;
		if (!*p)
			break;
		char	op = *p++;
		if (op == 'c' || op == 'k' || op == 'e' || op == 'n')
		{
			char   *end;
			unsigned long long v = strtoull(p, &end, 10);
			if (end == p)
				return -1;
			p = end;
			if (op == 'c' || op == 'n')
			{
				if (v < 1 || v > ncd)
					return -1;
				const kern_coldir &c = cd[v - 1];
				/* (cN: an integer-like column's zone map; nN: a numeric image column's integer-part bounds) */
				if (op == 'c' ? (!(c.stat_flags & KDS_COLSTAT_MINMAX) || (c.stat_flags & KDS_COLSTAT_ISFLOAT))
					: !(c.stat_flags & KDS_COLSTAT_INTPART))
					return -1;
				if (c.maxval < c.minval)
					return -1;
				cl_ulong lo = (cl_ulong)(c.minval < 0 ? -(unsigned __int128)c.minval : (unsigned __int128)c.minval);
				cl_ulong hi = (cl_ulong)(c.maxval < 0 ? -(unsigned __int128)c.maxval : (unsigned __int128)c.maxval);
				st.push_back(std::max(lo, hi));
			}
			else if (op == 'k')
				st.push_back(v);
			else
			{
				if (st.empty() || v > 38)
					return -1;
				for (unsigned long long i = 0; i < v && st.back() < CAP; i++)
					st.back() *= 10;
			}
		}
		else if (op == '+' || op == '*')
		{
			if (st.size() < 2)
				return -1;
			unsigned __int128 b = st.back();
			st.pop_back();
			unsigned __int128 a = st.back();
			a = std::min(a, CAP);
			b = std::min(b, CAP);
			st.back() = (op == '+' ? a + b : (a == 0 || b == 0) ? 0 : (a > CAP / b ? CAP : a * b));
		}
		else
			return -1;
	}
	if (st.size() != 1)
		return -1;
	unsigned __int128 v = st.back();
	int		bits = 0;
	while (v != 0 && bits < 127)
	{
		v >>= 1;
		bits++;
	}
	return bits;
}

/* the session's source behind a define block, as a program of its own: one per distinct block, made
 * on first use and kept with the session.  A request parks behind its build like behind any cold program. */
Program *
program_with_defines(strom_gpupreagg *sess, const std::string &defs)
{
	std::lock_guard<std::mutex> g(sess->lock);
	auto	it = sess->lookup_programs.find(defs);
	if (it != sess->lookup_programs.end())
		return it->second.second;
	std::string	source = defs + sess->prog->source;
	strom_devprog_key key = strom_get_devprog_key(source.c_str(), sess->prog->extra_flags);
	Program	   *prog = (key ? lookup_program(key) : nullptr);
	if (!prog)
		return nullptr;
	sess->lookup_programs[defs] = std::make_pair(key, prog);
	return prog;
}

/* the column mapping of a fused fold as build_fold_mapping found it, neutral of the control block the
 * kernel reads (write_joined_map, write_star_map lay it out).  Lives on the submitter's stack. */
struct fold_mapping {
	int			ncols = 0, nrels = 0;
	/* per column -- depth, col, recoff, nullbit, nshift / nmask / nmin: the star block's own record */
	decltype(gpupreagg_star_map::c) c;
	/* per relation, as parallel arrays (star_mapping_defines takes four of them as they are) */
	int32_t		key_col[GPUPREAGG_STAR_MAXRELS];		/* outer column (0-based) that is the join key */
	int32_t		key_attlen[GPUPREAGG_STAR_MAXRELS];
	int32_t		reclen[GPUPREAGG_STAR_MAXRELS];
	int32_t		narrow[GPUPREAGG_STAR_MAXRELS];
	uint64_t	inner_mask[GPUPREAGG_STAR_MAXRELS];		/* the virtual columns the relation serves */
	cl_long		key_min[GPUPREAGG_STAR_MAXRELS];
	cl_uint		nslots[GPUPREAGG_STAR_MAXRELS];
	cl_ulong	recs[GPUPREAGG_STAR_MAXRELS];			/* device address of the slot records */
	/* how the relation's presence enters the fold: 0 inner, 1 left, 2 semi, 3 anti (..._lookup_typed) */
	int32_t		jointype[GPUPREAGG_STAR_MAXRELS] = {};
	/* the tracked relation (1-based, 0: none) and the session's matched flags of its table (..._lookup_tracked);
	 * the unmatched pass: the work-groups of a role that walk the slots (0: all) */
	int			tracked = 0;
	cl_ulong	matches = 0;
	cl_uint		unmatched_wgs = 0;
};

/*
 * join-as-a-lookup: the session's source built FOR a column mapping -- which virtual column is an
 * inner one, the slot records' length and form, the key's width become compile-time constants
 * (strom_gpupreagg.h: gpupreagg_dense_lookup_body says what that is worth), and only the lookup
 * and merge kernels are built.  One program per distinct mapping (program_with_defines).
 */
/* the define block of a one-table mapping (strom_gpupreagg.h: GPUPREAGG_LOOKUP_*); an inner join names
 * no join type, so its block -- and its program -- is the one it always was.  "" = no valid mapping */
std::string
lookup_mapping_defines(int keylen, int reclen, int narrow, uint64_t inner_mask, int jointype, bool track = false)
{
	bool	ok = (narrow ? (reclen == 2 || reclen == 4) : (reclen >= 8 && reclen % 4 == 0));
	if (!ok || !(keylen == 4 || keylen == 8) || jointype < 0 || jointype > 3 || (jointype >= 2 && inner_mask != 0) ||
		(track && jointype >= 2))				/* (a tracked relation joins inner or left: RIGHT, FULL) */
		return "";
	char		defs[512];
	int			n = snprintf(defs, sizeof(defs),
			 "#define GPUPREAGG_LOOKUP_ONLY 1\n#define GPUPREAGG_LOOKUP_INNER_MASK 0x%lxUL\n"
			 "#define GPUPREAGG_LOOKUP_RECLEN %u\n#define GPUPREAGG_LOOKUP_NARROW %u\n"
			 "#define GPUPREAGG_LOOKUP_KEYLEN %d\n",
			 (unsigned long)inner_mask, (unsigned)reclen, narrow ? 1u : 0u, keylen);
	if (jointype != 0)
		n += snprintf(defs + n, sizeof(defs) - n, "#define GPUPREAGG_LOOKUP_JOINTYPE %d\n", jointype);
	if (track)
		snprintf(defs + n, sizeof(defs) - n, "#define GPUPREAGG_LOOKUP_TRACK 1\n");
	return defs;
}

Program *
lookup_mapping_program(strom_gpupreagg *sess, const fold_mapping &m, std::string *p_typed_defs, int *p_errcode)
{
	/* the run-time form: any INNER mapping, no build (it knows no join type and no flags: a typed or tracked
	 * lookup is always built) */
	const bool	plain = (m.jointype[0] == 0 && m.tracked == 0);
	if (plain && getenv("STROM_GPUPREAGG_LOOKUP_GENERIC"))
		return nullptr;
	/* (the checks of lookup_mapping_defines hold for every mapping build_fold_mapping describes: keys of 4 or 8
	 * bytes, narrow records of 2 or 4, plain ones of 8, 16, 32 or a multiple of 64 -- hashjoin_table_dimrecs.  An
	 * inner mapping that failed them would fold by the run-time form, which reads any mapping; a typed one has no
	 * other kernel and is refused) */
	std::string	defs = lookup_mapping_defines(m.key_attlen[0], m.reclen[0], m.narrow[0], m.inner_mask[0], m.jointype[0],
											  m.tracked != 0);
	if (plain)
		return (defs.empty() ? nullptr : program_with_defines(sess, defs));
	if (defs.empty())
	{
		*p_errcode = StromError_BadRequestMessage;		/* no valid mapping */
		return nullptr;
	}
	Program	   *prog = program_with_defines(sess, defs);
	if (!prog)
		*p_errcode = StromError_OutOfMemory;
	*p_typed_defs = defs;					/* (checked_program builds it again) */
	return prog;
}

/* the define block of a star mapping (strom_gpupreagg.h: GPUPREAGG_STAR_*); "" = no valid mapping */
std::string
star_mapping_defines(int nrels, const int32_t *keylen, const int32_t *reclen, const int32_t *narrow,
					 const uint64_t *inner_mask, const int32_t *jointype = nullptr, int tracked = 0)
{
	if (nrels < 1 || nrels > GPUPREAGG_STAR_MAXRELS || !keylen || !reclen || !narrow || !inner_mask ||
		tracked < 0 || tracked > nrels || (tracked != 0 && jointype && jointype[tracked - 1] >= 2))
		return "";
	char		buf[256];
	snprintf(buf, sizeof(buf), "#define GPUPREAGG_LOOKUP_ONLY 1\n#define GPUPREAGG_STAR_NRELS %d\n", nrels);
	std::string	defs = buf;
	unsigned	total = 0;
	for (int r = 0; r < nrels; r++)
	{
		bool	ok = (narrow[r] ? (reclen[r] == 2 || reclen[r] == 4) : (reclen[r] == 8 || reclen[r] == 16));
		if (!ok || !(keylen[r] == 4 || keylen[r] == 8))
			return "";
		for (int q = 0; q < r; q++)
			if (inner_mask[q] & inner_mask[r])
				return "";					/* a column has one source */
		total += (unsigned)reclen[r];
		snprintf(buf, sizeof(buf),
				 "#define GPUPREAGG_STAR_RECLEN_%d %d\n#define GPUPREAGG_STAR_NARROW_%d %d\n"
				 "#define GPUPREAGG_STAR_KEYLEN_%d %d\n#define GPUPREAGG_STAR_INNER_MASK_%d 0x%lxUL\n",
				 r + 1, reclen[r], r + 1, narrow[r] ? 1 : 0, r + 1, keylen[r], r + 1, (unsigned long)inner_mask[r]);
		defs += buf;
		/* (an inner relation names no join type: an all-inner star keeps its block and its program) */
		int		jt = (jointype ? jointype[r] : 0);
		if (jt < 0 || jt > 3 || (jt >= 2 && inner_mask[r] != 0))
			return "";						/* a semi or anti relation serves no column */
		if (jt != 0)
		{
			snprintf(buf, sizeof(buf), "#define GPUPREAGG_STAR_JOINTYPE_%d %d\n", r + 1, jt);
			defs += buf;
		}
	}
	if (total > GPUPREAGG_STAR_MAXRECBYTES)
		return "";
	if (tracked != 0)
	{
		snprintf(buf, sizeof(buf), "#define GPUPREAGG_STAR_TRACK_REL %d\n", tracked);
		defs += buf;
	}
	return defs;
}

/* the define block of the unmatched pass (strom_gpupreagg.h: gpupreagg_dense_lookup_unmatched): the tracked
 * relation's record facts and nothing else -- no fact column's width, no key width, so one program serves the
 * one-table call and every star around that relation.  "" = no valid records */
std::string
unmatched_mapping_defines(int reclen, int narrow, uint64_t inner_mask)
{
	if (!(narrow ? (reclen == 2 || reclen == 4) : (reclen >= 8 && reclen % 4 == 0)))
		return "";
	char		defs[384];
	snprintf(defs, sizeof(defs),
			 "#define GPUPREAGG_LOOKUP_ONLY 1\n#define GPUPREAGG_UNMATCHED_RECLEN %u\n"
			 "#define GPUPREAGG_UNMATCHED_NARROW %u\n#define GPUPREAGG_UNMATCHED_INNER_MASK 0x%lxUL\n",
			 (unsigned)reclen, narrow ? 1u : 0u, (unsigned long)inner_mask);
	return defs;
}

/* star of lookups: the session's source built FOR the mapping, like lookup_mapping_program -- and ALWAYS: the
 * star kernels have no run-time-mapping form (STROM_GPUPREAGG_LOOKUP_GENERIC is the one-table call's) */
Program *
star_mapping_program(strom_gpupreagg *sess, const std::string &mapping_defs)
{
	return program_with_defines(sess, mapping_defs);
}

/*
 * the program that folds a request again whose integer sums could not be proven to stay in int8
 * (strom_gpupreagg.h, "integer sums never wrap"): built with GPUPREAGG_CHECKED, on first use --
 * such chunks are rare.  A star's kernels live in its mapping's own program, so that is the one
 * built again; every other kind folds with the session's own source (a lookup: by the run-time
 * form of its kernel).
 */
Program *
checked_program(const preagg_request &req)
{
	/* (a typed one-table lookup brings its block too: the run-time form of the kernel knows no join type) */
	return program_with_defines(req.sess, "#define GPUPREAGG_CHECKED 1\n" +
								((req.kind == PREAGG_STAR || req.kind == PREAGG_LOOKUP || req.kind == PREAGG_UNMATCHED)
								 ? req.mapping_defs : std::string()));
}

/*
 * The fused join-and-aggregate kernels and a program with text / character(n) variables: the
 * kernels stream the outer chunk's column arrays and turn a text column's 8-byte offsets into
 * addresses (strom_gpupreagg.h: strom_kvars_from_outer_column), which is right only when every
 * such variable IS a varlena column of the outer chunk -- it maps to depth 0, the mapping names
 * the variable's own type, and the chunk column has attlen == -1 (oh: the chunk's downloaded
 * head).  A dimension cannot serve one: slot records hold fixed-width values.  Anything else is
 * the caller's BadRequest.  (A program whose only text values are constants or parameters has no
 * such variable and nothing to map: their datums live in the kern_parambuf.)
 */
bool
varlena_mapping_ok(const strom_gpupreagg *sess, int ncols, const int32_t *src_depth,
				   const int32_t *src_colidx, const int32_t *type_oids, const kern_data_store *oh)
{
	for (auto &v : sess->varlena_vars)
	{
		int		i = v.first - 1;
		if (i >= ncols || src_depth[i] != 0 || type_oids[i] != v.second ||
			src_colidx[i] < 0 || src_colidx[i] >= (int)oh->ncols ||
			oh->colmeta[src_colidx[i]].attlen != -1)
			return false;
	}
	return true;
}

/* virtual column i of a lookup's mapping: where it comes from; returns the mapping's column count */
cl_uint
map_column_source(const preagg_request &req, cl_uint i, cl_int *p_depth, cl_int *p_col)
{
	if (req.kind == PREAGG_STAR)
	{
		const gpupreagg_star_map *sm = (const gpupreagg_star_map *)req.map->data();
		*p_depth = sm->c[i].depth;
		*p_col = sm->c[i].col;
		return sm->ncols;
	}
	const gpupreagg_joined_map *jm = (const gpupreagg_joined_map *)req.map->data();
	*p_depth = jm->c[i].depth;
	*p_col = jm->c[i].col;
	return jm->ncols;
}

/*
 * launch step A -- a chunk's column directory (NULL bitmaps present?  zone maps), from the host image
 * or the device store's snapshot.  lookup: that request's VIRTUAL columns, which its program reads -- an
 * outer column brings its own entry, an inner one counts as "may be NULL, no zone map".  cd NULL: none.
 */
struct chunk_coldir {
	const kern_coldir  *cd = nullptr;
	cl_uint				ncols = 0;
	std::shared_ptr<std::vector<kern_coldir>> snap;
	std::vector<kern_coldir> virt;
};

void
chunk_coldir_of(const kern_data_store *kds, strom_dstore *kds_dev, const preagg_request *lookup, chunk_coldir *out)
{
	if (kds)
	{
		out->cd = KERN_DATA_STORE_COLDIR(kds);
		out->ncols = kds->ncols;
	}
	else if ((out->snap = dstore_coldir(kds_dev)) != nullptr)
	{
		out->cd = out->snap->data();
		out->ncols = (cl_uint)out->snap->size();
	}
	if (!out->cd || !lookup)
		return;
	cl_int		depth = 0, col = 0;
	out->virt.resize(map_column_source(*lookup, 0, &depth, &col));
	for (cl_uint i = 0; i < out->virt.size(); i++)
	{
		map_column_source(*lookup, i, &depth, &col);
		memset(&out->virt[i], 0, sizeof(kern_coldir));
		if (depth == 0 && col >= 0 && (cl_uint)col < out->ncols)
			out->virt[i] = out->cd[col];
		else
			out->virt[i].nulls_off = 1;
	}
	out->cd = out->virt.data();
	out->ncols = (cl_uint)out->virt.size();
}

/* per kind, the fold kernel and its packed-accumulator variant (NULL: none); a plain request that
 * streams a COLUMN chunk has kernels of its own (plan_fold) */
const char *const fold_kernels[][2] = {
	/* PREAGG_PLAIN */	{ "gpupreagg_dense_generic", nullptr },
	/* PREAGG_JOINED */	{ "gpupreagg_dense_joined", nullptr },
	/* PREAGG_LOOKUP */	{ "gpupreagg_dense_lookup", "gpupreagg_packed_lookup" },
	/* PREAGG_STAR */	{ "gpupreagg_dense_lookup_star", "gpupreagg_packed_lookup_star" },
	/* PREAGG_UNMATCHED */	{ "gpupreagg_dense_lookup_unmatched", nullptr },
};

/*
 * sums of PLAIN columns (GPUPREAGG_SUMBITS_<a> 65) and of expressions over decimal columns (66)
 * over a COLUMN chunk with zone maps: bounded here, the fold does not measure them (top bit of
 * the second word; the streaming kernels read it, the row-at-a-time ones measure as always).
 * True when every such sum is bounded; *p_bits: bits of the largest magnitude.
 */
bool
zone_sum_bound(const strom_gpupreagg *sess, const kern_coldir *cd, cl_uint ncd, cl_uint *p_bits)
{
	bool		all = (cd != nullptr), any = false;
	cl_uint		zbits = 0;
	for (size_t a = 0; all && a < sess->agg_resno.size(); a++)
	{
		if (sess->sumbits[a] == 66)
		{
			/* an expression over decimal columns: the code generator's formula */
			int		bits = eval_sum_bound(sess->sumbound[a], cd, ncd);
			if (bits < 0 || bits > 63)
				all = false;			/* (no zone map -- or a bound beyond int8: measured, then checked) */
			else
			{
				zbits = std::max(zbits, (cl_uint)bits);
				any = true;
			}
			continue;
		}
		if (sess->sumbits[a] != 65)
			continue;
		int		col = (a < sess->pack_attno.size() ? sess->pack_attno[a] - 1 : -1);
		if (col < 0 || col >= (int)ncd || !(cd[col].stat_flags & KDS_COLSTAT_MINMAX) ||
			(cd[col].stat_flags & KDS_COLSTAT_ISFLOAT) || cd[col].maxval < cd[col].minval)
			all = false;
		else
		{
			zbits = std::max(zbits, zone_magbits(cd[col]));
			any = true;
		}
	}
	*p_bits = zbits;
	return all && any;
}

/* launch step B -- how this request is folded: which kernel, packed accumulators or not, the range
 * proof's inputs.  Host work only (packed_plan makes a role count's geometry once). */
struct fold_plan {
	hipFunction_t	fn = nullptr, fn_merge = nullptr;
	bool			use_column = false;		/* a COLUMN chunk streamed as arrays: no pairs, no lookup, no row map */
	bool			use_reg = false;		/* ... by the register / lane-private kernels */
	strom_gpupreagg::packed_geom *packed = nullptr;
	gpupreagg_pack_ctl pk;
	cl_uint			magbits = 0;			/* what is known about the integer sums' inputs before the fold measures the rest */
	bool			zone_bounded = false;
	size_t			wg_rows = 0;
};

int
plan_fold(Device *dev, Program *prog, const preagg_request &req, bool checked, fold_plan *plan)
{
	strom_gpupreagg *sess = req.sess;
	/* (the unmatched pass walks slots in the lookups' tiles; it reads no chunk: no column directory) */
	bool		use_lookup = (req.kind == PREAGG_LOOKUP || req.kind == PREAGG_STAR || req.kind == PREAGG_UNMATCHED);
	int			errcode = 0;
	const char *name = fold_kernels[req.kind][0], *name_packed = fold_kernels[req.kind][1];

	plan->use_column = (req.kind == PREAGG_PLAIN && req.format == KDS_FORMAT_COLUMN &&
						req.krowmap == nullptr && req.rowmap_dev == nullptr);
	/* (the checked program adds in LDS with returning atomics: the LDS-atomics kernels only) */
	plan->use_reg = (plan->use_column && sess->reg_groups != 0 && !checked);
	if (plan->use_reg)
		name = (sess->reg_groups == 1 ? "gpupreagg_reg1_column" : "gpupreagg_priv_column");
	else if (plan->use_column)
	{
		name = "gpupreagg_dense_column";
		name_packed = "gpupreagg_packed_column";
	}
	plan->fn = prog->get_function(dev, name, &errcode);
	plan->fn_merge = plan->fn ? prog->get_function(dev, "gpupreagg_dense_merge", &errcode) : nullptr;
	if (!plan->fn || !plan->fn_merge)
		return errcode;
	plan->magbits = sess->static_magbits;
	chunk_coldir	dir;
	bool		want_packed = (name_packed && sess->packable && sess->ctl.nsplits > 1 && !checked);
	if (want_packed || (!checked && plan->use_column))
		chunk_coldir_of(req.kds, req.kds_dev, use_lookup ? &req : nullptr, &dir);
	/* packed accumulators for this chunk?  (fewer id-range roles: see packed_plan) */
	if (want_packed)
	{
		int		e2 = 0;
		hipFunction_t fn_packed = prog->get_function(dev, name_packed, &e2);
		plan->packed = packed_plan(sess, fn_packed, dir.cd, dir.ncols, req.nrows, &plan->pk);
		if (plan->packed)
		{
			plan->fn = fn_packed;
			/* the packed fold measures nothing: the zone maps that bound its fields bound
			 * the integer sums' inputs too */
			for (size_t a = 0; a < sess->agg_resno.size(); a++)
				if (sess->pack_kind[a] == 2 && sess->sumbits[a] >= 64)
					plan->magbits = std::max(plan->magbits, zone_magbits(dir.cd[sess->pack_attno[a] - 1]));
		}
	}
	/*
	 * the range proof's inputs (strom_gpupreagg.h, "integer sums never wrap"): rows of the
	 * request, bits of the largest input magnitude known so far, and the rows ONE work-group
	 * folds at most -- tiles (or, row by row, blocks) are dealt round-robin to the work-groups
	 * of a role; one unit of slack
	 */
	const gpupreagg_dense_ctl &g = (plan->packed ? plan->packed->ctl : sess->ctl);
	size_t		unit = (plan->use_reg ? (size_t)256 * 4 * sess->quads
						: (plan->use_column || use_lookup) ? (size_t)sess->block * 4 * sess->quads
						: (size_t)sess->block);
	size_t		units = ((size_t)req.nrows + unit - 1) / unit;
	size_t		wgs_per_role = std::max<size_t>(1, g.nslabs / std::max<cl_uint>(1, g.nsplits));
	plan->wg_rows = std::min<size_t>(((units + wgs_per_role - 1) / wgs_per_role + 1) * unit, 0xffffffffUL);
	cl_uint		zbits = 0;
	if (!plan->packed && !checked && plan->use_column && zone_sum_bound(sess, dir.cd, dir.ncols, &zbits))
	{
		plan->zone_bounded = true;
		plan->magbits = std::max(plan->magbits, zbits);
	}
	return 0;
}

/*
 * launch step C, the dense and the hashed launch alike -- stage and send the kern_gpupreagg image {status,
 * sortbuf_len, pad, kern_parambuf} [+ the pack control block] on s_in, then the chunk and the row map
 * (unless they are resident) on the task's stream
 */
struct sent_request {
	char	   *stage = nullptr;		/* pinned: the image as sent; the status comes back behind it */
	char	   *d_kg = nullptr;
	size_t		kg_len = 0;				/* the kern_gpupreagg image alone */
	size_t		send_len = 0;			/* ... with the pack control block */
	const void *d_kds = nullptr;
	const void *d_rowmap = nullptr;
};

bool
send_request(strom_task_impl *task, const preagg_request &req, hipStream_t s_in,
			 cl_uint magbits, size_t wg_rows, bool zone_bounded, const gpupreagg_pack_ctl *pk, sent_request *out)
{
	strom_gpupreagg *sess = req.sess;
	Device	   *dev = task->dev;
	size_t		kg_len = STROMALIGN(offsetof(kern_gpupreagg, kparams) + sess->kparams.size());
	size_t		send_len = kg_len + (pk ? STROMALIGN(sizeof(gpupreagg_pack_ctl)) : 0);
	char	   *stage = dev->pinned.alloc();
	char	   *d_kg = (char *)dev->pool.alloc(send_len);
	if (!stage || !d_kg || send_len + 64 > PinnedPool::BLOCK)
	{
		if (stage) dev->pinned.release(stage);
		if (d_kg) dev->pool.release(d_kg);
		task_fail(task, StromError_OutOfMemory);
		return false;
	}
	task->pinned_blocks.push_back(stage);
	task->main_devptr = d_kg;
	memset(stage, 0, kg_len);
	memcpy(stage + offsetof(kern_gpupreagg, kparams), sess->kparams.data(), sess->kparams.size());
	kern_gpupreagg_set_chunk_words((kern_gpupreagg *)stage, req.nrows, magbits, wg_rows, zone_bounded);
	if (pk)
		memcpy(stage + kg_len, pk, sizeof(*pk));
	out->stage = stage;
	out->d_kg = d_kg;
	out->kg_len = kg_len;
	out->send_len = send_len;

	task_event(task, s_in);								/* ev[0] */
	REQ_CHECK_OR(hipMemcpyAsync(d_kg, stage, send_len, hipMemcpyHostToDevice, s_in),
				 "send kern_gpupreagg", false);
	task->pfm.num_dma_send++;
	task->pfm.bytes_dma_send += send_len;
	if (req.kind == PREAGG_UNMATCHED)
		out->d_kds = nullptr;						/* (no chunk) */
	else if (req.kds_dev)
		out->d_kds = req.kds_dev->devptr;
	else
	{
		size_t	kds_len = req.kds->length;
		if (req.kds->format == KDS_FORMAT_ROW)
			kds_len = KERN_DATA_STORE_ROWBLOCK_OFFSET(req.kds) + (size_t)BLCKSZ * req.kds->nblocks;
		void   *p = dev->pool.alloc(kds_len);
		if (!p)
		{
			task_fail(task, StromError_OutOfMemory);
			return false;
		}
		task->devbufs.push_back(p);
		REQ_CHECK_OR(hipMemcpyAsync(p, req.kds, kds_len, hipMemcpyHostToDevice, task->stream),
					 "send kern_data_store", false);
		task->pfm.num_dma_send++;
		task->pfm.bytes_dma_send += kds_len;
		out->d_kds = p;
	}
	out->d_rowmap = (req.rowmap_dev ? req.rowmap_dev->devptr : nullptr);
	if (!req.rowmap_dev && req.krowmap)
	{
		size_t	len = offsetof(kern_row_map, rindex) + sizeof(cl_int) * (size_t)req.krowmap->nvalids;
		void   *p = dev->pool.alloc(len);
		if (!p)
		{
			task_fail(task, StromError_OutOfMemory);
			return false;
		}
		task->devbufs.push_back(p);
		REQ_CHECK_OR(hipMemcpyAsync(p, req.krowmap, len, hipMemcpyHostToDevice, task->stream),
					 "send kern_row_map", false);
		out->d_rowmap = p;
	}
	return true;
}

/* launch step D -- queue the fold behind the request head, the merge check and the merge behind the fold,
 * and the status read-back; the session's launch_lock is held.  False: the task has failed. */
bool
queue_fold_and_merge(strom_task_impl *task, const preagg_request &req, Program *prog, bool checked,
					 const fold_plan &plan, const sent_request &sent, const void *d_jmap,
					 bool piped, hipStream_t s_in, hipStream_t s_mrg)
{
	strom_gpupreagg *sess = req.sess;
	Device	   *dev = task->dev;
	strom_gpupreagg::packed_geom *packed = plan.packed;

	/* this request's slab buffer; whoever read it last must be through */
	unsigned	turn = (sess->slab_turn++ & 1);
	for (int b = 0; b < 2; b++)
		if (!sess->merge_ev[b] &&
			hipEventCreateWithFlags(&sess->merge_ev[b], hipEventDisableTiming) != hipSuccess)
		{
			task_fail(task, StromError_HipInternal);
			return false;
		}
	if (piped)
	{
		hipEvent_t sent_ev = task_event(task, s_in);		/* ev[1]: head is down */
		REQ_CHECK_OR(hipStreamWaitEvent(task->stream, sent_ev, 0), "wait for the request head", false);
	}
	else
		task_event(task);									/* ev[1] */
	if (sess->merge_ev_used[turn])
		REQ_CHECK_OR(hipStreamWaitEvent(task->stream, sess->merge_ev[turn], 0), "wait for the slab buffer", false);
	/* piped: the fold kernel carries its own start / stop events (see task_event_slot) */
	bool		ext_launch = (piped && use_ext_launch());
	hipEvent_t	ev_fold_begin = nullptr, ev_fold_done = nullptr;
	if (piped)
	{
		ev_fold_begin = (ext_launch ? task_event_slot(task) : task_event(task));	/* ev[2]: the fold begins */
		if (ext_launch)
			ev_fold_done = task_event_slot(task);			/* ev[3] */
		if (ext_launch && (!ev_fold_begin || !ev_fold_done))
		{
			task_fail(task, StromError_HipInternal);
			return false;
		}
	}
	void	   *a_kg = sent.d_kg;
	const void *a_kds = sent.d_kds;
	const void *a_toast = nullptr;
	const void *a_map = sent.d_rowmap;
	const gpupreagg_dense_ctl &lctl = (packed ? packed->ctl : sess->ctl);		/* this launch's geometry */
	void	   *a_ctl = (packed ? packed->d_ctl : sess->d_ctl);
	void	   *a_slabs = (packed ? packed->d_slabs : sess->d_slabs) +
		(size_t)turn * lctl.nslabs * lctl.slab_bytes;
	void	   *a_table = sess->table;
	const void *a_res = req.joined_results;
	const void *a_jmap = d_jmap;
	const void *a_pack = sent.d_kg + sent.kg_len;
	/* the fold kernels' parameters, every kind's in this one order: kg, [result pairs,] kds,
	 * [toast, row map,] [column mapping,] ctl, [pack ctl,] slabs; the unmatched pass has no kds */
	void	   *fold_args[8];
	int			na = 0;
	fold_args[na++] = &a_kg;
	if (req.kind == PREAGG_JOINED)
		fold_args[na++] = &a_res;
	if (req.kind != PREAGG_UNMATCHED)
		fold_args[na++] = &a_kds;
	if (req.kind == PREAGG_PLAIN && !plan.use_column)
	{
		fold_args[na++] = &a_toast;
		fold_args[na++] = &a_map;
	}
	if (req.kind != PREAGG_PLAIN)
		fold_args[na++] = &a_jmap;
	fold_args[na++] = &a_ctl;
	if (packed)
		fold_args[na++] = &a_pack;
	fold_args[na++] = &a_slabs;
	void	   *args_mrg[] = { &a_kg, &a_ctl, &a_slabs, &a_table };
	unsigned	fold_block = (plan.use_reg ? 256 : (unsigned)sess->block);
	unsigned	fold_lds = (unsigned)(packed ? packed->lds_bytes : sess->lds_bytes);
	if (ext_launch)
		REQ_CHECK_OR(hipExtModuleLaunchKernel(plan.fn, lctl.nslabs * fold_block, 1, 1, fold_block, 1, 1, fold_lds,
											  task->stream, fold_args, nullptr, ev_fold_begin, ev_fold_done, 0),
					 "launch gpupreagg reduction", false);
	else
		REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn, lctl.nslabs, 1, 1, fold_block, 1, 1, fold_lds, task->stream,
										   fold_args, nullptr),
					 "launch gpupreagg reduction", false);
	if (packed)
		task->pfm.num_kern_prep++;			/* (reported: this request took the packed path) */
	hipEvent_t fold_done = ev_fold_done;
	if (!ext_launch && (task->pfm.enabled || piped))
	{
		fold_done = task_event(task);				/* ev[2] (piped: ev[3]): main kernel done */
		task->has_ev_proj = !piped;
	}
	if (piped)
	{
		/* the merge stream takes over: behind this fold and behind the previous merge */
		if (!fold_done)
		{
			task_fail(task, StromError_HipInternal);
			return false;
		}
		REQ_CHECK_OR(hipStreamWaitEvent(s_mrg, fold_done, 0), "merge waits for the fold", false);
	}
	if (sess->merge_ev_used[turn ^ 1])
		REQ_CHECK_OR(hipStreamWaitEvent(s_mrg, sess->merge_ev[turn ^ 1], 0), "merge waits for the previous merge", false);
	/* the merge kernel lays 256 threads out as GL group lanes x stripes
	 * over the slabs (strom_gpupreagg.h) */
	unsigned ws = 1, per_split = lctl.nslabs / lctl.nsplits;
	while (ws < 64 && ws * 8 < per_split)
		ws <<= 1;
	if (lctl.merge_ws != 0)
		ws = lctl.merge_ws;
	unsigned gl = 256 / ws;
	unsigned mgrid = std::min<unsigned>((lctl.ngroups + gl - 1) / gl,
										(unsigned)dev->prop.multiProcessorCount * 8);
	/* the slab check: numeric sums; integer sums whose chunk totals the range proof may
	 * not cover (tier 2: the kernel leaves at once when it does) */
	if (sess->numeric_aggs || checked ||
		(sess->nintsums > 0 && (sess->sums_measured || sess->static_magbits > 31)))
	{
		/* numeric sums may leave the 64-bit form while slabs are added up: find
		 * out BEFORE the table takes any of it (gpupreagg_dense_merge_body<CHECK>) */
		int		e3 = 0;
		hipFunction_t fn_check = prog->get_function(dev, "gpupreagg_dense_merge_check", &e3);
		if (!fn_check)
		{
			task_fail(task, e3);
			return false;
		}
		REQ_CHECK_OR(hipModuleLaunchKernel(fn_check, std::max(1u, mgrid), 1, 1, 256, 1, 1, 0,
										   s_mrg, args_mrg, nullptr),
					 "launch gpupreagg merge check", false);
		task->pfm.num_kern_exec++;
	}
	REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn_merge, std::max(1u, mgrid), 1, 1, 256, 1, 1, 0,
									   s_mrg, args_mrg, nullptr),
				 "launch gpupreagg merge", false);
	task->pfm.num_kern_exec += 2;
	REQ_CHECK_OR(hipEventRecord(sess->merge_ev[turn], s_mrg), "mark the merge", false);
	sess->merge_ev_used[turn] = true;
	task_event(task, s_mrg);							/* ev[2] (+1 with the fold event; piped: ev[4]) */
	REQ_CHECK_OR(hipMemcpyAsync(sent.stage + sent.send_len, sent.d_kg + offsetof(kern_gpupreagg, status), sizeof(cl_int),
								hipMemcpyDeviceToHost, s_mrg),
				 "recv status", false);
	task->pfm.num_dma_recv++;
	task->pfm.bytes_dma_recv += sizeof(cl_int);
	task_event(task, s_mrg);							/* ev[3] (+1; piped: ev[5]) */
	task->ev_preagg_piped = piped;
	return true;
}

void
gpupreagg_launch(strom_task_impl *task, preagg_request req, bool checked = false)
{
	strom_gpupreagg *sess = req.sess;
	Device	   *dev = task->dev;
	/* (a lookup, a star and a checked retry bring their program: lookup_mapping_program,
	 * star_mapping_program, checked_program) */
	Program	   *prog = (req.prog ? req.prog : sess->prog);

	(void)hipSetDevice(dev->hip_id);
	if (req.joined_buffer && !checked)
		task->devbufs.push_back(req.joined_buffer);		/* released with this task, whatever happens */
	if (prog->state != STROM_DEVPROG_READY)
	{
		task_fail(task, StromError_ProgramBuildFailure);
		return;
	}
	task->pfm.time_kern_build = (cl_ulong)prog->build_usec;
	/* chunks fold into one table: keep them in order on one stream */
	task->stream = dev->streams[0];
	/*
	 * resident chunk: no bulk DMA, so the small copies and the slab merge leave
	 * the fold stream -- the request head goes down on copy_in, the merge of
	 * chunk k (and its status read-back) runs on merge_stream while chunk k+1 is
	 * folded.  Measured for C4 (1e9 rows in 10 chunks): 317 us of wall clock per
	 * chunk with everything on one stream, of which 250 us are the fold kernel.
	 */
	bool		piped = (req.kds_dev != nullptr && dev->copy_in && dev->merge_stream &&
						 !getenv("STROM_GPUPREAGG_NO_PIPE"));
	hipStream_t	s_in = (piped ? dev->copy_in : task->stream);
	hipStream_t	s_mrg = (piped ? dev->merge_stream : task->stream);
	/* one launch at a time per session: the slab turn and the event chain are ordered */
	std::lock_guard<std::mutex> launch_guard(sess->launch_lock);

	fold_plan	plan;
	int			errcode = plan_fold(dev, prog, req, checked, &plan);
	if (errcode != 0)
	{
		task_fail(task, errcode);
		return;
	}
	sent_request sent;
	if (!send_request(task, req, s_in, plan.magbits, plan.wg_rows, plan.zone_bounded,
					  plan.packed ? &plan.pk : nullptr, &sent))
		return;
	void   *d_jmap = nullptr;
	if (req.kind != PREAGG_PLAIN)
	{
		d_jmap = dev->pool.alloc(req.map->size());
		if (!d_jmap)
		{
			task_fail(task, StromError_OutOfMemory);
			return;
		}
		task->devbufs.push_back(d_jmap);
		/* small and pageable: a synchronous copy keeps the source alive */
		REQ_CHECK(hipMemcpy(d_jmap, req.map->data(), req.map->size(), hipMemcpyHostToDevice),
				  "send joined map");
	}
	if (!queue_fold_and_merge(task, req, prog, checked, plan, sent, d_jmap, piped, s_in, s_mrg))
		return;
	if (checked)
		sess->checked_folds++;
	char   *stage_status = sent.stage + sent.send_len;
	task->finish = [stage_status, req, checked](strom_task_impl *t)
	{
		cl_int status;
		memcpy(&status, stage_status, sizeof(status));
		if (status == StromError_SumRangeUnproven && !checked)
		{
			/*
			 * the merge could not prove that the chunk's integer sums stay in int8 and left
			 * the table alone: the chunk is folded again by the checked program (on a worker
			 * thread: the program may have to be built first), and this request completes
			 * when that is through
			 */
			t->retry = [t, req]()
			{
				preagg_request again = req;
				again.prog = checked_program(req);
				if (!again.prog)
				{
					task_fail(t, StromError_OutOfMemory);
					return;
				}
				program_run_or_park(again.prog, [t, again]() { gpupreagg_launch(t, again, true); });
			};
			return;
		}
		if (status == StromError_SumRangeUnproven)
			status = StromError_CpuReCheck;		/* (not reached: the checked merge has no proof to fail) */
		t->errcode = status;		/* 0, CpuReCheck, or significant */
	};
	task_enqueue(task);
}


/* ------------------------------------------------------------------ *
 * hashed GROUP BY (gpupreagg_hash_* of strom_gpupreagg.h)
 * ------------------------------------------------------------------ */

/* what a fold reads back of the head: capacity, nkeys and the two counters the kernels raise */
const size_t HASH_HEAD_COUNTERS = offsetof(gpupreagg_hash_head, stride);

/* the head of a table of 'capacity' slots as the host writes it (strom_ctl.h), and the table's bytes */
gpupreagg_hash_head
hash_table_head(const strom_gpupreagg *sess, cl_uint capacity, size_t *p_total)
{
	gpupreagg_hash_head head = {};
	size_t		nkeys = sess->key_resno.size(), naggs = sess->agg_resno.size();

	head.capacity = capacity;
	head.nkeys = (cl_uint)nkeys;
	head.stride = (cl_uint)GPUPREAGG_HASH_STRIDE_OF(nkeys, naggs);
	head.naggs = (cl_uint)naggs;
	*p_total = GPUPREAGG_HASH_HEAD + (size_t)head.stride * capacity;
	return head;
}

/* launch step A -- the STROM_GPUPREAGG_HASH_* knobs (README), read on every call: tests change the
 * environment between two folds of one process.  A value that fails its reader's test is ignored. */
struct hashed_knobs {
	cl_uint		lds_slots, roles, parts, unit_rows, scatter_rows;		/* 0: not set */
	unsigned	scatter_block, fold_block;								/* 0: not set */
	unsigned	check_block, check_per_cu, unit_lds_kb;
	cl_ulong	parts_min;
	cl_ulong	fill_num, fill_den;	/* the part of a role's LDS table its share of the groups may fill */
	bool		lds_64kb, no_rolemap, no_parts, no_lds_scatter, no_exact;
};

/* a power of two within lo ... hi (a work-group size: 256, 512 or 1024), or dflt */
cl_uint
knob_pow2(const char *name, int lo, int hi, cl_uint dflt)
{
	const char *v = getenv(name);
	int		want = (v ? atoi(v) : 0);
	return (want >= lo && want <= hi && (want & (want - 1)) == 0) ? (cl_uint)want : dflt;
}
/* an integer, raised to 'lo' where it is below; dflt when the knob is not set */
int
knob_at_least(const char *name, int lo, int dflt)
{
	const char *v = getenv(name);
	return v ? std::max(lo, atoi(v)) : dflt;
}

hashed_knobs
read_hashed_knobs()
{
	hashed_knobs k;
	const char *kb = getenv("STROM_GPUPREAGG_HASH_LDS_KB"), *fill = getenv("STROM_GPUPREAGG_HASH_FILL");
	const char *parts_min = getenv("STROM_GPUPREAGG_HASH_PARTS_MIN");
	/* tests: a tiny table in front of the global one sends (nearly) every row to the global
	 * table's claim / probe protocol */
	k.lds_slots = knob_pow2("STROM_GPUPREAGG_HASH_LDS_SLOTS", 64, 16384, 0);
	k.lds_64kb = (kb && atol(kb) <= 64);
	k.unit_lds_kb = (cl_uint)std::min(159, knob_at_least("STROM_GPUPREAGG_HASH_UNIT_LDS_KB", 8, 159));
	k.roles = knob_pow2("STROM_GPUPREAGG_HASH_ROLES", 1, 64, 0);	/* 1, 2, 4 ... 64; anything else would break the tile walk */
	k.fill_num = (fill ? (cl_ulong)atoi(fill) : 5);		/* 64 probes find room at 5/8 */
	k.fill_den = (fill ? 100 : 8);
	k.no_rolemap = (getenv("STROM_GPUPREAGG_HASH_NO_ROLEMAP") != nullptr);
	k.parts_min = (parts_min ? strtoul(parts_min, nullptr, 10) : 10000);
	k.no_parts = (getenv("STROM_GPUPREAGG_HASH_NO_PARTS") != nullptr);
	k.parts = knob_pow2("STROM_GPUPREAGG_HASH_PARTS", 64, 4096, 0);
	k.unit_rows = (cl_uint)knob_at_least("STROM_GPUPREAGG_HASH_UNIT_ROWS", 1024, 0);
	/* (1024 threads, two work-groups per CU: 2.37 against 2.48 ms for the whole plan with 256 x 4,
	 * the other combinations in between -- scripts/hashed_check_sweep.sh) */
	k.check_block = knob_pow2("STROM_GPUPREAGG_HASH_CHECK_BLOCK", 256, 1024, 1024);
	k.check_per_cu = (unsigned)knob_at_least("STROM_GPUPREAGG_HASH_CHECK_PER_CU", 1, 2);
	k.scatter_block = knob_pow2("STROM_GPUPREAGG_HASH_SCATTER_BLOCK", 256, 1024, 0);
	k.fold_block = knob_pow2("STROM_GPUPREAGG_HASH_FOLD_BLOCK", 256, 1024, 0);
	k.no_lds_scatter = (getenv("STROM_GPUPREAGG_HASH_NO_LDS_SCATTER") != nullptr);
	k.scatter_rows = (cl_uint)knob_at_least("STROM_GPUPREAGG_HASH_SCATTER_ROWS", 1, 0);
	k.no_exact = (getenv("STROM_GPUPREAGG_HASH_NO_EXACT") != nullptr);
	return k;
}

/* slots of the work-group's LDS table in front of the global one, and its bytes */
cl_uint
hash_lds_slots(const strom_gpupreagg *sess, const hashed_knobs &knobs, size_t *p_bytes, bool for_units = false)
{
	size_t		nkeys = sess->key_resno.size();
	/* after the table: GPUPREAGG_HASH_QUEUE queued row numbers per wave (used with roles) */
	size_t		queue = (for_units ? 16 /* the unit's flags */ : ((size_t)sess->block / 64) * GPUPREAGG_HASH_QUEUE * sizeof(cl_uint));
	auto bytes_of = [&](cl_uint slots) -> size_t {
		return sess->image_offset(sess->nsections(), slots, 1) + (size_t)slots * GPUPREAGG_HASH_LDS_ENTRY(nkeys) + queue;
	};
	/*
	 * LDS per work-group: ONE work-group per CU with a table of up to 136 KB, four times the
	 * slots of the 64 KB table two work-groups per CU had.  Every doubling of the table halves
	 * the hash roles, and each role is a scan of every row's key columns: 1e4 groups 5.1 ->
	 * 3.4 ms per 1e8 rows, 3e4 groups 13.2 -> 7.1 ms; a fuller small table also probes longer,
	 * so the big one wins from 100 groups on (698 -> 656 us; 600 groups 1463 -> 932 us).
	 * profiles/r02_hashed_lds_tables.txt
	 * The partition plan's units: no role queues, and as much of the CU's 160 KB as a power of
	 * two of slots takes.
	 */
	size_t		budget = (size_t)(for_units ? knobs.unit_lds_kb : knobs.lds_64kb ? 64 : 136) * 1024;
	cl_uint		slots = 16384;
	if (!for_units && knobs.lds_slots)
		slots = knobs.lds_slots;			/* (as asked for, whatever it takes) */
	else
		while (bytes_of(slots) > budget && slots > 64)
			slots >>= 1;
	*p_bytes = bytes_of(slots);
	return slots;
}

/* a zeroed, initialised table of 'capacity' slots on the session's stream */
int
hash_table_new(strom_gpupreagg *sess, cl_uint capacity, char **p_tab, size_t *p_bytes, char *reuse)
{
	Device	   *dev = sess->dev;
	hipStream_t	stream = dev->streams[0];
	size_t		total = 0;
	gpupreagg_hash_head head = hash_table_head(sess, capacity, &total);
	int			errcode = 0;
	hipFunction_t fn_init = sess->prog->get_function(dev, "gpupreagg_hash_init", &errcode);
	if (!fn_init)
		return errcode;
	char   *tab = (reuse ? reuse : (char *)dev->pool.alloc(total));
	if (!tab)
		return StromError_OutOfMemory;
	/* the head is tiny: a synchronous copy from pageable memory is fine and keeps
	 * the source alive */
	if (hipMemsetAsync(tab, 0, total, stream) != hipSuccess ||
		hipStreamSynchronize(stream) != hipSuccess ||
		hipMemcpy(tab, &head, sizeof(head), hipMemcpyHostToDevice) != hipSuccess)
	{
		if (!reuse) dev->pool.release(tab);
		return StromError_HipInternal;
	}
	void   *a_tab = tab;
	void   *args[] = { &a_tab };
	unsigned grid = std::max(1u, std::min<unsigned>((capacity + 255) / 256,
													(unsigned)dev->prop.multiProcessorCount * 8));
	if (hipModuleLaunchKernel(fn_init, grid, 1, 1, 256, 1, 1, 0, stream, args, nullptr) != hipSuccess)
	{
		if (!reuse) dev->pool.release(tab);
		return StromError_HipInternal;
	}
	*p_tab = tab;
	*p_bytes = total;
	return 0;
}

/* groups the table takes before it must grow: 7/8 of the slots minus what racing threads and
 * the work-groups' final LDS flushes can still claim (never negative: a table made by an
 * import may be smaller than a fold's headroom -- the fold grows it first, see the callers) */
cl_ulong
hash_fill_limit(const strom_gpupreagg *sess, cl_ulong headroom)
{
	cl_ulong	room = (cl_ulong)sess->hash_capacity / 8 * 7;
	return room > headroom ? room - headroom : 0;
}

/* groups claimed so far (drains the session's stream) */
int
hash_table_ngroups(strom_gpupreagg *sess, cl_uint *p_ngroups, cl_uint *p_overflow)
{
	gpupreagg_hash_head head;
	if (hipStreamSynchronize(sess->dev->streams[0]) != hipSuccess ||
		hipMemcpy(&head, sess->htab, HASH_HEAD_COUNTERS, hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_HipInternal;
	*p_ngroups = head.ngroups;
	sess->groups_known = std::max<cl_uint>(sess->groups_known, head.ngroups);
	if (p_overflow)
		*p_overflow = head.overflow;
	return 0;
}

/*
 * a table of at least min_capacity slots, the groups of the current one
 * re-inserted by gpupreagg_hash_rehash (drains the stream)
 */
int
hash_table_grow(strom_gpupreagg *sess, cl_ulong min_capacity)
{
	Device	   *dev = sess->dev;
	cl_ulong	capacity = sess->hash_capacity;
	cl_uint		ngroups = 0;
	int			rc = hash_table_ngroups(sess, &ngroups, nullptr);

	if (rc)
		return rc;
	while (capacity < min_capacity)
		capacity <<= 1;
	if (capacity > (1UL << 31))
		return StromError_DataStoreNoSpace;
	if (capacity == sess->hash_capacity)
		return 0;
	char	   *ntab = nullptr;
	size_t		nbytes = 0;
	rc = hash_table_new(sess, (cl_uint)capacity, &ntab, &nbytes, nullptr);
	if (rc)
		return rc;
	if (ngroups > 0)
	{
		int		errcode = 0;
		hipFunction_t fn = sess->prog->get_function(dev, "gpupreagg_hash_rehash", &errcode);
		const void *a_old = sess->htab;
		void	   *a_new = ntab;
		void	   *args[] = { &a_old, &a_new };
		unsigned	grid = std::min<unsigned>((sess->hash_capacity + 255) / 256,
											  (unsigned)dev->prop.multiProcessorCount * 8);
		if (!fn ||
			hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, dev->streams[0], args, nullptr) != hipSuccess ||
			hipStreamSynchronize(dev->streams[0]) != hipSuccess)
		{
			dev->pool.release(ntab);
			return fn ? StromError_HipInternal : errcode;
		}
	}
	dev->pool.release(sess->htab);
	sess->htab = ntab;
	sess->htab_bytes = nbytes;
	sess->hash_capacity = (cl_uint)capacity;
	sess->groups_upper = ngroups;
	return 0;
}

/*
 * the bound of the table's integer sums restarts from what the table really holds
 * (gpupreagg_hash_sum_refresh; queued on the session's stream, sess->lock held)
 */
int
hash_sum_refresh(strom_gpupreagg *sess)
{
	Device	   *dev = sess->dev;
	int			errcode = 0;
	if (sess->nintsums == 0 || !sess->htab)
		return 0;
	hipFunction_t fn = sess->prog->get_function(dev, "gpupreagg_hash_sum_refresh", &errcode);
	if (!fn)
		return errcode;
	void	   *a_tab = sess->htab;
	void	   *args[] = { &a_tab };
	unsigned	grid = std::max(1u, std::min<unsigned>((sess->hash_capacity + 255) / 256,
													(unsigned)dev->prop.multiProcessorCount * 8));
	if (hipMemsetAsync(sess->htab + offsetof(gpupreagg_hash_head, sum_bound), 0, sizeof(gpupreagg_hash_head::sum_bound),
					   dev->streams[0]) != hipSuccess ||
		hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, dev->streams[0], args, nullptr) != hipSuccess)
		return StromError_HipInternal;
	return 0;
}

/*
 * the largest |integer sum| the table holds, plus one (0: no integer sums, or an empty table):
 * measured by hash_sum_refresh, read back.  sess->lock held.
 */
int
hash_sum_measured_bound(strom_gpupreagg *sess, cl_ulong *p_bound)
{
	*p_bound = 0;
	if (sess->nintsums == 0 || !sess->htab)
		return 0;
	int		rc = hash_sum_refresh(sess);
	if (rc)
		return rc;
	if (hipStreamSynchronize(sess->dev->streams[0]) != hipSuccess ||
		hipMemcpy(p_bound, sess->htab + offsetof(gpupreagg_hash_head, sum_bound), sizeof(cl_ulong), hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_HipInternal;
	return 0;
}

void gpupreagg_launch_hashed(strom_task_impl *task, preagg_request req, bool second = false);
/*
 * The exact fold of a hashed session ("integer sums never wrap", strom_gpupreagg.h).  The running
 * bound of a hashed table -- rows x largest input magnitude, over all groups at once -- can fail
 * although no group comes near the edge (2e6 rows of 1e13 in a thousand groups).  Such a chunk is
 * folded into a SCRATCH session of the same targets whose program is built with GPUPREAGG_CHECKED
 * (every LDS and table addition returns what it was added to and is checked, the reference's
 * CHECK_OVERFLOW_INT on every accumulate, opencl_gpupreagg.h:142-143): an addition that leaves int8
 * inside the chunk is CpuReCheck and the session's table has not been touched.  Then the scratch
 * groups join the table: a read-only pass checks every group that exists on both sides
 * (gpupreagg_hash_import_verify), and only when all fit are they imported.  Exact, or CpuReCheck
 * with the table as it was.  Rare and slower (a second table, one more pass): the price is paid by
 * the chunks that need it.  The scratch session lives for the request (strom_task_impl::at_complete).
 */
void
gpupreagg_hashed_exact(strom_task_impl *task, preagg_request req)
{
	int		errcode = 0;
	strom_gpupreagg *child = gpupreagg_exact_child(req.sess, &errcode);
	if (!child)
	{
		task_fail(task, errcode ? errcode : StromError_OutOfMemory);
		return;
	}
	task->at_complete.push_back([child]() { strom_gpupreagg_release(child); });
	req.sess->checked_folds++;
	preagg_request creq = req;
	creq.exact_parent = req.sess;
	creq.sess = child;
	program_run_or_park(child->prog, [task, creq]() { gpupreagg_launch_hashed(task, creq, false); });
}

void
gpupreagg_hashed_exact_merge(strom_task_impl *task, preagg_request req)
{
	strom_gpupreagg *child = req.sess, *parent = req.exact_parent;
	char	   *d_recs = nullptr;
	cl_uint		count = 0;
	size_t		reclen = 0;
	int			rc = gpupreagg_hash_export_device(child, &d_recs, &count, &reclen);
	if (rc == 0 && count > 0)
		rc = gpupreagg_hash_import_device(parent, d_recs, count, 1, &count, ~0u, GPUPREAGG_IMPORT_EXACT);
	gpupreagg_hash_release(child, d_recs);
	if (rc != 0 && rc != StromError_CpuReCheck)
	{
		task_fail(task, rc);
		return;
	}
	task->finish = [rc](strom_task_impl *t) { t->errcode = rc; };
	task_enqueue(task);
}

/* launch step B -- how this request is folded: by hash roles or by the partition plan, and every kernel's
 * geometry.  Host arithmetic and get_function only.  The roles' LDS table and the units' have their own fields. */
struct hashed_plan {
	/* plan_role_table: the roles' kernels and their table; 'block' is the session's work-group size */
	hipFunction_t fn_check = nullptr, fn_fold = nullptr;
	unsigned	block = 0, role_fold_grid = 0;
	cl_uint		role_lds_slots = 0;
	size_t		role_lds_bytes = 0;
	/* free slots a fold needs (see plan_role_table).  From the ROLES' figures for both plans: the
	 * partition plan's turns keep this headroom too, not one made of the units' grid and table */
	cl_ulong	headroom = 0;
	/* plan_hashed_fold */
	bool		column_streams = false, use_parts = false;
	/* ... the partition plan: check, part_plan, scatter (lds_rows 0: the direct one), fold of the units */
	hipFunction_t fn_pcheck = nullptr, fn_plan = nullptr, fn_scatter = nullptr, fn_units = nullptr;
	cl_uint		nparts = 0, max_units = 0, lds_rows = 0, unit_lds_slots = 0;
	size_t		reclen = 0, scatter_lds_bytes = 0, unit_lds_bytes = 0;
	gpupreagg_part_ctl ctl_img = {};
	unsigned	check_block = 0, check_grid = 0, scatter_block = 0, scatter_grid = 0, unit_fold_grid = 0, unit_fold_block = 0;
};

/*
 * geometry of the roles' fold: two work-groups per CU (64 KB of LDS each), or one with the large
 * table.  Slots can be claimed past the fill limit by threads that raced through the limit test
 * (one each at most) and by the work-groups' final LDS flushes: that much headroom, and an
 * eighth of the table on top, always stays free.
 */
int
plan_role_table(Device *dev, Program *prog, strom_gpupreagg *sess, const hashed_knobs &knobs, hashed_plan *plan)
{
	int		errcode = 0;
	plan->fn_check = prog->get_function(dev, "gpupreagg_hash_check", &errcode);
	plan->fn_fold = plan->fn_check ? prog->get_function(dev, "gpupreagg_hash_fold", &errcode) : nullptr;
	if (!plan->fn_check || !plan->fn_fold)
		return errcode;
	plan->block = (unsigned)sess->block;
	plan->role_lds_slots = hash_lds_slots(sess, knobs, &plan->role_lds_bytes);
	plan->role_fold_grid = (unsigned)dev->prop.multiProcessorCount * (plan->role_lds_bytes <= 72 * 1024 ? 2 : 1);
	plan->headroom = (cl_ulong)plan->role_fold_grid * plan->block + (cl_ulong)plan->role_fold_grid * plan->role_lds_slots;
	return 0;
}

/* the rest of the plan.  It reads the table's capacity and the groups known: the table stands by now */
int
plan_hashed_fold(Device *dev, Program *prog, const preagg_request &req, const hashed_knobs &knobs, hashed_plan *plan)
{
	strom_gpupreagg *sess = req.sess;
	cl_uint		nrows = req.nrows;
	unsigned	ncus = (unsigned)dev->prop.multiProcessorCount, block = plan->block;
	int			errcode = 0;

	/* hash roles, the role map and the partition plan scan a COLUMN chunk's arrays as they are: not
	 * for a program with text / character(n) variables (their column holds offsets that each row
	 * turns into an address -- strom_kvars_from_column, the one-role walk does it) */
	plan->column_streams = (req.format == KDS_FORMAT_COLUMN && !(prog->extra_flags & DEVTYPE_IS_VARLENA));
	/*
	 * More groups than the hash roles' LDS tables take together (or than a few roles, each a
	 * scan of the chunk, are worth): the chunk is ordered by hash partition first and folded
	 * unit by unit (strom_gpupreagg.h: gpupreagg_hash_check_parts ... _fold_parts).  1e8 rows,
	 * 1e5 / 1e6 groups: 23 / 42 ms through the global table; profiles/r02_hashed_partitions.txt
	 */
	/* nothing known about the group count yet (no hint, first chunk; every chunk of the stateless
	 * per-chunk message): a large chunk takes the plan whose cost does not depend on it -- 2.6 ms
	 * per 1e8 rows whatever the count, against 0.7 ... 14 ms through the LDS table and the global one */
	bool		unknown = (sess->groups_known == 0 && nrows >= (4u << 20));
	plan->use_parts = (nrows > 0 && ((cl_ulong)sess->groups_known >= knobs.parts_min || (unknown && knobs.parts_min > 0)) &&
					   !knobs.no_parts);
	if (!plan->use_parts)
		return 0;
	plan->fn_pcheck = prog->get_function(dev, "gpupreagg_hash_check_parts", &errcode);
	plan->fn_plan = plan->fn_pcheck ? prog->get_function(dev, "gpupreagg_hash_part_plan", &errcode) : nullptr;
	hipFunction_t fn_scatter = plan->fn_plan ? prog->get_function(dev, "gpupreagg_hash_scatter", &errcode) : nullptr;
	hipFunction_t fn_scatter_lds = fn_scatter ? prog->get_function(dev, "gpupreagg_hash_scatter_lds", &errcode) : nullptr;
	plan->fn_units = fn_scatter_lds ? prog->get_function(dev, "gpupreagg_hash_fold_parts", &errcode) : nullptr;
	if (!plan->fn_units)
		return errcode;
	/* the units' LDS table: no role queues, one work-group per CU unless two tables fit */
	plan->unit_lds_slots = hash_lds_slots(sess, knobs, &plan->unit_lds_bytes, true);
	plan->unit_fold_grid = ncus * (plan->unit_lds_bytes <= 79 * 1024 ? 2 : 1);
	/*
	 * its size in threads is the CU's whole occupancy, so the full GPUPREAGG_BLOCK (1024: four waves
	 * per SIMD).  Smaller work-groups are slower all the way: 256 / 512 / 1024 threads fold 1e8 rows
	 * at 1e6 groups in 7.0 / 4.1 / 3.2 ms, and the LDS scatter likewise (profiles/r03_hashed_block_sweep.txt).
	 */
	plan->unit_fold_block = (knobs.fold_block && knobs.fold_block <= block ? knobs.fold_block : block);
	/*
	 * partitions: as few as keep a partition's groups within 5/8 of a unit's LDS table --
	 * the fewer, the longer the runs the scatter writes (a tile of ~4096 rows leaves in
	 * runs of 4096 / nparts records)
	 */
	cl_uint		nparts = 256;
	cl_ulong	per_unit = (cl_ulong)plan->unit_lds_slots * 5 / 8;
	while (nparts < 4096 && (cl_ulong)sess->groups_known > (cl_ulong)nparts * per_unit)
		nparts <<= 1;
	if (knobs.parts)
		nparts = knobs.parts;
	/* a unit is a whole partition unless the partition is four times the average (one
	 * heavy key must not be one work-group's job): every unit ends in a flush of its
	 * groups to the global table, the fewer the better */
	cl_uint		unit_rows = std::max<cl_uint>(32768, (cl_uint)std::min<cl_ulong>(1u << 30, 4 * (cl_ulong)nrows / nparts));
	if (knobs.unit_rows)
		unit_rows = knobs.unit_rows;
	int			log2cap = bits_for(sess->hash_capacity) - 1, log2parts = bits_for(nparts) - 1;
	size_t		nvals = 0;
	for (int resno : sess->agg_resno)
		nvals += (sess->targets[resno].kind != STROM_PREAGG_NROWS ? 1 : 0);
	size_t		reclen = plan->reclen = 8 * (1 + sess->key_resno.size() + nvals);
	plan->nparts = nparts;
	plan->max_units = nparts + nrows / unit_rows + 1;
	plan->ctl_img = { nparts, (cl_uint)(log2cap > log2parts ? log2cap - log2parts : 0), unit_rows, 0, 0, 0, plan->max_units, (cl_uint)reclen };
	plan->check_block = knobs.check_block;
	plan->check_grid = std::max(1u, std::min<unsigned>((nrows + 2 * knobs.check_block - 1) / (2 * knobs.check_block),
													   ncus * knobs.check_per_cu));
	/* the scatter goes through LDS (records leave in runs) when a tile of at least one row
	 * per thread fits next to the partitions' counters */
	size_t		stage_fixed = 12 * (size_t)nparts + 128, stage_budget = 159 * 1024;
	unsigned	sblock = (knobs.scatter_block && knobs.scatter_block <= block ? knobs.scatter_block : block);
	if (nparts <= 4 * sblock && stage_fixed < stage_budget && !knobs.no_lds_scatter)
		plan->lds_rows = (cl_uint)std::min<size_t>(4, (stage_budget - stage_fixed) / ((reclen + 2) * sblock));
	if (knobs.scatter_rows)
		plan->lds_rows = std::min(plan->lds_rows, knobs.scatter_rows);
	bool		lds = (plan->lds_rows > 0);
	size_t		tile = (lds ? (size_t)sblock * plan->lds_rows : (size_t)block * 32);
	plan->fn_scatter = (lds ? fn_scatter_lds : fn_scatter);
	plan->scatter_block = (lds ? sblock : block);
	plan->scatter_lds_bytes = (lds ? stage_fixed + tile * (reclen + 2) : 0);
	plan->scatter_grid = (unsigned)std::max<size_t>(1, std::min<size_t>((nrows + tile - 1) / tile,
																		 (size_t)ncus * (plan->scatter_lds_bytes <= 72 * 1024 ? 2 : 1)));
	return 0;
}

/* the table a fold needs: made, or grown when a merge / import made it before the first fold
 * (at the session's initial size): 'min_capacity' slots whatever made the table */
int
hash_table_for_fold(strom_gpupreagg *sess, cl_ulong min_capacity)
{
	if (sess->htab)
		return ((cl_ulong)sess->hash_capacity < min_capacity ? hash_table_grow(sess, min_capacity) : 0);
	cl_ulong	capacity = sess->hash_capacity;
	while (capacity < min_capacity)
		capacity <<= 1;
	sess->hash_capacity = (cl_uint)capacity;
	return hash_table_new(sess, sess->hash_capacity, &sess->htab, &sess->htab_bytes, nullptr);
}

/*
 * the turns of a fold over 'nrows' rows, both plans: make room for the groups the turn may bring, launch,
 * and when rows (roles) or units (partition plan) were deferred for want of room, wait and go round with
 * them.  While even 'incoming' new groups fit under the fill limit nothing can be deferred and the task
 * stays asynchronous.  launch(turn, carried, claim_limit, a_turn, p_count) queues one turn: 'carried' is
 * what the turn before deferred (0 in turn 0); with p_count it resets the device's count of deferred rows /
 * units before the kernel and says in *p_count where it is: the loop reads it back behind the fold.
 *
 * a_turn is the fold's turn for gpupreagg_hash_sum_account: the parity; 'attempt' is 4 on a second
 * attempt whose failed proof is final; relaunches for deferred work add 2.  The parity advances
 * here, where a fold's first launch is queued, and nowhere else: that launch always writes the slot
 * the next fold reads (gpupreagg_hash_sum_account, or gpupreagg_hash_sum_carry when it folds
 * nothing).  A request that queues no fold -- no rows, a failure on the way -- leaves the slots
 * alone and so must leave the parity alone.
 */
template <typename Launch>
bool
hash_fold_turns(strom_task_impl *task, strom_gpupreagg *sess, cl_ulong headroom, cl_uint nrows,
				bool deferred_are_rows, cl_uint attempt, Launch launch)
{
	cl_uint		sum_turn = (sess->sum_turn & 1u) | attempt, incoming = nrows, carried = 0;

	for (int turn = 0; incoming > 0; turn++)
	{
		cl_ulong	fill_limit = hash_fill_limit(sess, headroom);
		if (sess->groups_upper + incoming > fill_limit)
		{
			/* the bound is stale or the table is small: look */
			cl_uint	ngroups = 0;
			int		rc = hash_table_ngroups(sess, &ngroups, nullptr);
			if (rc == 0)
			{
				sess->groups_upper = ngroups;
				/* (geometric: what was deferred says little about the groups in it) */
				if (turn > 0 || (cl_ulong)ngroups * 2 > fill_limit)
					rc = hash_table_grow(sess, (cl_ulong)sess->hash_capacity * 4);
			}
			if (rc)
			{
				task_fail(task, rc);
				return false;
			}
			fill_limit = hash_fill_limit(sess, headroom);
		}
		bool		may_defer = (sess->groups_upper + incoming > fill_limit);
		cl_uint		claim_limit = (may_defer ? (cl_uint)fill_limit : ~0u), deferred = 0;
		const void *d_count = nullptr;
		if (!launch(turn, carried, claim_limit, sum_turn | (turn > 0 ? 2u : 0u), may_defer ? &d_count : nullptr))
			return false;
		task->pfm.num_kern_exec++;
		if (turn == 0)
			sess->sum_turn++;
		if (!may_defer)
		{
			sess->groups_upper += incoming;
			break;
		}
		REQ_CHECK_OR(hipMemcpyAsync(&deferred, d_count, sizeof(cl_uint), hipMemcpyDeviceToHost, task->stream),
					 "recv the deferred count", false);
		REQ_CHECK_OR(hipStreamSynchronize(task->stream), "hashed fold's turn", false);
		sess->groups_upper = std::min<cl_ulong>(sess->groups_upper + incoming, sess->hash_capacity);
		if (deferred == 0)
			break;
		carried = deferred;
		if (deferred_are_rows)
			incoming = deferred;		/* (units: any of the chunk's rows may still bring a group) */
	}
	return true;
}

/* what every kernel over the chunk begins with: kern_gpupreagg, chunk, toast (none), row map */
struct chunk_args { void *kg; const void *kds, *toast, *map; };

/* launch step D, partition plan -- check, plan, scatter, then the fold, unit by unit.  A unit with a new
 * group beyond the claim limit comes back on the redo list with nothing merged: the table grows and the
 * list is run.  False: the task has failed. */
bool
queue_partition_plan(strom_task_impl *task, const preagg_request &req, const hashed_plan &plan,
					 const sent_request &sent, cl_uint attempt)
{
	strom_gpupreagg *sess = req.sess;
	Device	   *dev = task->dev;
	cl_uint		nrows = req.nrows, nparts = plan.nparts, max_units = plan.max_units;
	/* ctl | hist[P] | cursor[P] | units[2 * max_units] | two redo lists of max_units */
	size_t		ctl_len = sizeof(gpupreagg_part_ctl) + sizeof(cl_uint) * ((size_t)2 * nparts + (size_t)4 * max_units);
	char	   *d_ctl = (char *)dev->pool.alloc(ctl_len);
	char	   *d_partmap = (char *)dev->pool.alloc(STROMALIGN((size_t)nrows * sizeof(cl_ushort)));
	char	   *d_records = (char *)dev->pool.alloc((size_t)nrows * plan.reclen);
	for (char *p : { d_ctl, d_partmap, d_records })
		if (p) task->devbufs.push_back(p);
	if (!d_ctl || !d_partmap || !d_records || sent.kg_len + 128 + sizeof(gpupreagg_part_ctl) > PinnedPool::BLOCK)
	{
		task_fail(task, StromError_OutOfMemory);
		return false;
	}
	char	   *stage_ctl = sent.stage + sent.kg_len + 64;
	memcpy(stage_ctl, &plan.ctl_img, sizeof(plan.ctl_img));
	REQ_CHECK_OR(hipMemsetAsync(d_ctl, 0, sizeof(gpupreagg_part_ctl) + sizeof(cl_uint) * nparts, task->stream),
				 "reset partition counts", false);
	REQ_CHECK_OR(hipMemcpyAsync(d_ctl, stage_ctl, sizeof(gpupreagg_part_ctl), hipMemcpyHostToDevice, task->stream),
				 "send partition plan", false);
	chunk_args	ca = { sent.d_kg, sent.d_kds, nullptr, sent.d_rowmap };
	cl_uint	   *d_words = (cl_uint *)(d_ctl + sizeof(gpupreagg_part_ctl));
	void	   *a_ctl = d_ctl, *a_hist = d_words, *a_cursor = d_words + nparts, *a_units = d_words + (size_t)2 * nparts;
	cl_uint	   *d_lists = d_words + (size_t)2 * nparts + (size_t)2 * max_units;
	void	   *a_partmap = d_partmap, *a_records = d_records;
	cl_uint		lds_rows = plan.lds_rows, unit_lds_slots = plan.unit_lds_slots;
	void	   *args_check[] = { &ca.kg, &ca.kds, &ca.toast, &ca.map, &a_partmap, &a_hist, &a_ctl };
	void	   *args_plan[] = { &a_hist, &a_cursor, &a_units, &a_ctl };
	/* (the LDS scatter's last parameter is its rows per thread; the direct one ends before it) */
	void	   *args_scatter[] = { &ca.kg, &ca.kds, &ca.toast, &ca.map, &a_partmap, &a_cursor, &a_records, &a_ctl, &lds_rows };
	REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn_pcheck, plan.check_grid, 1, 1, plan.check_block, 1, 1, 0, task->stream, args_check, nullptr),
				 "launch gpupreagg hash check (partitions)", false);
	REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn_plan, 1, 1, 1, 256, 1, 1, 0, task->stream, args_plan, nullptr),
				 "launch gpupreagg partition plan", false);
	REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn_scatter, plan.scatter_grid, 1, 1, plan.scatter_block, 1, 1,
									   (unsigned)plan.scatter_lds_bytes, task->stream, args_scatter, nullptr),
				 plan.lds_rows ? "launch gpupreagg hash scatter (LDS)" : "launch gpupreagg hash scatter", false);
	task->pfm.num_kern_exec += 3;
	task->pfm.num_kern_prep++;				/* (reported: this request took the partition plan) */
	return hash_fold_turns(task, sess, plan.headroom, nrows, false, attempt,
		[&](int turn, cl_uint ntodo, cl_uint claim_limit, cl_uint a_turn, const void **p_count) -> bool
		{
			void	   *a_tab = sess->htab, *a_deferred = d_ctl + offsetof(gpupreagg_part_ctl, deferred);
			/* two redo lists: this turn runs the one the turn before wrote */
			void	   *a_todo = (turn > 0 ? d_lists + (size_t)max_units * ((turn - 1) & 1) : nullptr);
			void	   *a_redo = d_lists + (size_t)max_units * (turn & 1);
			void	   *args[] = { &ca.kg, &a_tab, &claim_limit, &a_ctl, &a_units, &a_records, &unit_lds_slots,
								   &a_todo, &ntodo, &a_redo, &a_turn };
			if (p_count)
			{
				*p_count = a_deferred;
				REQ_CHECK_OR(hipMemsetAsync(a_deferred, 0, sizeof(cl_uint), task->stream), "reset the redo list", false);
			}
			REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn_units, plan.unit_fold_grid, 1, 1, plan.unit_fold_block, 1, 1,
											   (unsigned)plan.unit_lds_bytes, task->stream, args, nullptr),
						 "launch gpupreagg hash fold (partitions)", false);
			return true;
		});
}

/*
 * roles: as many as it takes for a role's share of the groups seen so far to fill 5/8 of its LDS
 * table (64 probes find room at that fill).  Every role scans every row's key columns: ~0.2 ms
 * per 1e8 rows and role against 23-47 ms through the global table, so up to 64 roles pay
 * (measured, 1e8 rows: 1000 groups 11.5 -> 1.6 ms with 2 roles, 1e4 groups 26.7 -> 5.1 ms with
 * 16, 3e4 groups 13.2 ms with 64).  Counted anew in every turn: making room may have looked at
 * the table and learnt of more groups.
 */
cl_uint
hash_role_count(const strom_gpupreagg *sess, const hashed_knobs &knobs, const hashed_plan &plan)
{
	cl_uint		nroles = 1;
	cl_ulong	per_role = std::max<cl_ulong>(1, (cl_ulong)plan.role_lds_slots * knobs.fill_num / knobs.fill_den);
	cl_ulong	known = sess->groups_known;
	if (plan.column_streams && known > per_role && known <= per_role * 64)
		while (nroles < 64 && (cl_ulong)nroles * per_role < known)
			nroles <<= 1;
	if (plan.column_streams && knobs.roles)
		nroles = knobs.roles;
	return nroles;
}

/* launch step D, hash roles -- pass 1, errors only (a chunk with a CpuReCheck row is not folded at all),
 * then the fold.  Rows that need a new group beyond the claim limit come back as a row map, the table
 * grows, and they are folded again.  False: the task has failed. */
bool
queue_role_fold(strom_task_impl *task, const preagg_request &req, const hashed_knobs &knobs,
				const hashed_plan &plan, const sent_request &sent, cl_uint attempt)
{
	strom_gpupreagg *sess = req.sess;
	Device	   *dev = task->dev;
	chunk_args	ca = { sent.d_kg, sent.d_kds, nullptr, sent.d_rowmap };
	cl_uint		nrows = req.nrows, lds_slots = plan.role_lds_slots;
	unsigned	block = plan.block;
	/*
	 * role map: when the fold will run with hash roles (COLUMN chunk, no row map, more
	 * groups than one LDS table takes) the check pass leaves one byte per row -- the
	 * row's role -- and the roles' scans read that instead of the qual's and the keys'
	 * columns.  Padded with ROLE_NONE to whole scan tiles (16 rows per lane of a
	 * fold work-group).
	 */
	void	   *a_rolemap = nullptr;
	if (plan.column_streams && !ca.map && nrows > 0 &&
		(cl_ulong)sess->groups_known > (cl_ulong)lds_slots * 5 / 8 && !knobs.no_rolemap)
	{
		size_t	tile = (size_t)block * 16;
		size_t	len = (((size_t)nrows + tile - 1) / tile) * tile;
		a_rolemap = dev->pool.alloc(len);
		if (a_rolemap)
		{
			task->devbufs.push_back(a_rolemap);
			REQ_CHECK_OR(hipMemsetAsync(a_rolemap, 0xff, len, task->stream), "pad the role map", false);
		}
	}
	{
		void	   *a_tab = sess->htab, *a_nodefer = nullptr;
		cl_uint		no_limit = ~0u, one_role = 1;
		void	   *args[] = { &ca.kg, &ca.kds, &ca.toast, &ca.map, &a_tab, &no_limit, &a_nodefer, &lds_slots,
							   &one_role, &a_rolemap };
		/* (the kernels deal tiles to 8 XCDs: grids are multiples of 8) */
		unsigned	maxgrid = (unsigned)dev->prop.multiProcessorCount * 8;
		unsigned	grid = std::max(8u, std::min<unsigned>((nrows + 255) / 256 + 7, maxgrid) & ~7u);
		REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn_check, grid, 1, 1, 256, 1, 1, 0, task->stream, args, nullptr),
					 "launch gpupreagg hash check", false);
		task->pfm.num_kern_exec++;
	}
	void	   *d_defer[2] = { nullptr, nullptr };
	return hash_fold_turns(task, sess, plan.headroom, nrows, true, attempt,
		[&](int turn, cl_uint carried, cl_uint claim_limit, cl_uint a_turn, const void **p_count) -> bool
		{
			cl_uint		todo = (turn > 0 ? carried : nrows);
			void	   *a_tab = sess->htab;
			/* (the rows a turn deferred are the next launch's row map: the scan over the columns) */
			const void *a_map = (turn > 0 ? d_defer[(turn - 1) & 1] : ca.map);
			void	   *a_defer = nullptr;
			if (p_count)
			{
				if (!d_defer[turn & 1])
				{
					d_defer[turn & 1] = dev->pool.alloc(offsetof(kern_row_map, rindex) + sizeof(cl_int) * (size_t)todo);
					if (!d_defer[turn & 1])
					{
						task_fail(task, StromError_OutOfMemory);
						return false;
					}
					task->devbufs.push_back(d_defer[turn & 1]);
				}
				*p_count = a_defer = d_defer[turn & 1];		/* (a kern_row_map begins with its count) */
				REQ_CHECK_OR(hipMemsetAsync(a_defer, 0, offsetof(kern_row_map, rindex), task->stream),
							 "reset deferred rows", false);
			}
			cl_uint		nroles = hash_role_count(sess, knobs, plan);
			void	   *a_rm = (turn == 0 && nroles > 1 ? a_rolemap : nullptr);
			void	   *args[] = { &ca.kg, &ca.kds, &ca.toast, &a_map, &a_tab, &claim_limit, &a_defer, &lds_slots,
								   &nroles, &a_rm, &a_turn };
			unsigned	unit = 8 * nroles;
			unsigned	grid = std::min<unsigned>(((todo + block - 1) / block + unit - 1) / unit * unit, plan.role_fold_grid);
			grid = std::max(unit, grid / unit * unit);
			REQ_CHECK_OR(hipModuleLaunchKernel(plan.fn_fold, grid, 1, 1, block, 1, 1, (unsigned)plan.role_lds_bytes,
											   task->stream, args, nullptr),
						 "launch gpupreagg hash fold", false);
			return true;
		});
}

/* The hashed launch, step by step.  sess->lock is held throughout, the turns that wait for the device
 * included: the table, its bounds and the sums' parity belong to one fold at a time. */
void
gpupreagg_launch_hashed(strom_task_impl *task, preagg_request req, bool second)
{
	strom_gpupreagg *sess = req.sess;
	Device	   *dev = task->dev;
	Program	   *prog = sess->prog;
	std::lock_guard<std::mutex> g(sess->lock);

	(void)hipSetDevice(dev->hip_id);
	if (prog->state != STROM_DEVPROG_READY)
	{
		task_fail(task, StromError_ProgramBuildFailure);
		return;
	}
	task->pfm.time_kern_build = (cl_ulong)prog->build_usec;
	task->stream = dev->streams[0];
	const hashed_knobs knobs = read_hashed_knobs();							/* A */
	/* B, around the table: the roles' geometry says how large it must be, the rest reads it */
	hashed_plan	plan;
	int			rc = plan_role_table(dev, prog, sess, knobs, &plan);
	if (rc == 0)
		rc = hash_table_for_fold(sess, 4 * plan.headroom);
	if (rc == 0)
		rc = plan_hashed_fold(dev, prog, req, knobs, &plan);
	/* a second attempt: the sums' bound is measured from the table first */
	if (rc == 0 && second)
		rc = hash_sum_refresh(sess);
	if (rc)
	{
		task_fail(task, rc);
		return;
	}
	/* C.  integer sums never wrap (strom_gpupreagg.h): rows of the request, what is known about
	 * the inputs before the check pass measures the rest */
	sent_request sent;
	if (!send_request(task, req, task->stream, sess->static_magbits, 0, false, nullptr, &sent))	/* ev[0] */
		return;
	task_event(task);									/* ev[1] */
	/* D.  (bit 2 of the turn -- "a failed proof is final: CpuReCheck" -- only where the exact fold,
	 * gpupreagg_hashed_exact, is switched off: the host sends an unproven chunk there instead) */
	const bool	no_exact = knobs.no_exact;
	cl_uint		attempt = (second && no_exact ? 4u : 0u);
	if (!(plan.use_parts ? queue_partition_plan(task, req, plan, sent, attempt)
						 : queue_role_fold(task, req, knobs, plan, sent, attempt)))
		return;
	task_event(task);									/* ev[2] */
	char   *stage_status = sent.stage + sent.kg_len;
	REQ_CHECK(hipMemcpyAsync(stage_status, sent.d_kg + offsetof(kern_gpupreagg, status), sizeof(cl_int), hipMemcpyDeviceToHost, task->stream),
			  "recv status");
	REQ_CHECK(hipMemcpyAsync(stage_status + 16, sess->htab, HASH_HEAD_COUNTERS, hipMemcpyDeviceToHost, task->stream),
			  "recv table head");
	task->pfm.num_dma_recv += 2;
	task->pfm.bytes_dma_recv += sizeof(cl_int) + 16;
	task_event(task);									/* ev[3] */
	task->finish = [stage_status, sess, req, second, no_exact](strom_task_impl *t)
	{
		cl_int	status;
		gpupreagg_hash_head head;
		memcpy(&status, stage_status, sizeof(status));
		memcpy(&head, stage_status + 16, HASH_HEAD_COUNTERS);
		if (status == StromError_SumRangeUnproven && !second)
		{
			/* the running bound of the integer sums reached 2^63 and nothing was folded:
			 * once more, with the bound measured from the table (hash_sum_refresh) */
			t->retry = [t, req]() { gpupreagg_launch_hashed(t, req, true); };
			return;
		}
		if (status == StromError_SumRangeUnproven && !req.exact_parent && !no_exact)
		{
			/* rows x largest magnitude still reaches 2^63 -- a bound over ALL groups at once,
			 * which says little about any one of them: the chunk is folded exactly instead */
			t->retry = [t, req]() { gpupreagg_hashed_exact(t, req); };
			return;
		}
		if (status == StromError_Success && req.exact_parent)
		{
			/* the scratch session holds the chunk's groups, every addition checked: they
			 * join the parent's under a per-group range check */
			t->retry = [t, req]() { gpupreagg_hashed_exact_merge(t, req); };
			return;
		}
		if (status == StromError_SumRangeUnproven)
			status = StromError_CpuReCheck;
		if (status == StromError_Success && head.overflow != 0)
			status = StromError_DataStoreNoSpace;	/* cannot happen: headroom is kept for every claim */
		sess->groups_known = std::max<cl_uint>(sess->groups_known, head.ngroups);
		t->errcode = status;
	};
	task_enqueue(task);
}

}	/* namespace */

/* ================================================================== *
 * C ABI
 * ================================================================== */
static strom_gpupreagg *
gpupreagg_session_new(strom_devprog_key key,
					  const strom_preagg_target *targets, int ntargets,
					  const kern_parambuf *kparams,
					  const strom_preagg_domain *domain, bool hashed,
					  int dindex, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	*p_errcode = 0;
	Program *prog = lookup_program(key);
	Device *dev = get_device(dindex);
	if (!prog || !dev || !targets || ntargets < 1 || !kparams)
	{
		*p_errcode = (!dev ? StromError_ServerNotReady : StromError_BadRequestMessage);
		return nullptr;
	}
	strom_gpupreagg *sess = new strom_gpupreagg();
	sess->key = key;
	sess->prog = prog;
	sess->dev = dev;
	sess->targets.assign(targets, targets + ntargets);
	for (int i = 0; i < ntargets; i++)
	{
		if (targets[i].kind == STROM_PREAGG_KEY)
		{
			if (!hashed && (type_is_float(targets[i].type_oid) || targets[i].type_oid == STROM_NUMERICOID))
			{
				/* dense ids need integer-like keys */
				*p_errcode = StromError_DataStoreOutOfRange;
				delete sess;
				return nullptr;
			}
			sess->key_resno.push_back(i);
		}
		else
			sess->agg_resno.push_back(i);
	}
	sess->kparams.assign((const char *)kparams, (const char *)kparams + kparams->length);
	{
		/* what the code generator says about packed accumulators (codegen_preagg.cpp) */
		const char *src = prog->source.c_str();
		const char *lst = strstr(src, "#define GPUPREAGG_PACK_LIST(X)");
		sess->numeric_aggs = (strstr(src, "#define GPUPREAGG_NUMERIC_AGGS 1") != nullptr);
		if (const char *vl = strstr(src, "#define STROM_KVARLENA_LIST(X)"))
		{
			/* (codegen.cpp: codegen_var_list -- X(attno,text) / X(attno,bpcharn)) */
			const char *eol = strchr(vl, '\n');
			for (const char *p = strstr(vl, " X("); p && (!eol || p < eol); p = strstr(p + 1, " X("))
			{
				int		attno = 0;
				char	name[16] = "";
				if (sscanf(p, " X(%d,%15[a-z0-9])", &attno, name) == 2 && attno >= 1)
					sess->varlena_vars.emplace_back(attno, !strcmp(name, "text") ? STROM_TEXTOID : STROM_BPCHARNOID);
			}
		}
		sess->packable = (strstr(src, "#define GPUPREAGG_PACKABLE 1") != nullptr && lst != nullptr);
		if (lst)
		{
			/* (read for every program: the source column of a plain-column sum also bounds it,
			 * see gpupreagg_launch) */
			bool		whole = true;
			const char *eol = strchr(lst, '\n');
			for (const char *p = strstr(lst, " X("); p && (!eol || p < eol); p = strstr(p + 1, " X("))
			{
				int		aidx = -1, kind = 0, attno = 0;
				if (sscanf(p, " X(%d,%d,%d)", &aidx, &kind, &attno) != 3 || aidx != (int)sess->pack_kind.size())
				{
					whole = false;
					break;
				}
				sess->pack_kind.push_back(kind);
				sess->pack_attno.push_back(attno);
			}
			if (!whole || sess->pack_kind.size() != sess->agg_resno.size())
			{
				sess->pack_kind.assign(sess->agg_resno.size(), 0);
				sess->pack_attno.assign(sess->agg_resno.size(), 0);
				sess->packable = false;
			}
			if (sess->agg_resno.size() > GPUPREAGG_PACK_MAXAGGS)
				sess->packable = false;
		}
		else
		{
			sess->pack_kind.assign(sess->agg_resno.size(), 0);
			sess->pack_attno.assign(sess->agg_resno.size(), 0);
		}
		/* integer sums: which aggregates, and what the code generator knows about their inputs */
		for (size_t a = 0; a < sess->agg_resno.size(); a++)
		{
			const strom_preagg_target &t = sess->targets[sess->agg_resno[a]];
			bool	intsum = (t.kind == STROM_PREAGG_PSUM &&
							  (t.type_oid == STROM_INT8OID || (t.type_oid == STROM_NUMERICOID && t.scale >= 0)));
			char	name[64];
			int		bits = 64;
			snprintf(name, sizeof(name), "#define GPUPREAGG_SUMBITS_%zu ", a);
			const char *def = strstr(src, name);
			if (def)
				bits = atoi(def + strlen(name));
			if (intsum != (bits != 0))
			{
				/* the caller's targets do not describe this program */
				*p_errcode = StromError_BadRequestMessage;
				delete sess;
				return nullptr;
			}
			sess->sumbits.push_back(bits);
			{
				std::string	formula;
				snprintf(name, sizeof(name), "#define GPUPREAGG_SUMBOUND_%zu \"", a);
				const char *fdef = strstr(src, name);
				if (fdef)
				{
					const char *q = strchr(fdef + strlen(name), '"');
					if (q)
						formula.assign(fdef + strlen(name), q);
				}
				sess->sumbound.push_back(formula);
			}
			sess->intsum_of.push_back(intsum ? sess->nintsums++ : -1);
			if (bits >= 1 && bits <= 63)
				sess->static_magbits = std::max(sess->static_magbits, (cl_uint)bits);
			if (intsum && bits >= 64)
				sess->sums_measured = true;
		}
	}
	if (const char *v = getenv("STROM_GPUPREAGG_BLOCK"))
		sess->block = atoi(v);
	if (const char *v = getenv("STROM_GPUPREAGG_QUADS"))
		sess->quads = atoi(v);
	strom_retain_devprog_key(key);
	sess->hashed = hashed;
	if (hashed && (sess->key_resno.size() > 31 || sess->agg_resno.size() > 30 || sess->numeric_aggs))
	{
		*p_errcode = StromError_BadRequestMessage;
		strom_gpupreagg_release(sess);
		return nullptr;
	}
	if (domain)
	{
		int rc = setup_geometry(sess, domain);
		if (rc == 0)
			rc = alloc_session_buffers(sess);
		if (rc != 0)
		{
			*p_errcode = rc;
			strom_gpupreagg_release(sess);
			return nullptr;
		}
	}
	return sess;
	STROM_ABI_CATCH(nullptr, p_errcode)
}

extern "C" strom_gpupreagg *
strom_gpupreagg_create(strom_devprog_key key,
					   const strom_preagg_target *targets, int ntargets,
					   const kern_parambuf *kparams,
					   const strom_preagg_domain *domain,
					   int dindex, int *p_errcode)
{
	return gpupreagg_session_new(key, targets, ntargets, kparams, domain, false, dindex, p_errcode);
}

extern "C" strom_gpupreagg *
strom_gpupreagg_create_hashed(strom_devprog_key key,
							  const strom_preagg_target *targets, int ntargets,
							  const kern_parambuf *kparams,
							  uint32_t ngroups_hint,
							  int dindex, int *p_errcode)
{
	/* the hashed kernels are a program of their own, derived from the caller's
	 * (strom_gpupreagg.h builds one family or the other); it builds in the
	 * background, the first fold parks behind it */
	Program *base = lookup_program(key);
	if (!base)
	{
		if (p_errcode)
			*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	const char *hashed_define = "#define GPUPREAGG_HASHED 1\n";
	std::string	hsource = base->source;
	if (hsource.compare(0, strlen(hashed_define), hashed_define) != 0)
		hsource = hashed_define + hsource;	/* (a caller may also hand over the derived program itself) */
	strom_devprog_key hkey = strom_get_devprog_key(hsource.c_str(), base->extra_flags);
	strom_gpupreagg *sess = gpupreagg_session_new(hkey, targets, ntargets, kparams, nullptr, true,
												  dindex, p_errcode);
	strom_put_devprog_key(hkey);			/* the session holds its own reference */
	if (!sess)
		return nullptr;
	/* the table itself is made by the first fold (the program may still be building) */
	cl_ulong	capacity = 1UL << 16;
	while (capacity < (cl_ulong)ngroups_hint * 2 && capacity < (1UL << 31))
		capacity <<= 1;
	sess->hash_capacity = (cl_uint)capacity;
	sess->groups_known = ngroups_hint;
	return sess;
}

static strom_gpupreagg *
gpupreagg_exact_child(strom_gpupreagg *sess, int *p_errcode)
{
	std::string	source = "#define GPUPREAGG_CHECKED 1\n" + sess->prog->source;
	strom_devprog_key ckey = strom_get_devprog_key(source.c_str(), sess->prog->extra_flags);
	if (!ckey)
	{
		*p_errcode = StromError_OutOfMemory;
		return nullptr;
	}
	strom_gpupreagg *child = gpupreagg_session_new(ckey, sess->targets.data(), (int)sess->targets.size(),
												   (const kern_parambuf *)sess->kparams.data(), nullptr, true,
												   sess->dev->dindex, p_errcode);
	strom_put_devprog_key(ckey);			/* the session holds its own reference */
	if (!child)
		return nullptr;
	child->hash_capacity = 1u << 16;		/* grows with the chunk's groups like any hashed table */
	return child;
}

/* the bound formula of a summed expression (GPUPREAGG_SUMBOUND_<a> of a generated program) over
 * a COLUMN chunk's zone maps: bits of the largest magnitude, or -1 (a column without a zone map,
 * another format, a malformed formula).  No device involved: what the launch path computes. */
extern "C" int
strom_gpupreagg_sum_bound_bits(const char *formula, const kern_data_store *kds)
{
	if (!formula || !kds || kds->format != KDS_FORMAT_COLUMN)
		return -1;
	return eval_sum_bound(formula, KERN_DATA_STORE_COLDIR(kds), kds->ncols);
}

extern "C" size_t
strom_gpupreagg_table_length(strom_gpupreagg *sess)
{
	return (sess && sess->has_domain) ? sess->table_bytes : 0;
}

extern "C" int
strom_gpupreagg_bind_table(strom_gpupreagg *sess, void *table_devptr)
{
	if (!sess || !sess->has_domain || !table_devptr)
		return StromError_BadRequestMessage;
	std::lock_guard<std::mutex> g(sess->lock);
	(void)hipSetDevice(sess->dev->hip_id);
	if (session_quiesce(sess) != hipSuccess ||
		hipMemcpy(table_devptr, sess->table, sess->table_bytes, hipMemcpyDeviceToDevice) != hipSuccess)
		return StromError_HipInternal;
	if (sess->table_owned)
		sess->dev->pool.release(sess->table);
	sess->table = (char *)table_devptr;
	sess->table_owned = false;
	return 0;
}

extern "C" void *
strom_gpupreagg_table_devptr(strom_gpupreagg *sess) { return sess ? sess->table : nullptr; }

extern "C" uint32_t
strom_gpupreagg_num_groups(strom_gpupreagg *sess)
{
	if (sess && sess->hashed)
	{
		cl_uint	ngroups = 0;
		std::lock_guard<std::mutex> g(sess->lock);
		(void)hipSetDevice(sess->dev->hip_id);
		if (!sess->htab || hash_table_ngroups(sess, &ngroups, nullptr) != 0)
			return 0;
		return ngroups;
	}
	return (sess && sess->has_domain) ? sess->ctl.ngroups : 0;
}

extern "C" uint32_t
strom_gpupreagg_checked_folds(strom_gpupreagg *sess) { return sess ? sess->checked_folds.load() : 0; }

extern "C" uint32_t
strom_gpupreagg_dense_groups(strom_gpupreagg *sess) { return (sess && sess->has_domain) ? sess->ctl.dense_ngroups : 0; }

extern "C" int
strom_gpupreagg_table_layout(strom_gpupreagg *sess, int resno, size_t *p_bits_off, size_t *p_vals_off)
{
	if (!sess || !sess->has_domain || resno < 0 || resno >= (int)sess->targets.size())
		return StromError_BadRequestMessage;
	if (sess->targets[resno].kind == STROM_PREAGG_KEY)
	{
		*p_bits_off = 0;
		*p_vals_off = 0;
		return 0;
	}
	int a = (int)(std::find(sess->agg_resno.begin(), sess->agg_resno.end(), resno) - sess->agg_resno.begin());
	*p_bits_off = 0;			/* flags word: bit 0 seen, bit 1+a has-value */
	*p_vals_off = gpupreagg_table_offset(1 + a, sess->ctl.ngroups);
	return 0;
}

static strom_task *
submit_gpupreagg_common(strom_gpupreagg *sess,
						const kern_data_store *kds, strom_dstore *kds_dev,
						const kern_row_map *krowmap, strom_rowmap *rowmap_dev,
						strom_done_cb done, void *arg, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	*p_errcode = 0;
	if (!sess || (!kds) == (!kds_dev))
	{
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	if ((kds_dev && kds_dev->dindex != sess->dev->dindex) ||
		(rowmap_dev && (!kds_dev || krowmap || rowmap_dev->dindex != kds_dev->dindex)))
	{
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	if (!sess->hashed && !sess->has_domain)
	{
		/* first chunk fixes the dense domain (see strom_hip.h) */
		*p_errcode = StromError_DataStoreOutOfRange;
		return nullptr;
	}
	preagg_request req;
	req.sess = sess;
	req.kds = kds;
	req.kds_dev = kds_dev;
	req.krowmap = (krowmap && krowmap->nvalids >= 0) ? krowmap : nullptr;
	req.rowmap_dev = rowmap_dev;
	kern_data_store head;
	if (kds)
		memcpy(&head, kds, offsetof(kern_data_store, colmeta));
	else
		head = kds_dev->head;
	req.format = head.format;
	if (!program_accepts_format(sess->prog, head.format))
	{
		*p_errcode = StromError_BadRequestMessage;		/* text columns live in heap tuples */
		return nullptr;
	}
	req.nrows = (rowmap_dev ? rowmap_dev->nvalids
				 : req.krowmap ? (uint32_t)req.krowmap->nvalids : head.nitems);
	sess->nfolds++;
	strom_task_impl *task = task_create(sess->dev, done, arg);
	if (sess->hashed)
		program_run_or_park(sess->prog, [task, req]() { gpupreagg_launch_hashed(task, req); });
	else
		program_run_or_park(sess->prog, [task, req]() { gpupreagg_launch(task, req); });
	return task;
	STROM_ABI_CATCH(nullptr, p_errcode)
}

extern "C" strom_task *
strom_submit_gpupreagg(strom_gpupreagg *sess,
					   const kern_data_store *kds, strom_dstore *kds_dev,
					   const kern_row_map *krowmap,
					   strom_done_cb done, void *arg, int *p_errcode)
{
	return submit_gpupreagg_common(sess, kds, kds_dev, krowmap, nullptr, done, arg, p_errcode);
}

extern "C" strom_task *
strom_submit_gpupreagg_mapped(strom_gpupreagg *sess, strom_dstore *kds_dev, strom_rowmap *rowmap,
							  strom_done_cb done, void *arg, int *p_errcode)
{
	if (!rowmap)
	{
		if (p_errcode)
			*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	return submit_gpupreagg_common(sess, nullptr, kds_dev, nullptr, rowmap, done, arg, p_errcode);
}


namespace {

/*
 * the wanted columns of relation 'depth' (1-based) as hashjoin_table_dimrecs takes them: cols[] / lens[] /
 * ints[] (may take the narrow form: not a float, not a numeric image), which[] the virtual column each one
 * serves.  Returns their number, -1 for more than HASHJOIN_DIMREC_MAXCOLS.  Pure: no device, no session.
 */
int
collect_relation_columns(int depth, int ncols, const int32_t *src_depth, const int32_t *src_colidx,
						 const int32_t *type_oids, int *cols, int *lens, int *ints, int *which, uint64_t *p_mask)
{
	int		n = 0;
	*p_mask = 0;
	for (int i = 0; i < ncols; i++)
	{
		if (src_depth[i] != depth)
			continue;
		if (n == HASHJOIN_DIMREC_MAXCOLS)
			return -1;
		int		oid = (type_oids[i] < 0 ? -type_oids[i] : type_oids[i]);
		cols[n] = src_colidx[i];
		lens[n] = type_length(oid);
		ints[n] = !(type_is_float(oid) || oid == STROM_NUMERICOID);
		which[n++] = i;
		*p_mask |= ((uint64_t)1 << i);
	}
	return n;
}

/*
 * One mapping builder for strom_submit_gpupreagg_joined, _lookup and _lookup_star: checks the arguments,
 * asks every table what it is, downloads the outer chunk's head for its column widths, has every relation's
 * slot records made and describes the result in *m.  Returns 0, or the code to refuse the request with.
 * The entry points answer some faults with different codes and in a different order; callers may rely on
 * either, so each difference is kept and marked where the code branches on the entry: (1) to (4) below.
 * PREAGG_UNMATCHED (strom_submit_gpupreagg_lookup_unmatched) describes the mapping of a lookup (ntbls == 1) or
 * a star WITHOUT a chunk: outer is NULL, so nothing is held against a chunk's head -- no key width, no fact
 * column's width, no text variable's column (every fact column of that pass is NULL) -- and only relation
 * 'tracked' has its slot records made, the same records the folds of that mapping read.
 */
int
build_fold_mapping(strom_gpupreagg *sess, preagg_kind entry, strom_task_impl *jtask,
				   strom_hashjoin_table *const *tbls, int ntbls, strom_dstore *outer,
				   int ncols, const int32_t *src_depth, const int32_t *src_colidx, const int32_t *type_oids,
				   fold_mapping *m, int tracked = 0)
{
	const bool	nochunk = (entry == PREAGG_UNMATCHED);
	const bool	star = (entry == PREAGG_STAR || (nochunk && ntbls != 1));

	if (!sess || sess->hashed || !sess->has_domain || (entry == PREAGG_JOINED && !jtask) || !tbls || (!outer) != nochunk ||
		ntbls < 1 || ntbls > GPUPREAGG_STAR_MAXRELS ||
		ncols < 1 || ncols > GPUPREAGG_JOINED_MAXCOLS || !src_depth || !src_colidx || !type_oids)
		return StromError_BadRequestMessage;
	for (int r = 0; r < ntbls; r++)
		if (!tbls[r])
			return StromError_BadRequestMessage;
	if (jtask)
		task_wait_completed(jtask);
	/* needs: (joined) a finished join with STROM_RESULTS_ON_DEVICE; per table one inner relation with a DIRECT
	 * index and unique keys, joined on a plain outer column; a resident COLUMN chunk; all on the session's device */
	int			outer_ncols = (nochunk ? 0 : (int)outer->head.ncols);
	bool		ok = (!jtask || (jtask->res_is_join && jtask->keep_main && jtask->errcode == 0 && jtask->main_devptr));
	/* the records of the unmatched pass of a RIGHT / FULL join have no outer row (word 0 == 0): the
	 * joined fold reads the outer chunk at word 0 - 1 and would leave it.  They go through
	 * strom_hashjoin_project_column(task, tbl, NULL, ..) and a plain fold. */
	ok = ok && !(jtask && jtask->res_is_unmatched);
	ok = ok && (nochunk || (outer->head.format == KDS_FORMAT_COLUMN && outer->dindex == sess->dev->dindex));
	m->ncols = ncols;
	m->nrels = ntbls;
	for (int r = 0; ok && r < ntbls; r++)
	{
		int		key_attno = 0, tbl_dindex = -1, has_outer_qual = 0;
		ok = (hashjoin_table_direct_info(tbls[r], &m->key_min[r], &m->nslots[r], &key_attno,
										 &tbl_dindex, &has_outer_qual) == 0 &&
			  /* a lookup runs the aggregate program only: a WHERE that lives in the join
			   * program would silently not be applied */
			  !(entry != PREAGG_JOINED && has_outer_qual) &&
			  /* ... and probes without running the join program: a table whose program tracks
			   * matches (RIGHT / FULL) would keep every flag clear and its unmatched pass would
			   * silently emit matched entries.  The joined fold is fine: the join ran and flagged. */
			  !(entry != PREAGG_JOINED && strom_hashjoin_table_tracked_depth(tbls[r]) != 0) &&
			  key_attno >= 1 && (nochunk || key_attno <= outer_ncols) && tbl_dindex == sess->dev->dindex);
		m->key_col[r] = key_attno - 1;
	}
	if (!ok)
		return ((jtask && jtask->errcode) ? jtask->errcode : StromError_BadRequestMessage);
	/* (1) the star refuses a depth outside 0 .. ntbls and ANY negative column index up front, as a
	 * BadRequest; the one-table calls meet them column by column below, where a negative index of an
	 * OUTER column is a DataStoreCorruption */
	for (int i = 0; star && i < ncols; i++)
		if (src_depth[i] < 0 || src_depth[i] > ntbls || src_colidx[i] < 0)
			return StromError_BadRequestMessage;
	(void)hipSetDevice(sess->dev->hip_id);
	/* the outer chunk's column widths */
	std::vector<char> ohead(KDS_HEAD_LENGTH(outer_ncols));
	if (!nochunk && hipMemcpy(ohead.data(), outer->devptr, ohead.size(), hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_BadRequestMessage;
	const kern_data_store *oh = (const kern_data_store *)ohead.data();
	/* (these kernels stream the outer columns: a text variable must be one of them) */
	if (!nochunk && !varlena_mapping_ok(sess, ncols, src_depth, src_colidx, type_oids, oh))
		return StromError_BadRequestMessage;
	/* (2) the width of a join key: 4 or 8 bytes for a lookup (BadRequest), 1, 2, 4 or 8 for result
	 * pairs (DataStoreCorruption); the star looks BEFORE the columns, the one-table calls AFTER */
	auto key_widths = [&]() -> int {
		for (int r = 0; r < ntbls && !nochunk; r++)
		{
			int		len = m->key_attlen[r] = oh->colmeta[m->key_col[r]].attlen;
			if (!(len == 4 || len == 8 || (entry == PREAGG_JOINED && (len == 1 || len == 2))))
				return (entry == PREAGG_JOINED ? StromError_DataStoreCorruption : StromError_BadRequestMessage);
		}
		return 0;
	};
	int			rc = (star ? key_widths() : 0);
	if (rc != 0)
		return rc;
	for (int i = 0; i < ncols; i++)
	{
		memset(&m->c[i], 0, sizeof(m->c[i]));
		m->c[i].depth = src_depth[i];
		m->c[i].col = src_colidx[i];
		if (src_depth[i] == 0)
		{
			/* a text / character(n) column is an outer column's offset array: attlen -1.
			 * (3) the one-table calls know the type by |oid|, the star by the oid as given: under
			 * a negative oid it takes text for an 8-byte value, and refuses */
			int		oid = (star ? type_oids[i] : type_oids[i] < 0 ? -type_oids[i] : type_oids[i]);
			int		attlen = ((oid == STROM_TEXTOID || oid == STROM_BPCHARNOID) ? -1 : type_length(oid));
			if (!nochunk &&
				(src_colidx[i] < 0 || src_colidx[i] >= outer_ncols || oh->colmeta[src_colidx[i]].attlen != attlen))
				return StromError_DataStoreCorruption;
		}
		else if (src_depth[i] < 1 || src_depth[i] > ntbls || src_colidx[i] < 0)
			return StromError_BadRequestMessage;	/* (an inner column itself: the build kernel checks it) */
	}
	rc = (star ? 0 : key_widths());
	if (rc != 0)
		return rc;
	for (int r = 0; r < ntbls; r++)
	{
		m->inner_mask[r] = 0;
		m->reclen[r] = m->narrow[r] = 0;
		m->recs[r] = 0;
		if (nochunk && r + 1 != tracked)
			continue;
		/* one packed record per slot: presence, NULL bits and the wanted columns of relation r + 1 */
		int			cols[HASHJOIN_DIMREC_MAXCOLS], lens[HASHJOIN_DIMREC_MAXCOLS];
		int			which[HASHJOIN_DIMREC_MAXCOLS], ints[HASHJOIN_DIMREC_MAXCOLS];
		unsigned	offs[HASHJOIN_DIMREC_MAXCOLS], reclen = 0;
		void	   *recs = nullptr;
		dimrec_narrow nw;
		int			n = collect_relation_columns(r + 1, ncols, src_depth, src_colidx, type_oids,
												 cols, lens, ints, which, &m->inner_mask[r]);
		if (n < 0)
			return StromError_BadRequestMessage;
		/* (4) the lookup kernels also read the narrow form (2 / 4 bytes per slot: more of the table
		 * stays in L2 while the fact columns stream past); the result pairs' kernel does not */
		rc = hashjoin_table_dimrecs(tbls[r], n, cols, lens, offs, &recs, &reclen, ints,
									entry == PREAGG_JOINED ? nullptr : &nw);
		if (rc != 0)
			return rc;
		bool		narrow = (entry != PREAGG_JOINED && nw.spec.reclen != 0);
		m->recs[r] = (cl_ulong)(uintptr_t)(narrow ? nw.recs : recs);
		m->reclen[r] = (narrow ? nw.spec.reclen : reclen);
		m->narrow[r] = (narrow ? 1 : 0);
		for (int k = 0; k < n; k++)
		{
			auto   &c = m->c[which[k]];
			c.recoff = (narrow ? 0 : offs[k]);		/* byte offset in the record */
			c.nullbit = 1 + k;						/* bit in the flags word */
			if (narrow)
			{
				c.nshift = nw.spec.shift[k];
				c.nmask = nw.spec.mask[k];
				c.nmin = nw.spec.vmin[k];
			}
		}
	}
	return 0;
}

/*
 * The mapping of strom_submit_gpupreagg_lookup_snowflake: the tree flattened into its roots' slot records
 * (hashjoin_snowflake_dimrecs), and *m the star of those roots -- a virtual column of any relation of a
 * subtree points at its field in the ROOT's record.  The checks, their order and their codes are the
 * star's (build_fold_mapping); what is new is said where it is checked.
 */
int
build_snowflake_mapping(strom_gpupreagg *sess, strom_hashjoin_table *const *tbls, int ntbls,
						const int32_t *parent, const int32_t *link_type_oids, strom_dstore *outer,
						int ncols, const int32_t *src_depth, const int32_t *src_colidx, const int32_t *type_oids,
						fold_mapping *m)
{
	int32_t		root_of[STROM_LOOKUP_SNOWFLAKE_MAXRELS], col_root[GPUPREAGG_JOINED_MAXCOLS];
	int			link_col[STROM_LOOKUP_SNOWFLAKE_MAXRELS] = {}, link_attlen[STROM_LOOKUP_SNOWFLAKE_MAXRELS] = {};

	if (!sess || sess->hashed || !sess->has_domain || !tbls || !parent || !link_type_oids || !outer ||
		ncols < 1 || ncols > GPUPREAGG_JOINED_MAXCOLS || !src_depth || !src_colidx || !type_oids)
		return StromError_BadRequestMessage;
	int			nroots = strom_gpupreagg_lookup_snowflake_roots(ntbls, parent, ncols, src_depth, root_of, col_root);
	if (nroots < 1)
		return StromError_BadRequestMessage;
	for (int d = 1; d <= ntbls; d++)
		if (!tbls[d - 1])
			return StromError_BadRequestMessage;
	int			outer_ncols = (int)outer->head.ncols;
	if (outer->head.format != KDS_FORMAT_COLUMN || outer->dindex != sess->dev->dindex)
		return StromError_BadRequestMessage;
	m->ncols = ncols;
	m->nrels = nroots;
	for (int d = 1; d <= ntbls; d++)
	{
		int			key_attno = 0, tbl_dindex = -1, has_outer_qual = 0;
		cl_long		key_min;
		cl_uint		nslots;
		if (hashjoin_table_direct_info(tbls[d - 1], &key_min, &nslots, &key_attno, &tbl_dindex, &has_outer_qual) != 0 ||
			has_outer_qual || key_attno < 1 || tbl_dindex != sess->dev->dindex ||
			strom_hashjoin_table_tracked_depth(tbls[d - 1]) != 0)		/* (as build_fold_mapping says) */
			return StromError_BadRequestMessage;
		if (parent[d - 1] == 0)
		{
			int		r = root_of[d - 1] - 1;
			if (key_attno > outer_ncols)
				return StromError_BadRequestMessage;
			m->key_col[r] = key_attno - 1;
			m->key_min[r] = key_min;
			m->nslots[r] = nslots;
			continue;
		}
		/* the table's program names a column of its PARENT relation; its type is the caller's word (the
		 * build kernel holds it against the parent's rows: DataStoreCorruption) */
		int		oid = link_type_oids[d - 1];
		if (!(oid == STROM_INT4OID || oid == STROM_DATEOID || oid == STROM_INT8OID))
			return StromError_BadRequestMessage;
		link_col[d - 1] = key_attno - 1;
		link_attlen[d - 1] = type_length(oid);
	}
	for (int i = 0; i < ncols; i++)
		if (src_colidx[i] < 0)
			return StromError_BadRequestMessage;
	(void)hipSetDevice(sess->dev->hip_id);
	std::vector<char> ohead(KDS_HEAD_LENGTH(outer_ncols));
	if (hipMemcpy(ohead.data(), outer->devptr, ohead.size(), hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_BadRequestMessage;
	const kern_data_store *oh = (const kern_data_store *)ohead.data();
	if (!varlena_mapping_ok(sess, ncols, src_depth, src_colidx, type_oids, oh))
		return StromError_BadRequestMessage;
	for (int r = 0; r < nroots; r++)
	{
		int		len = m->key_attlen[r] = oh->colmeta[m->key_col[r]].attlen;
		if (!(len == 4 || len == 8))
			return StromError_BadRequestMessage;
	}
	for (int i = 0; i < ncols; i++)
	{
		memset(&m->c[i], 0, sizeof(m->c[i]));
		m->c[i].depth = col_root[i];
		m->c[i].col = src_colidx[i];
		if (src_depth[i] == 0)
		{
			int		oid = type_oids[i];
			int		attlen = ((oid == STROM_TEXTOID || oid == STROM_BPCHARNOID) ? -1 : type_length(oid));
			if (src_colidx[i] >= outer_ncols || oh->colmeta[src_colidx[i]].attlen != attlen)
				return StromError_DataStoreCorruption;
		}
	}
	for (int d = 1; d <= ntbls; d++)
	{
		if (parent[d - 1] != 0)
			continue;
		/* the served columns of this root's whole subtree, in one composed record per slot of the root */
		int			r = root_of[d - 1] - 1;
		snowflake_column cols[HASHJOIN_DIMREC_MAXCOLS];
		int			which[HASHJOIN_DIMREC_MAXCOLS], n = 0;
		unsigned	reclen = 0;
		void	   *recs = nullptr;
		dimrec_narrow nw;
		m->inner_mask[r] = 0;
		for (int i = 0; i < ncols; i++)
		{
			if (col_root[i] != r + 1)
				continue;
			if (n == HASHJOIN_DIMREC_MAXCOLS)
				return StromError_BadRequestMessage;
			int		oid = (type_oids[i] < 0 ? -type_oids[i] : type_oids[i]);
			cols[n] = { src_depth[i], src_colidx[i], type_length(oid),
						!(type_is_float(oid) || oid == STROM_NUMERICOID), 0, 0 };
			which[n++] = i;
			m->inner_mask[r] |= ((uint64_t)1 << i);
		}
		int			rc = hashjoin_snowflake_dimrecs(tbls, ntbls, parent, link_col, link_attlen, d, cols, n,
													&recs, &reclen, &nw);
		if (rc != 0)
			return rc;
		bool		narrow = (nw.spec.reclen != 0);
		m->recs[r] = (cl_ulong)(uintptr_t)(narrow ? nw.recs : recs);
		m->reclen[r] = (narrow ? nw.spec.reclen : reclen);
		m->narrow[r] = (narrow ? 1 : 0);
		for (int k = 0; k < n; k++)
		{
			auto   &c = m->c[which[k]];
			c.recoff = (narrow ? 0 : cols[k].offset);
			c.nullbit = 1 + cols[k].recpos;
			if (narrow)
			{
				c.nshift = nw.spec.shift[cols[k].recpos];
				c.nmask = nw.spec.mask[cols[k].recpos];
				c.nmin = nw.spec.vmin[cols[k].recpos];
			}
		}
	}
	return 0;
}

/* the mapping as gpupreagg_dense_joined / _lookup read it (one relation) */
std::shared_ptr<std::vector<char>>
write_joined_map(const fold_mapping &m)
{
	auto	img = std::make_shared<std::vector<char>>(sizeof(gpupreagg_joined_map), 0);
	gpupreagg_joined_map *jm = (gpupreagg_joined_map *)img->data();
	jm->ncols = m.ncols;
	jm->key_col = m.key_col[0];
	jm->key_attlen = m.key_attlen[0];
	jm->nslots = m.nslots[0];
	jm->key_min = m.key_min[0];
	jm->recs = m.recs[0];
	jm->reclen = m.reclen[0];
	jm->narrow = m.narrow[0];
	jm->matches = m.matches;
	jm->unmatched_wgs = m.unmatched_wgs;
	for (int i = 0; i < m.ncols; i++)
	{
		jm->c[i].depth = m.c[i].depth;
		jm->c[i].col = m.c[i].col;
		jm->c[i].dimvalues = m.c[i].recoff;
		jm->c[i].dimisnull = m.c[i].nullbit;
		jm->nshift[i] = m.c[i].nshift;
		jm->nmask[i] = m.c[i].nmask;
		jm->nmin[i] = m.c[i].nmin;
	}
	return img;
}

/* ... and as gpupreagg_dense_lookup_star / _packed_lookup_star read it */
std::shared_ptr<std::vector<char>>
write_star_map(const fold_mapping &m)
{
	auto	img = std::make_shared<std::vector<char>>(sizeof(gpupreagg_star_map), 0);
	gpupreagg_star_map *sm = (gpupreagg_star_map *)img->data();
	sm->ncols = m.ncols;
	sm->nrels = m.nrels;
	for (int r = 0; r < m.nrels; r++)
	{
		sm->rel[r].key_col = m.key_col[r];
		sm->rel[r].key_attlen = m.key_attlen[r];
		sm->rel[r].nslots = m.nslots[r];
		sm->rel[r].reclen = m.reclen[r];
		sm->rel[r].key_min = m.key_min[r];
		sm->rel[r].recs = m.recs[r];
		sm->rel[r].narrow = m.narrow[r];
	}
	memcpy(sm->c, m.c, sizeof(sm->c[0]) * m.ncols);
	sm->matches = m.matches;
	return img;
}

}	/* namespace */

/*
 * The fused folds (strom_hip.h): the rows a finished GpuHashJoin produced, straight from its result
 * pairs (gpupreagg_dense_joined); the join as a lookup inside the aggregate's own pass over the outer chunk,
 * no join request at all (gpupreagg_dense_lookup); a star of such lookups, one table per relation
 * (gpupreagg_dense_lookup_star) -- and a snowflake, which is the lookup or the star it flattens to.  One launch
 * path: the request of a mapping, whichever builder described it.
 */
static strom_task *
launch_fused_fold(strom_gpupreagg *sess, preagg_kind entry, strom_task_impl *jtask, const fold_mapping &m,
				  strom_dstore *outer, strom_done_cb done, void *arg, int *p_errcode)
{
	preagg_request req;
	req.sess = sess;
	req.kds_dev = outer;
	req.format = KDS_FORMAT_COLUMN;
	req.nrows = (outer ? outer->head.nitems : 0);
	req.kind = entry;
	if (entry == PREAGG_UNMATCHED)
	{
		/* (m is the one-relation mapping of the tracked relation: its slots are the rows) */
		req.mapping_defs = unmatched_mapping_defines(m.reclen[0], m.narrow[0], m.inner_mask[0]);
		if (req.mapping_defs.empty())
		{
			*p_errcode = StromError_BadRequestMessage;
			return nullptr;
		}
		req.prog = program_with_defines(sess, req.mapping_defs);
		if (!req.prog)
		{
			*p_errcode = StromError_OutOfMemory;
			return nullptr;
		}
		req.map = write_joined_map(m);
		req.nrows = m.nslots[0];
	}
	else if (entry == PREAGG_STAR)
	{
		/* (a record longer than GPUPREAGG_STAR_MAXRECLEN, or more than GPUPREAGG_STAR_MAXRECBYTES over
		 * all relations: no define block -- the kernel keeps a row's records in registers) */
		req.mapping_defs = star_mapping_defines(m.nrels, m.key_attlen, m.reclen, m.narrow, m.inner_mask, m.jointype,
												m.tracked);
		if (req.mapping_defs.empty())
		{
			*p_errcode = StromError_BadRequestMessage;
			return nullptr;
		}
		req.prog = star_mapping_program(sess, req.mapping_defs);
		if (!req.prog)
		{
			*p_errcode = StromError_OutOfMemory;
			return nullptr;
		}
		req.map = write_star_map(m);
	}
	else if (entry == PREAGG_LOOKUP)
	{
		int		rc = 0;
		req.prog = lookup_mapping_program(sess, m, &req.mapping_defs, &rc);
		if (rc != 0)
		{
			*p_errcode = rc;
			return nullptr;
		}
		req.map = write_joined_map(m);
	}
	else
	{
		req.map = write_joined_map(m);
		req.nrows = jtask->res_nitems;
		req.joined_results = (const char *)jtask->main_devptr + jtask->res_offset;
		/* the result pairs now belong to this request: the join task can be
		 * waited for and released in any order */
		req.joined_buffer = jtask->main_devptr;
		jtask->main_devptr = nullptr;
		jtask->keep_main = false;
	}
	sess->nfolds++;
	strom_task_impl *task = task_create(sess->dev, done, arg);
	program_run_or_park(req.prog ? req.prog : sess->prog, [task, req]() { gpupreagg_launch(task, req); });
	return task;
}

/*
 * The session's matched flags for tracked relation 'pos' of a fold over 'tbl' (nslots slots): made on first
 * use, zeroed, and from then on bound to that table and position.  A table with a NULL-key entry is refused:
 * such an entry has no slot, the unmatched pass could never emit it, and the caller takes the join's RIGHT
 * path, which does.  for_fold: a chunk fold, which may not follow the unmatched pass without a reset; the
 * unmatched pass itself may not run twice.  Returns 0 and the flags' address, or the code to refuse with.
 */
static int
session_bind_matches(strom_gpupreagg *sess, strom_hashjoin_table *tbl, int pos, cl_uint nslots, bool for_fold,
					 cl_ulong *p_matches)
{
	uint64_t	serial = 0;
	cl_uint		null_keys = 0;
	int			rc = hashjoin_table_null_key_entries(tbl, &serial, &null_keys);
	if (rc != 0)
		return rc;
	if (null_keys != 0)
		return StromError_BadRequestMessage;
	std::lock_guard<std::mutex> g(sess->lock);
	if (sess->d_matches)
	{
		if (sess->matches_serial != serial || sess->matches_pos != pos || sess->matches_len != nslots ||
			sess->unmatched_done)
			return StromError_BadRequestMessage;
	}
	else
	{
		Device *dev = sess->dev;
		(void)hipSetDevice(dev->hip_id);
		char   *p = (char *)dev->pool.alloc(nslots);
		if (!p)
			return StromError_OutOfMemory;
		if (hipMemset(p, 0, nslots) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
		{
			dev->pool.release(p);
			return StromError_HipInternal;
		}
		sess->d_matches = p;
		sess->matches_len = nslots;
		sess->matches_serial = serial;
		sess->matches_pos = pos;
		sess->unmatched_done = false;
	}
	if (!for_fold)
		sess->unmatched_done = true;
	*p_matches = (cl_ulong)(uintptr_t)sess->d_matches;
	return 0;
}

/* _joined, _lookup and _lookup_star: build_fold_mapping, then the launch */
static strom_task *
submit_gpupreagg_fused(strom_gpupreagg *sess, preagg_kind entry, strom_task *join_handle,
					   strom_hashjoin_table *const *tbls, int ntbls, strom_dstore *outer,
					   int ncols, const int32_t *src_depth, const int32_t *src_colidx, const int32_t *type_oids,
					   strom_done_cb done, void *arg, int *p_errcode, const int32_t *jointypes = nullptr,
					   int tracked = 0)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	strom_task_impl *jtask = static_cast<strom_task_impl *>(join_handle);
	fold_mapping m;
	*p_errcode = build_fold_mapping(sess, entry, jtask, tbls, ntbls, outer, ncols, src_depth, src_colidx, type_oids, &m);
	if (*p_errcode != 0)
		return nullptr;
	for (int r = 0; jointypes && r < ntbls; r++)
		m.jointype[r] = jointypes[r];
	if (tracked != 0)
	{
		/* (a star's records must fit the kernel whatever is tracked: refuse before the flags are made) */
		if (entry == PREAGG_STAR &&
			star_mapping_defines(m.nrels, m.key_attlen, m.reclen, m.narrow, m.inner_mask, m.jointype, tracked).empty())
			*p_errcode = StromError_BadRequestMessage;
		else
			*p_errcode = session_bind_matches(sess, tbls[tracked - 1], tracked, m.nslots[tracked - 1], true, &m.matches);
		if (*p_errcode != 0)
			return nullptr;
		m.tracked = tracked;
	}
	return launch_fused_fold(sess, entry, jtask, m, outer, done, arg, p_errcode);
	STROM_ABI_CATCH(nullptr, p_errcode)
}

extern "C" strom_task *
strom_submit_gpupreagg_joined(strom_gpupreagg *sess, strom_task *join_handle,
							  strom_hashjoin_table *tbl, strom_dstore *outer,
							  int ncols, const int32_t *src_depth, const int32_t *src_colidx,
							  const int32_t *type_oids,
							  strom_done_cb done, void *arg, int *p_errcode)
{
	return submit_gpupreagg_fused(sess, PREAGG_JOINED, join_handle, &tbl, 1, outer, ncols, src_depth, src_colidx,
								  type_oids, done, arg, p_errcode);
}

extern "C" strom_task *
strom_submit_gpupreagg_lookup(strom_gpupreagg *sess,
							  strom_hashjoin_table *tbl, strom_dstore *outer,
							  int ncols, const int32_t *src_depth, const int32_t *src_colidx,
							  const int32_t *type_oids,
							  strom_done_cb done, void *arg, int *p_errcode)
{
	return submit_gpupreagg_fused(sess, PREAGG_LOOKUP, nullptr, &tbl, 1, outer, ncols, src_depth, src_colidx,
								  type_oids, done, arg, p_errcode);
}

extern "C" int
strom_gpupreagg_lookup_star_defines(int ntbls, const int32_t *keylen, const int32_t *reclen,
									const int32_t *narrow, const uint64_t *inner_mask,
									char *buf, size_t buflen)
{
	std::string	defs = star_mapping_defines(ntbls, keylen, reclen, narrow, inner_mask);
	if (defs.empty() || !buf || defs.size() + 1 > buflen)
		return -1;
	memcpy(buf, defs.c_str(), defs.size() + 1);
	return (int)defs.size();
}

extern "C" strom_task *
strom_submit_gpupreagg_lookup_star(strom_gpupreagg *sess,
								   strom_hashjoin_table *const *tbls, int ntbls, strom_dstore *outer,
								   int ncols, const int32_t *src_depth, const int32_t *src_colidx,
								   const int32_t *type_oids,
								   strom_done_cb done, void *arg, int *p_errcode)
{
	static_assert(STROM_LOOKUP_STAR_MAXRELS == GPUPREAGG_STAR_MAXRELS, "star relations");
	/* (one relation is the one-table call, its kernel and its error codes) */
	return submit_gpupreagg_fused(sess, (ntbls == 1 && tbls) ? PREAGG_LOOKUP : PREAGG_STAR, nullptr, tbls, ntbls, outer,
								  ncols, src_depth, src_colidx, type_oids, done, arg, p_errcode);
}

extern "C" int
strom_gpupreagg_lookup_typed_defines(int ntbls, const int32_t *keylen, const int32_t *reclen,
									 const int32_t *narrow, const uint64_t *inner_mask, const int32_t *jointypes,
									 char *buf, size_t buflen)
{
	if (ntbls < 1 || ntbls > GPUPREAGG_STAR_MAXRELS || !keylen || !reclen || !narrow || !inner_mask || !jointypes)
		return -1;
	/* (one relation: the one-table kernels' block, as the submit call builds it) */
	std::string	defs = (ntbls == 1 ? lookup_mapping_defines(keylen[0], reclen[0], narrow[0], inner_mask[0], jointypes[0])
							   : star_mapping_defines(ntbls, keylen, reclen, narrow, inner_mask, jointypes));
	if (defs.empty() || !buf || defs.size() + 1 > buflen)
		return -1;
	memcpy(buf, defs.c_str(), defs.size() + 1);
	return (int)defs.size();
}

extern "C" int
strom_gpupreagg_mapping_defines(strom_gpupreagg *sess, char *buf, size_t buflen)
{
	if (!sess)
		return -1;
	std::string	all;
	{
		std::lock_guard<std::mutex> g(sess->lock);
		for (auto &kv : sess->lookup_programs)
			all += kv.first + "\n";
	}
	if (buf && all.size() + 1 <= buflen)
		memcpy(buf, all.c_str(), all.size() + 1);
	else if (buf)
		return -1;
	return (int)all.size();
}

extern "C" strom_task *
strom_submit_gpupreagg_lookup_typed(strom_gpupreagg *sess,
									strom_hashjoin_table *const *tbls, int ntbls, const int32_t *jointypes,
									strom_dstore *outer,
									int ncols, const int32_t *src_depth, const int32_t *src_colidx,
									const int32_t *type_oids,
									strom_done_cb done, void *arg, int *p_errcode)
{
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	bool	typed = false;
	for (int r = 0; jointypes && r >= 0 && r < ntbls && r < GPUPREAGG_STAR_MAXRELS; r++)
		typed = typed || (jointypes[r] != 0);
	/* (all inner: the star call -- its code path, its error codes, its programs) */
	if (jointypes && !typed)
		return strom_submit_gpupreagg_lookup_star(sess, tbls, ntbls, outer, ncols, src_depth, src_colidx, type_oids,
												  done, arg, p_errcode);
	/* a join type outside 0 .. 3; a column asked of a relation that only filters (semi, anti) */
	bool	ok = (jointypes && ntbls >= 1 && ntbls <= GPUPREAGG_STAR_MAXRELS);
	for (int r = 0; ok && r < ntbls; r++)
		ok = (jointypes[r] >= 0 && jointypes[r] <= 3);
	for (int i = 0; ok && src_depth && i < ncols && i < GPUPREAGG_JOINED_MAXCOLS; i++)
		ok = !(src_depth[i] >= 1 && src_depth[i] <= ntbls && jointypes[src_depth[i] - 1] >= 2);
	if (!ok)
	{
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	return submit_gpupreagg_fused(sess, ntbls == 1 ? PREAGG_LOOKUP : PREAGG_STAR, nullptr, tbls, ntbls, outer,
								  ncols, src_depth, src_colidx, type_oids, done, arg, p_errcode, jointypes);
}

/* the checks of the tracked calls on top of the typed call's: join types 0 .. 3, no column under a semi or anti
 * relation, tracked 1 .. ntbls and that relation inner or left */
static bool
tracked_arguments_ok(int ntbls, const int32_t *jointypes, int tracked, int ncols, const int32_t *src_depth)
{
	bool	ok = (jointypes && ntbls >= 1 && ntbls <= GPUPREAGG_STAR_MAXRELS && tracked >= 1 && tracked <= ntbls);
	for (int r = 0; ok && r < ntbls; r++)
		ok = (jointypes[r] >= 0 && jointypes[r] <= 3);
	ok = ok && jointypes[tracked - 1] <= 1;
	for (int i = 0; ok && src_depth && i < ncols && i < GPUPREAGG_JOINED_MAXCOLS; i++)
		ok = !(src_depth[i] >= 1 && src_depth[i] <= ntbls && jointypes[src_depth[i] - 1] >= 2);
	return ok;
}

extern "C" int
strom_gpupreagg_lookup_tracked_defines(int ntbls, const int32_t *keylen, const int32_t *reclen,
									   const int32_t *narrow, const uint64_t *inner_mask, const int32_t *jointypes,
									   int tracked, char *buf, size_t buflen)
{
	if (tracked == 0)
		return strom_gpupreagg_lookup_typed_defines(ntbls, keylen, reclen, narrow, inner_mask, jointypes, buf, buflen);
	if (ntbls < 1 || ntbls > GPUPREAGG_STAR_MAXRELS || !keylen || !reclen || !narrow || !inner_mask || !jointypes ||
		tracked < 1 || tracked > ntbls)
		return -1;
	std::string	defs = (ntbls == 1 ? lookup_mapping_defines(keylen[0], reclen[0], narrow[0], inner_mask[0], jointypes[0], true)
						   : star_mapping_defines(ntbls, keylen, reclen, narrow, inner_mask, jointypes, tracked));
	if (defs.empty() || !buf || defs.size() + 1 > buflen)
		return -1;
	memcpy(buf, defs.c_str(), defs.size() + 1);
	return (int)defs.size();
}

extern "C" int
strom_gpupreagg_lookup_unmatched_defines(int reclen, int narrow, uint64_t inner_mask, char *buf, size_t buflen)
{
	std::string	defs = unmatched_mapping_defines(reclen, narrow, inner_mask);
	if (defs.empty() || !buf || defs.size() + 1 > buflen)
		return -1;
	memcpy(buf, defs.c_str(), defs.size() + 1);
	return (int)defs.size();
}

extern "C" strom_task *
strom_submit_gpupreagg_lookup_tracked(strom_gpupreagg *sess,
									  strom_hashjoin_table *const *tbls, int ntbls, const int32_t *jointypes,
									  int tracked, strom_dstore *outer,
									  int ncols, const int32_t *src_depth, const int32_t *src_colidx,
									  const int32_t *type_oids,
									  strom_done_cb done, void *arg, int *p_errcode)
{
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	/* (nothing tracked: the typed call -- its code path, its error codes, its programs) */
	if (tracked == 0)
		return strom_submit_gpupreagg_lookup_typed(sess, tbls, ntbls, jointypes, outer, ncols, src_depth, src_colidx,
												   type_oids, done, arg, p_errcode);
	if (!tracked_arguments_ok(ntbls, jointypes, tracked, ncols, src_depth))
	{
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	return submit_gpupreagg_fused(sess, ntbls == 1 ? PREAGG_LOOKUP : PREAGG_STAR, nullptr, tbls, ntbls, outer,
								  ncols, src_depth, src_colidx, type_oids, done, arg, p_errcode, jointypes, tracked);
}

extern "C" strom_task *
strom_submit_gpupreagg_lookup_unmatched(strom_gpupreagg *sess,
										strom_hashjoin_table *const *tbls, int ntbls, const int32_t *jointypes,
										int tracked,
										int ncols, const int32_t *src_depth, const int32_t *src_colidx,
										const int32_t *type_oids,
										strom_done_cb done, void *arg, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	if (!tracked_arguments_ok(ntbls, jointypes, tracked, ncols, src_depth))
	{
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	fold_mapping m;
	*p_errcode = build_fold_mapping(sess, PREAGG_UNMATCHED, nullptr, tbls, ntbls, nullptr, ncols, src_depth, src_colidx,
									type_oids, &m, tracked);
	if (*p_errcode != 0)
		return nullptr;
	/* the tracked relation alone, as a one-relation mapping: its records, its columns; every other column
	 * keeps depth and col for the record, and is NULL in the kernel */
	const int	t = tracked - 1;
	fold_mapping u = m;
	u.nrels = 1;
	u.key_col[0] = m.key_col[t];
	u.key_attlen[0] = 0;
	u.reclen[0] = m.reclen[t];
	u.narrow[0] = m.narrow[t];
	u.inner_mask[0] = m.inner_mask[t];
	u.key_min[0] = m.key_min[t];
	u.nslots[0] = m.nslots[t];
	u.recs[0] = m.recs[t];
	u.tracked = tracked;
	*p_errcode = session_bind_matches(sess, tbls[t], tracked, u.nslots[0], false, &u.matches);
	if (*p_errcode != 0)
		return nullptr;
	/* every fold of this table queued so far has set its flags before the pass reads them */
	(void)hipSetDevice(sess->dev->hip_id);
	if (hipDeviceSynchronize() != hipSuccess)
	{
		*p_errcode = StromError_HipInternal;
		return nullptr;
	}
	/* a cap on the work-groups that walk the slots (tests: one work-group walks many tiles); read on every call */
	if (const char *v = getenv("STROM_GPUPREAGG_UNMATCHED_MAX_GRID"))
		u.unmatched_wgs = (cl_uint)std::max(1, atoi(v) / (int)std::max<cl_uint>(1, sess->ctl.nsplits));
	return launch_fused_fold(sess, PREAGG_UNMATCHED, nullptr, u, nullptr, done, arg, p_errcode);
	STROM_ABI_CATCH(nullptr, p_errcode)
}

/* the flags of the session's tracked relation: the multi-GPU / multi-shard seam, and the reset of a rescan.
 * Each synchronises the device first (strom_hip.h). */
extern "C" size_t
strom_gpupreagg_lookup_matches_length(strom_gpupreagg *sess)
{
	if (!sess)
		return 0;
	std::lock_guard<std::mutex> g(sess->lock);
	return (sess->d_matches ? sess->matches_len : 0);
}

extern "C" int
strom_gpupreagg_lookup_matches_fetch(strom_gpupreagg *sess, void *buf, size_t len)
{
	if (!sess || !buf)
		return StromError_BadRequestMessage;
	std::lock_guard<std::mutex> g(sess->lock);
	if (!sess->d_matches || len != sess->matches_len)
		return StromError_BadRequestMessage;
	(void)hipSetDevice(sess->dev->hip_id);
	if (hipDeviceSynchronize() != hipSuccess ||
		hipMemcpy(buf, sess->d_matches, len, hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_HipInternal;
	return 0;
}

extern "C" int
strom_gpupreagg_lookup_matches_merge(strom_gpupreagg *sess, const void *buf, size_t len)
{
	STROM_ABI_TRY
	if (!sess || !buf)
		return StromError_BadRequestMessage;
	std::lock_guard<std::mutex> g(sess->lock);
	if (!sess->d_matches || len != sess->matches_len)
		return StromError_BadRequestMessage;
	const unsigned char *in = (const unsigned char *)buf;
	for (size_t i = 0; i < len; i++)
		if (in[i] > 1)
			return StromError_BadRequestMessage;		/* (no image of these flags: nothing is merged) */
	std::vector<unsigned char> mine(len);
	(void)hipSetDevice(sess->dev->hip_id);
	if (hipDeviceSynchronize() != hipSuccess ||
		hipMemcpy(mine.data(), sess->d_matches, len, hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_HipInternal;
	for (size_t i = 0; i < len; i++)
		mine[i] |= in[i];
	if (hipMemcpy(sess->d_matches, mine.data(), len, hipMemcpyHostToDevice) != hipSuccess)
		return StromError_HipInternal;
	return 0;
	STROM_ABI_CATCH(StromError_OutOfMemory, (int *)nullptr)
}

extern "C" int
strom_gpupreagg_lookup_reset_matches(strom_gpupreagg *sess)
{
	if (!sess)
		return StromError_BadRequestMessage;
	std::lock_guard<std::mutex> g(sess->lock);
	if (!sess->d_matches)
		return StromError_BadRequestMessage;
	(void)hipSetDevice(sess->dev->hip_id);
	if (hipDeviceSynchronize() != hipSuccess ||
		hipMemset(sess->d_matches, 0, sess->matches_len) != hipSuccess ||
		hipDeviceSynchronize() != hipSuccess)
		return StromError_HipInternal;
	sess->unmatched_done = false;
	return 0;
}

extern "C" int
strom_gpupreagg_lookup_snowflake_roots(int ntbls, const int32_t *parent, int ncols, const int32_t *src_depth,
									   int32_t *root_of, int32_t *col_root)
{
	/* relation d hangs on a fact column (parent 0: a root, numbered 1 .. in the order they come) or on a
	 * column of an EARLIER relation, whose root is then its own */
	int32_t		roots[STROM_LOOKUP_SNOWFLAKE_MAXRELS];
	int			nroots = 0;
	if (ntbls < 1 || ntbls > STROM_LOOKUP_SNOWFLAKE_MAXRELS || !parent || ncols < 0 || (ncols > 0 && !src_depth))
		return -1;
	for (int d = 1; d <= ntbls; d++)
	{
		if (parent[d - 1] < 0 || parent[d - 1] >= d)
			return -1;
		roots[d - 1] = (parent[d - 1] == 0 ? ++nroots : roots[parent[d - 1] - 1]);
	}
	if (nroots > STROM_LOOKUP_STAR_MAXRELS)
		return -1;
	for (int i = 0; i < ncols; i++)
	{
		if (src_depth[i] < 0 || src_depth[i] > ntbls)
			return -1;
		if (col_root)
			col_root[i] = (src_depth[i] == 0 ? 0 : roots[src_depth[i] - 1]);
	}
	if (root_of)
		memcpy(root_of, roots, sizeof(int32_t) * ntbls);
	return nroots;
}

extern "C" strom_task *
strom_submit_gpupreagg_lookup_snowflake(strom_gpupreagg *sess,
										strom_hashjoin_table *const *tbls, int ntbls,
										const int32_t *parent, const int32_t *link_type_oids,
										strom_dstore *outer,
										int ncols, const int32_t *src_depth, const int32_t *src_colidx,
										const int32_t *type_oids,
										strom_done_cb done, void *arg, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	if (!parent || ntbls < 1 || ntbls > STROM_LOOKUP_SNOWFLAKE_MAXRELS)
	{
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	/* (no relation hangs on another: the star call, one relation: the one-table call -- their code
	 * paths and their error codes) */
	bool	star = true;
	for (int d = 1; d <= ntbls; d++)
		star = star && (parent[d - 1] == 0);
	if (star)
		return strom_submit_gpupreagg_lookup_star(sess, tbls, ntbls, outer, ncols, src_depth, src_colidx, type_oids,
												  done, arg, p_errcode);
	fold_mapping m;
	*p_errcode = build_snowflake_mapping(sess, tbls, ntbls, parent, link_type_oids, outer, ncols, src_depth, src_colidx,
										 type_oids, &m);
	if (*p_errcode != 0)
		return nullptr;
	return launch_fused_fold(sess, m.nrels == 1 ? PREAGG_LOOKUP : PREAGG_STAR, nullptr, m, outer, done, arg, p_errcode);
	STROM_ABI_CATCH(nullptr, p_errcode)
}

/*
 * census / compact: see gpupreagg_census in strom_gpupreagg.h.  Both are
 * planning-time calls (blocking); they must precede the first fold.
 */
extern "C" int
strom_gpupreagg_census(strom_gpupreagg *sess,
					   const kern_data_store *kds, strom_dstore *kds_dev,
					   const kern_row_map *krowmap,
					   uint32_t *bitmap_out, size_t nwords)
{
	if (!sess || !sess->has_domain || (!kds) == (!kds_dev))
		return StromError_BadRequestMessage;
	if (sess->ctl.remap != 0)
		return StromError_BadRequestMessage;		/* already compacted */
	Device *dev = sess->dev;
	if (kds_dev && kds_dev->dindex != dev->dindex)
		return StromError_BadRequestMessage;
	size_t	words = ((size_t)sess->ctl.dense_ngroups + 31) / 32;
	if (bitmap_out && nwords < words)
		return StromError_DataStoreNoSpace;
	if (!program_accepts_format(sess->prog, kds ? kds->format : kds_dev->head.format))
		return StromError_BadRequestMessage;
	if (strom_lookup_device_program(sess->key, 1) != STROM_DEVPROG_READY)
		return StromError_ProgramBuildFailure;
	std::lock_guard<std::mutex> g(sess->lock);
	(void)hipSetDevice(dev->hip_id);
	hipStream_t stream = dev->streams[0];
	int		errcode = 0;
	hipFunction_t fn = sess->prog->get_function(dev, "gpupreagg_census", &errcode);
	if (!fn)
		return errcode;
	if (!sess->d_census)
	{
		sess->d_census = (char *)dev->pool.alloc(words * sizeof(cl_uint));
		if (!sess->d_census)
			return StromError_OutOfMemory;
		if (hipMemsetAsync(sess->d_census, 0, words * sizeof(cl_uint), stream) != hipSuccess)
			return StromError_HipInternal;
	}
	size_t	kg_len = STROMALIGN(offsetof(kern_gpupreagg, kparams) + sess->kparams.size());
	std::vector<char> kg(kg_len, 0);
	memcpy(kg.data() + offsetof(kern_gpupreagg, kparams), sess->kparams.data(), sess->kparams.size());
	char   *d_kg = (char *)dev->pool.alloc(kg_len);
	void   *d_chunk = nullptr, *d_map = nullptr;
	int		rc = 0;
	do {
		if (!d_kg || hipMemcpyAsync(d_kg, kg.data(), kg_len, hipMemcpyHostToDevice, stream) != hipSuccess)
		{
			rc = StromError_OutOfMemory;
			break;
		}
		const void *a_kds = (kds_dev ? kds_dev->devptr : nullptr);
		cl_uint	nrows;
		if (kds)
		{
			size_t	len = kds->length;
			if (kds->format == KDS_FORMAT_ROW)
				len = KERN_DATA_STORE_ROWBLOCK_OFFSET(kds) + (size_t)BLCKSZ * kds->nblocks;
			d_chunk = dev->pool.alloc(len);
			if (!d_chunk || hipMemcpyAsync(d_chunk, kds, len, hipMemcpyHostToDevice, stream) != hipSuccess)
			{
				rc = StromError_OutOfMemory;
				break;
			}
			a_kds = d_chunk;
			nrows = kds->nitems;
		}
		else
			nrows = kds_dev->head.nitems;
		const void *a_map = nullptr;
		if (krowmap && krowmap->nvalids >= 0)
		{
			size_t	len = offsetof(kern_row_map, rindex) + sizeof(cl_int) * (size_t)krowmap->nvalids;
			d_map = dev->pool.alloc(len);
			if (!d_map || hipMemcpyAsync(d_map, krowmap, len, hipMemcpyHostToDevice, stream) != hipSuccess)
			{
				rc = StromError_OutOfMemory;
				break;
			}
			a_map = d_map;
			nrows = (cl_uint)krowmap->nvalids;
		}
		const void *a_kg = d_kg;
		const void *a_toast = nullptr;
		const void *a_ctl = sess->d_ctl;
		void	   *a_bitmap = sess->d_census;
		void	   *args[] = { &a_kg, &a_kds, &a_toast, &a_map, &a_ctl, &a_bitmap };
		unsigned	grid = (unsigned)std::min<size_t>(((size_t)nrows + 255) / 256,
													  (size_t)dev->prop.multiProcessorCount * 8);
		if (grid > 0 &&
			hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, stream, args, nullptr) != hipSuccess)
		{
			rc = StromError_HipInternal;
			break;
		}
		if (bitmap_out &&
			hipMemcpyAsync(bitmap_out, sess->d_census, words * sizeof(cl_uint),
						   hipMemcpyDeviceToHost, stream) != hipSuccess)
			rc = StromError_HipInternal;
	} while (0);
	if (hipStreamSynchronize(stream) != hipSuccess && rc == 0)
		rc = StromError_HipInternal;
	if (d_kg) dev->pool.release(d_kg);
	if (d_chunk) dev->pool.release(d_chunk);
	if (d_map) dev->pool.release(d_map);
	return rc;
}

extern "C" int
strom_gpupreagg_compact(strom_gpupreagg *sess, const uint32_t *bitmap, size_t nwords)
{
	if (!sess || !sess->has_domain || sess->nfolds != 0 || !sess->table_owned || sess->ctl.remap != 0)
		return StromError_BadRequestMessage;
	Device *dev = sess->dev;
	gpupreagg_dense_ctl &ctl = sess->ctl;
	size_t	words = ((size_t)ctl.dense_ngroups + 31) / 32;
	std::vector<cl_uint> bits(words, 0);
	std::lock_guard<std::mutex> g(sess->lock);

	(void)hipSetDevice(dev->hip_id);
	if (bitmap)
	{
		if (nwords < words)
			return StromError_BadRequestMessage;
		memcpy(bits.data(), bitmap, words * sizeof(cl_uint));
	}
	else if (sess->d_census)
	{
		if (session_quiesce(sess) != hipSuccess ||
			hipMemcpy(bits.data(), sess->d_census, words * sizeof(cl_uint), hipMemcpyDeviceToHost) != hipSuccess)
			return StromError_HipInternal;
	}
	std::vector<cl_uint> remap(ctl.dense_ngroups, 0xffffffffu);
	sess->present.clear();
	for (cl_uint d = 0; d < ctl.dense_ngroups; d++)
		if (bits[d >> 5] & (1u << (d & 31)))
		{
			remap[d] = (cl_uint)sess->present.size();
			sess->present.push_back(d);
		}
	if (sess->present.empty())
	{
		/* nothing passes the qual: keep one (never used) slot */
		sess->present.push_back(0);
	}
	sess->d_remap = (char *)dev->pool.alloc(remap.size() * sizeof(cl_uint));
	if (!sess->d_remap)
		return StromError_OutOfMemory;
	if (hipMemcpy(sess->d_remap, remap.data(), remap.size() * sizeof(cl_uint), hipMemcpyHostToDevice) != hipSuccess)
		return StromError_HipInternal;
	/* new table geometry over the compact slots */
	if (sess->table) dev->pool.release(sess->table);
	if (sess->d_ctl) dev->pool.release(sess->d_ctl);
	if (sess->d_slabs) dev->pool.release(sess->d_slabs);
	sess->table = sess->d_ctl = sess->d_slabs = nullptr;
	if (sess->d_export_spec)
	{
		dev->pool.release(sess->d_export_spec);
		sess->d_export_spec = nullptr;
	}
	ctl.ngroups = (cl_uint)sess->present.size();
	ctl.remap = (cl_ulong)(uintptr_t)sess->d_remap;
	int rc = setup_layout(sess);
	if (rc == 0)
		rc = alloc_session_buffers(sess);
	return rc;
}

/* what parallel.cpp needs to all-reduce the resident table in place */
bool
strom::gpupreagg_is_hashed(strom_gpupreagg *sess, int *p_dindex)
{
	if (!sess || !sess->hashed)
		return false;
	if (p_dindex)
		*p_dindex = sess->dev->dindex;
	return true;
}

/* the groups of a hashed session packed on the device: { knull, flags, keys[], vals[] } each */
int
strom::gpupreagg_hash_export_device(strom_gpupreagg *sess, char **p_recs, cl_uint *p_count, size_t *p_reclen,
									cl_ulong *p_sum_bound)
{
	Device *dev = sess->dev;
	size_t	reclen = GPUPREAGG_EXPORT_RECLEN(sess->key_resno.size(), sess->agg_resno.size());
	cl_uint	ngroups = 0, overflow = 0;
	std::lock_guard<std::mutex> g(sess->lock);

	*p_recs = nullptr;
	*p_count = 0;
	*p_reclen = reclen;
	if (p_sum_bound)
		*p_sum_bound = 0;
	(void)hipSetDevice(dev->hip_id);
	if (!sess->htab)
		return 0;
	int rc = hash_table_ngroups(sess, &ngroups, &overflow);
	if (rc == 0 && p_sum_bound)
		rc = hash_sum_measured_bound(sess, p_sum_bound);
	if (rc)
		return rc;
	if (overflow)
		return StromError_DataStoreNoSpace;
	if (ngroups == 0)
		return 0;
	int		errcode = 0;
	hipFunction_t fn = sess->prog->get_function(dev, "gpupreagg_hash_export", &errcode);
	if (!fn)
		return errcode;
	char   *d_out = (char *)dev->pool.alloc(reclen * ngroups + 16);
	if (!d_out)
		return StromError_OutOfMemory;
	char   *d_counter = d_out + reclen * ngroups;
	const void *a_tab = sess->htab;
	void	   *a_out = d_out, *a_cnt = d_counter;
	void	   *args[] = { &a_tab, &a_out, &a_cnt };
	unsigned	grid = std::min<unsigned>((sess->hash_capacity + 255) / 256, (unsigned)dev->prop.multiProcessorCount * 8);
	cl_uint		count = 0;
	bool ok = (hipMemsetAsync(d_counter, 0, 16, dev->streams[0]) == hipSuccess &&
			   hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, dev->streams[0], args, nullptr) == hipSuccess &&
			   hipStreamSynchronize(dev->streams[0]) == hipSuccess &&
			   hipMemcpy(&count, d_counter, sizeof(count), hipMemcpyDeviceToHost) == hipSuccess &&
			   count == ngroups);
	if (!ok)
	{
		dev->pool.release(d_out);
		return StromError_HipInternal;
	}
	*p_recs = d_out;
	*p_count = ngroups;
	return 0;
}

/*
 * ... packed by owner for the hash-partitioned exchange (devlib: gpupreagg_hash_export_parts): the
 * records of owner p are h_counts[p] records starting at record sum(h_counts[0 .. p)).
 */
int
strom::gpupreagg_hash_export_parts_device(strom_gpupreagg *sess, cl_uint nparts, char **p_recs, cl_uint *h_counts,
										  size_t *p_reclen, cl_ulong *p_sum_bound)
{
	Device *dev = sess->dev;
	size_t	reclen = GPUPREAGG_EXPORT_RECLEN(sess->key_resno.size(), sess->agg_resno.size());
	cl_uint	ngroups = 0, overflow = 0;
	std::lock_guard<std::mutex> g(sess->lock);

	*p_recs = nullptr;
	*p_reclen = reclen;
	*p_sum_bound = 0;
	for (cl_uint p = 0; p < nparts; p++)
		h_counts[p] = 0;
	if (nparts < 1 || nparts > 64)
		return StromError_BadRequestMessage;
	(void)hipSetDevice(dev->hip_id);
	if (!sess->htab)
		return 0;
	int rc = hash_table_ngroups(sess, &ngroups, &overflow);
	if (rc == 0)
		rc = hash_sum_measured_bound(sess, p_sum_bound);
	if (rc)
		return rc;
	if (overflow)
		return StromError_DataStoreNoSpace;
	if (ngroups == 0)
		return 0;
	int		errcode = 0;
	hipFunction_t fn_count = sess->prog->get_function(dev, "gpupreagg_hash_owner_count", &errcode);
	hipFunction_t fn_parts = fn_count ? sess->prog->get_function(dev, "gpupreagg_hash_export_parts", &errcode) : nullptr;
	if (!fn_parts)
		return errcode;
	/* behind the records: counts, offsets, cursors (nparts words each) */
	size_t	words_at = STROM_TYPEALIGN(16, reclen * ngroups);
	char   *d_out = (char *)dev->pool.alloc(words_at + 3 * sizeof(cl_uint) * 64);
	if (!d_out)
		return StromError_OutOfMemory;
	cl_uint	   *d_counts = (cl_uint *)(d_out + words_at);
	cl_uint	   *d_offsets = d_counts + 64, *d_cursors = d_counts + 128;
	hipStream_t	stream = dev->streams[0];
	const void *a_tab = sess->htab;
	void	   *a_out = d_out, *a_cnt = d_counts, *a_off = d_offsets, *a_cur = d_cursors;
	void	   *args_count[] = { &a_tab, &nparts, &a_cnt };
	void	   *args_parts[] = { &a_tab, &a_out, &nparts, &a_off, &a_cur };
	unsigned	grid = std::min<unsigned>((sess->hash_capacity + 255) / 256, (unsigned)dev->prop.multiProcessorCount * 8);
	cl_uint		offsets[64], total = 0;
	bool ok = (hipMemsetAsync(d_counts, 0, 3 * sizeof(cl_uint) * 64, stream) == hipSuccess &&
			   hipModuleLaunchKernel(fn_count, grid, 1, 1, 256, 1, 1, 0, stream, args_count, nullptr) == hipSuccess &&
			   hipMemcpyAsync(h_counts, d_counts, sizeof(cl_uint) * nparts, hipMemcpyDeviceToHost, stream) == hipSuccess &&
			   hipStreamSynchronize(stream) == hipSuccess);
	for (cl_uint p = 0; ok && p < nparts; p++)
	{
		offsets[p] = total;
		total += h_counts[p];
	}
	ok = ok && total == ngroups &&
		hipMemcpyAsync(d_offsets, offsets, sizeof(cl_uint) * nparts, hipMemcpyHostToDevice, stream) == hipSuccess &&
		hipModuleLaunchKernel(fn_parts, grid, 1, 1, 256, 1, 1, 0, stream, args_parts, nullptr) == hipSuccess &&
		hipStreamSynchronize(stream) == hipSuccess;
	if (!ok)
	{
		dev->pool.release(d_out);
		return StromError_HipInternal;
	}
	*p_recs = d_out;
	return 0;
}

void
strom::gpupreagg_hash_release(strom_gpupreagg *sess, char *recs)
{
	if (recs)
		sess->dev->pool.release(recs);
}

/* packed groups (nsegs segments of seg_len records, h_counts[seg] of them set) into the table */
/*
 * incoming_sum_bound: the sum over the segments of "largest |integer sum| + 1" of the tables the
 * records come from (gpupreagg_hash_export*_device), or 0 when no incoming group can meet a group
 * of this table or another segment (disjoint keys).  The import adds 64-bit sums with plain
 * atomics: it runs only when this table's own bound plus the incoming one stays below 2^63 --
 * no group's sum can then leave int8 -- and answers CpuReCheck, before anything is touched,
 * otherwise (integer sums never wrap: strom_gpupreagg.h).
 */
int
strom::gpupreagg_hash_import_device(strom_gpupreagg *sess, const char *d_recs, cl_uint seg_len, cl_uint nsegs,
									const cl_uint *h_counts, cl_uint skip_seg, cl_ulong incoming_sum_bound)
{
	Device *dev = sess->dev;
	std::lock_guard<std::mutex> g(sess->lock);
	cl_ulong	incoming = 0;

	for (cl_uint s = 0; s < nsegs; s++)
		incoming += (s == skip_seg ? 0 : h_counts[s]);
	if (incoming == 0)
		return 0;
	(void)hipSetDevice(dev->hip_id);
	if (incoming_sum_bound == GPUPREAGG_IMPORT_EXACT && sess->nintsums != 0 && sess->htab)
	{
		/* one segment of pairwise different keys: group by group (gpupreagg_hash_import_verify) */
		int		e2 = 0;
		hipFunction_t fn_verify = sess->prog->get_function(dev, "gpupreagg_hash_import_verify", &e2);
		if (!fn_verify)
			return e2;
		if (nsegs != 1 || skip_seg != ~0u)
			return StromError_BadRequestMessage;
		cl_uint	   *d_flag = (cl_uint *)dev->pool.alloc(sizeof(cl_uint));
		if (!d_flag)
			return StromError_OutOfMemory;
		void	   *a_tab = sess->htab;
		const void *a_recs = d_recs;
		cl_uint		a_count = h_counts[0], flag = 0;
		void	   *a_flag = d_flag;
		void	   *vargs[] = { &a_tab, &a_recs, &a_count, &a_flag };
		unsigned	vgrid = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)a_count + 255) / 256,
																			(size_t)dev->prop.multiProcessorCount * 8));
		bool	vok = (hipMemsetAsync(d_flag, 0, sizeof(cl_uint), dev->streams[0]) == hipSuccess &&
					   hipModuleLaunchKernel(fn_verify, vgrid, 1, 1, 256, 1, 1, 0, dev->streams[0], vargs, nullptr) == hipSuccess &&
					   hipMemcpyAsync(&flag, d_flag, sizeof(cl_uint), hipMemcpyDeviceToHost, dev->streams[0]) == hipSuccess &&
					   hipStreamSynchronize(dev->streams[0]) == hipSuccess);
		dev->pool.release(d_flag);
		if (!vok)
			return StromError_HipInternal;
		if (flag)
			return StromError_CpuReCheck;
	}
	else if (incoming_sum_bound != 0 && incoming_sum_bound != GPUPREAGG_IMPORT_EXACT && sess->nintsums != 0)
	{
		cl_ulong	mine = 0;
		int			brc = hash_sum_measured_bound(sess, &mine);
		if (brc)
			return brc;
		if (incoming_sum_bound >= (1UL << 63) || mine >= (1UL << 63) || mine + incoming_sum_bound >= (1UL << 63))
			return StromError_CpuReCheck;
	}
	int		errcode = 0;
	hipFunction_t fn = sess->prog->get_function(dev, "gpupreagg_hash_import", &errcode);
	if (!fn)
		return errcode;
	/* room for every incoming group, should all of them be new */
	cl_uint		ngroups = 0;
	int			rc = 0;
	if (!sess->htab)
		rc = hash_table_new(sess, sess->hash_capacity, &sess->htab, &sess->htab_bytes, nullptr);
	if (rc == 0)
		rc = hash_table_ngroups(sess, &ngroups, nullptr);
	if (rc == 0 && ((cl_ulong)ngroups + incoming) * 8 / 7 + 4096 > sess->hash_capacity)
		rc = hash_table_grow(sess, ((cl_ulong)ngroups + incoming) * 2 + 4096);
	if (rc)
		return rc;
	cl_uint	   *d_counts = (cl_uint *)dev->pool.alloc(sizeof(cl_uint) * nsegs);
	if (!d_counts)
		return StromError_OutOfMemory;
	void	   *a_tab = sess->htab;
	const void *a_recs = d_recs;
	const void *a_counts = d_counts;
	void	   *args[] = { &a_tab, &a_recs, &seg_len, &nsegs, &a_counts, &skip_seg };
	size_t		total = (size_t)seg_len * nsegs;
	unsigned	grid = (unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, (size_t)dev->prop.multiProcessorCount * 8));
	bool ok = (hipMemcpy(d_counts, h_counts, sizeof(cl_uint) * nsegs, hipMemcpyHostToDevice) == hipSuccess &&
			   hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, dev->streams[0], args, nullptr) == hipSuccess &&
			   hipStreamSynchronize(dev->streams[0]) == hipSuccess);
	dev->pool.release(d_counts);
	if (!ok)
		return StromError_HipInternal;
	/* groups arrived otherwise than by a fold: the integer sums' bound is measured anew */
	rc = hash_sum_refresh(sess);
	if (rc)
		return rc;
	cl_uint		overflow = 0;
	rc = hash_table_ngroups(sess, &ngroups, &overflow);
	if (rc == 0)
	{
		sess->groups_upper = ngroups;
		sess->groups_known = std::max<cl_uint>(sess->groups_known, ngroups);
		if (overflow)
			rc = StromError_DataStoreNoSpace;
	}
	return rc;
}

int
strom::gpupreagg_get_merge_plan(strom_gpupreagg *sess, gpupreagg_merge_plan *plan)
{
	if (!sess || sess->hashed || !sess->has_domain || !sess->table || sess->agg_resno.size() > PREAGG_MERGE_MAXAGGS ||
		sess->numeric_aggs)				/* (64-bit numerics do not add up with ncclSum: gather the partial rows) */
		return StromError_BadRequestMessage;
	memset(&plan->spec, 0, sizeof(plan->spec));
	plan->spec.ngroups = sess->ctl.ngroups;
	plan->spec.naggs = (cl_uint)sess->agg_resno.size();
	for (size_t a = 0; a < sess->agg_resno.size(); a++)
	{
		const strom_preagg_target &t = sess->targets[sess->agg_resno[a]];
		bool	isfloat = type_is_float(t.type_oid);
		cl_uint	op;
		switch (t.kind)
		{
			case STROM_PREAGG_NROWS:	op = 0; break;
			case STROM_PREAGG_PSUM:		op = (isfloat ? 2 : 1); break;
			case STROM_PREAGG_PMIN:		op = (isfloat ? 5 : 3); break;
			case STROM_PREAGG_PMAX:		op = (isfloat ? 6 : 4); break;
			default:					return StromError_BadRequestMessage;
		}
		plan->spec.op[a] = op;
		plan->spec.vals_off[a] = gpupreagg_table_offset(1 + (int)a, sess->ctl.ngroups);
		if (sess->is_intsum((int)a))
		{
			/* 128 bits wide in the table: travels as three carry-free limbs (strom_merge.h) */
			plan->spec.hi_off[a] = sess->table_hi_offset((int)a, sess->ctl.ngroups);
			plan->spec.mid_idx[a] = (cl_uint)sess->intsum_of[a];
		}
	}
	plan->table = sess->table;
	plan->table_bytes = sess->table_bytes;
	plan->nmid = (cl_uint)sess->nintsums;
	plan->dindex = sess->dev->dindex;
	return 0;
}

bool
strom::gpupreagg_sessions_mergeable(strom_gpupreagg *dst, strom_gpupreagg *src)
{
	if (!dst || !src || dst == src || dst->dev != src->dev || dst->prog != src->prog ||
		dst->hashed != src->hashed || dst->targets.size() != src->targets.size())
		return false;
	for (size_t i = 0; i < dst->targets.size(); i++)
		if (dst->targets[i].kind != src->targets[i].kind || dst->targets[i].type_oid != src->targets[i].type_oid ||
			dst->targets[i].scale != src->targets[i].scale)
			return false;
	if (dst->hashed)
		return true;
	/* dense tables: slot i must be the same group in both */
	const gpupreagg_dense_ctl &a = dst->ctl, &b = src->ctl;
	if (!dst->has_domain || !src->has_domain || a.ngroups != b.ngroups || a.nkeys != b.nkeys ||
		a.dense_ngroups != b.dense_ngroups || dst->present != src->present)
		return false;
	for (cl_uint k = 0; k < a.nkeys; k++)
		if (a.key_min[k] != b.key_min[k] || a.key_range[k] != b.key_range[k] || a.key_stride[k] != b.key_stride[k])
			return false;
	return true;
}

int
strom::gpupreagg_get_census(strom_gpupreagg *sess, void **p_bitmap, cl_uint *p_nbits, int *p_dindex)
{
	if (!sess || sess->hashed || !sess->has_domain || sess->ctl.remap != 0)
		return StromError_BadRequestMessage;
	if (!sess->d_census)
	{
		/* a rank without rows still takes part in the union */
		size_t	words = ((size_t)sess->ctl.dense_ngroups + 31) / 32;
		std::lock_guard<std::mutex> g(sess->lock);
		(void)hipSetDevice(sess->dev->hip_id);
		sess->d_census = (char *)sess->dev->pool.alloc(words * sizeof(cl_uint));
		if (!sess->d_census)
			return StromError_OutOfMemory;
		if (hipMemset(sess->d_census, 0, words * sizeof(cl_uint)) != hipSuccess)
			return StromError_HipInternal;
	}
	*p_bitmap = sess->d_census;
	*p_nbits = sess->ctl.dense_ngroups;
	*p_dindex = sess->dev->dindex;
	return 0;
}

extern "C" void
strom_gpupreagg_reset(strom_gpupreagg *sess)
{
	if (sess && sess->hashed)
	{
		std::lock_guard<std::mutex> g(sess->lock);
		(void)hipSetDevice(sess->dev->hip_id);
		if (sess->htab)
			(void)hash_table_new(sess, sess->hash_capacity, &sess->htab, &sess->htab_bytes, sess->htab);
		sess->groups_upper = 0;
		sess->groups_known = 0;
		return;
	}
	if (!sess || !sess->table)
		return;
	(void)hipSetDevice(sess->dev->hip_id);
	(void)session_quiesce(sess);
	(void)hipMemset(sess->table, 0, sess->table_bytes);
}

extern "C" void
strom_gpupreagg_release(strom_gpupreagg *sess)
{
	if (!sess)
		return;
	Device *dev = sess->dev;
	(void)hipSetDevice(dev->hip_id);
	(void)session_quiesce(sess);
	if (sess->table_owned && sess->table)
		dev->pool.release(sess->table);
	if (sess->d_ctl)
		dev->pool.release(sess->d_ctl);
	if (sess->d_slabs)
		dev->pool.release(sess->d_slabs);
	if (sess->d_census)
		dev->pool.release(sess->d_census);
	if (sess->d_remap)
		dev->pool.release(sess->d_remap);
	if (sess->d_export_spec)
		dev->pool.release(sess->d_export_spec);
	if (sess->d_matches)
		dev->pool.release(sess->d_matches);
	for (auto &kv : sess->packed)
	{
		dev->pool.release(kv.second.d_ctl);
		dev->pool.release(kv.second.d_slabs);
	}
	for (int b = 0; b < 2; b++)
		if (sess->merge_ev[b])
			(void)hipEventDestroy(sess->merge_ev[b]);
	if (sess->htab)
		dev->pool.release(sess->htab);
	for (auto &kv : sess->lookup_programs)
		strom_put_devprog_key(kv.second.first);
	strom_put_devprog_key(sess->key);
	delete sess;
}

namespace {

/* int64 fixed point at 10^-scale -> 64-bit device numeric; false when the
 * mantissa does not fit 57 bits */
bool
fixed_to_numeric(cl_long v, int scale, cl_ulong *out)
{
	bool		sign = (v < 0);
	cl_ulong	mant = (sign ? (cl_ulong)0 - (cl_ulong)v : (cl_ulong)v);
	int			expo = -scale;

	if (mant == 0)
	{
		*out = 0;
		return true;
	}
	while (mant % 10 == 0 && expo < 31)
	{
		mant /= 10;
		expo++;
	}
	if (mant >= (1UL << 57) || expo < -32 || expo > 31)
		return false;
	*out = (((cl_ulong)(cl_long)expo) << 58) | (sign ? (1UL << 57) : 0) | mant;
	return true;
}

struct numeric_spill {
	cl_uint		gid;
	int			resno;
	cl_ulong	image;
};

/*
 * An integer sum of the resident table is 128 bits wide {lo, hi} (strom_gpupreagg.h:
 * "integer sums never wrap"); a partial row carries an int8, or a 64-bit numeric with a
 * 57-bit mantissa.  A total that does not fit leaves as SEVERAL partial rows of its group --
 * partial rows add up, so the final aggregate is unchanged: datum images of the pieces, the
 * first for the group's own row.  int8: pieces of +-(2^63 - 1); numeric at 10^-scale: the
 * total's base-10^17 digits (each a 57-bit mantissa with its own exponent).
 */
int
sum_pieces(const strom_preagg_target &t, cl_ulong lo, cl_long hi, std::vector<cl_ulong> &out)
{
	__int128	total = ((__int128)hi << 64) | (__int128)(unsigned __int128)lo;
	out.clear();
	if (t.type_oid != STROM_NUMERICOID)
	{
		const __int128 most = (__int128)INT64_MAX;
		for (int n = 0; ; n++)
		{
			if (n == 4096)
				return StromError_DataStoreOutOfRange;	/* (a total beyond 2^75: not a sum of int8 rows) */
			if (total >= -most - 1 && total <= most)
			{
				out.push_back((cl_ulong)(cl_long)total);
				return 0;
			}
			cl_long piece = (total > 0 ? INT64_MAX : -INT64_MAX);
			out.push_back((cl_ulong)piece);
			total -= piece;
		}
	}
	bool		neg = (total < 0);
	unsigned __int128 mag = (neg ? (unsigned __int128)0 - (unsigned __int128)total : (unsigned __int128)total);
	cl_ulong	img;
	if (mag < ((unsigned __int128)1 << 63) &&
		fixed_to_numeric(neg ? -(cl_long)(cl_ulong)mag : (cl_long)(cl_ulong)mag, t.scale, &img))
	{
		out.push_back(img);
		return 0;
	}
	const cl_ulong P17 = 100000000000000000UL;
	for (int k = 0; mag != 0; k++)
	{
		cl_long		digit = (cl_long)(cl_ulong)(mag % P17);
		mag /= P17;
		if (digit == 0 && !(mag == 0 && out.empty()))
			continue;
		/* digit x 10^(17k) at 10^-scale = digit at 10^-(scale - 17k) */
		if (!fixed_to_numeric(neg ? -digit : digit, t.scale - 17 * k, &img))
			return StromError_DataStoreOutOfRange;
		out.push_back(img);
	}
	if (out.empty())
		out.push_back(0);
	return 0;
}

}	/* namespace */

namespace {

void
fetch_init_head(strom_gpupreagg *sess, kern_data_store *dest, size_t need, size_t nrooms)
{
	int		ncols = (int)sess->targets.size();
	memset(dest, 0, KDS_HEAD_LENGTH(ncols));
	dest->hostptr = (hostptr_t)(uintptr_t)&dest->hostptr;
	dest->length = (cl_uint)need;
	dest->ncols = ncols;
	dest->nrooms = (cl_uint)nrooms;
	dest->format = KDS_FORMAT_TUPSLOT;
	dest->tdtypeid = 2249;
	dest->tdtypmod = -1;
	for (int i = 0; i < ncols; i++)
	{
		const strom_preagg_target &t = sess->targets[i];
		int len = (t.kind == STROM_PREAGG_NROWS ? 8 : type_length(t.type_oid));
		dest->colmeta[i].attbyval = 1;
		dest->colmeta[i].attalign = (cl_char)len;
		dest->colmeta[i].attlen = (cl_short)len;
		dest->colmeta[i].attnum = (cl_short)(i + 1);
		dest->colmeta[i].attcacheoff = -1;
	}
}

/* a float accumulator image -> the column's datum */
cl_ulong
float_image_to_datum(const strom_preagg_target &t, cl_ulong raw, bool ordered)
{
	if (ordered)		/* order-preserving key -> IEEE bits */
		raw = (raw & 0x8000000000000000UL) ? (raw & 0x7fffffffffffffffUL) : ~raw;
	if (t.type_oid == STROM_FLOAT4OID)
	{
		double d; float f;
		memcpy(&d, &raw, 8);
		f = (float)d;
		raw = 0;
		memcpy(&raw, &f, 4);
	}
	return raw;
}

/*
 * hashed sessions: gpupreagg_hash_export packs the groups on the device,
 * only ngroups records cross PCIe
 */
long
gpupreagg_fetch_hashed(strom_gpupreagg *sess, kern_data_store *dest, size_t destlen)
{
	Device *dev = sess->dev;
	int		ncols = (int)sess->targets.size();
	size_t	nkeys = sess->key_resno.size(), naggs = sess->agg_resno.size();
	size_t	reclen = GPUPREAGG_EXPORT_RECLEN(nkeys, naggs);
	cl_uint	ngroups = 0, overflow = 0;
	std::vector<char> recs;
	std::lock_guard<std::mutex> g(sess->lock);

	(void)hipSetDevice(dev->hip_id);
	if (sess->htab)
	{
		int rc = hash_table_ngroups(sess, &ngroups, &overflow);
		if (rc)
			return -rc;
		if (overflow)
			return -StromError_DataStoreNoSpace;
	}
	/*
	 * No 64-bit numeric partial (those may leave as two rows: the host decides): the rows are
	 * formatted on the device and cross PCIe once, into the caller's buffer.  The host loop
	 * below took 56 ms for 1e6 groups, and asking for the size ran all of it too.
	 */
	bool	any_numeric = false;
	for (size_t a = 0; a < naggs; a++)
	{
		const strom_preagg_target &t = sess->targets[sess->agg_resno[a]];
		any_numeric = any_numeric || (t.type_oid == STROM_NUMERICOID && t.kind != STROM_PREAGG_NROWS);
	}
	if (!any_numeric && ncols <= 64 && !getenv("STROM_GPUPREAGG_FETCH_ON_HOST"))
	{
		size_t	stride = KDS_TUPSLOT_STRIDE(ncols);
		size_t	need = STROMALIGN(KDS_HEAD_LENGTH(ncols) + stride * (size_t)ngroups);
		if (!dest)
			return (long)need;
		if (destlen < need)
			return -StromError_DataStoreNoSpace;
		fetch_init_head(sess, dest, need, ngroups);
		if (ngroups > 0)
		{
			int		errcode = 0;
			hipFunction_t fn = sess->prog->get_function(dev, "gpupreagg_hash_export_rows", &errcode);
			if (!fn)
				return -errcode;
			cl_uint	tmeta[64];
			for (size_t k = 0; k < nkeys; k++)
			{
				const strom_preagg_target &t = sess->targets[sess->key_resno[k]];
				tmeta[sess->key_resno[k]] = (cl_uint)type_length(t.type_oid) | 0x100u | ((cl_uint)k << 16) |
					(type_is_float(t.type_oid) ? 0x200u : 0u) | (t.type_oid == STROM_FLOAT4OID ? 0x400u : 0u);
			}
			for (size_t a = 0; a < naggs; a++)
			{
				const strom_preagg_target &t = sess->targets[sess->agg_resno[a]];
				bool	nrows = (t.kind == STROM_PREAGG_NROWS);
				tmeta[sess->agg_resno[a]] = (cl_uint)(nrows ? 8 : type_length(t.type_oid)) | ((cl_uint)a << 16) |
					(nrows ? 0x800u : 0u) |
					(!nrows && type_is_float(t.type_oid) ? 0x200u : 0u) |
					(!nrows && t.type_oid == STROM_FLOAT4OID ? 0x400u : 0u) |
					(!nrows && type_is_float(t.type_oid) && t.kind != STROM_PREAGG_PSUM ? 0x1000u : 0u);
			}
			size_t	rows_len = stride * (size_t)ngroups;
			char   *d_rows = (char *)dev->pool.alloc(rows_len + 16 + sizeof(tmeta));
			if (!d_rows)
				return -StromError_OutOfMemory;
			char   *d_counter = d_rows + rows_len;
			char   *d_meta = d_counter + 16;
			const void *a_tab = sess->htab;
			void	   *a_rows = d_rows, *a_cnt = d_counter;
			const void *a_meta = d_meta;
			cl_uint		a_stride = (cl_uint)stride, a_ncols = (cl_uint)ncols;
			void	   *args[] = { &a_tab, &a_rows, &a_stride, &a_ncols, &a_meta, &a_cnt };
			unsigned	grid = std::min<unsigned>((sess->hash_capacity + 255) / 256,
												  (unsigned)dev->prop.multiProcessorCount * 8);
			cl_uint		count = 0;
			bool ok = (hipMemsetAsync(d_counter, 0, 16, dev->streams[0]) == hipSuccess &&
					   hipMemcpyAsync(d_meta, tmeta, sizeof(cl_uint) * ncols, hipMemcpyHostToDevice, dev->streams[0]) == hipSuccess &&
					   hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, dev->streams[0], args, nullptr) == hipSuccess &&
					   hipStreamSynchronize(dev->streams[0]) == hipSuccess &&
					   hipMemcpy(&count, d_counter, sizeof(count), hipMemcpyDeviceToHost) == hipSuccess &&
					   count == ngroups &&
					   hipMemcpy((char *)dest + KDS_HEAD_LENGTH(ncols), d_rows, rows_len, hipMemcpyDeviceToHost) == hipSuccess);
			dev->pool.release(d_rows);
			if (!ok)
				return -StromError_HipInternal;
		}
		dest->nitems = ngroups;
		return (long)ngroups;
	}
	if (ngroups > 0)
	{
		int		errcode = 0;
		hipFunction_t fn = sess->prog->get_function(dev, "gpupreagg_hash_export", &errcode);
		if (!fn)
			return -errcode;
		char   *d_out = (char *)dev->pool.alloc(reclen * ngroups + 16);
		if (!d_out)
			return -StromError_OutOfMemory;
		char   *d_counter = d_out + reclen * ngroups;
		const void *a_tab = sess->htab;
		void	   *a_out = d_out, *a_cnt = d_counter;
		void	   *args[] = { &a_tab, &a_out, &a_cnt };
		unsigned	grid = std::min<unsigned>((sess->hash_capacity + 255) / 256,
											  (unsigned)dev->prop.multiProcessorCount * 8);
		cl_uint		count = 0;
		recs.resize(reclen * ngroups);
		bool ok = (hipMemsetAsync(d_counter, 0, 16, dev->streams[0]) == hipSuccess &&
				   hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, dev->streams[0], args, nullptr) == hipSuccess &&
				   hipStreamSynchronize(dev->streams[0]) == hipSuccess &&
				   hipMemcpy(&count, d_counter, sizeof(count), hipMemcpyDeviceToHost) == hipSuccess &&
				   count == ngroups &&
				   hipMemcpy(recs.data(), d_out, recs.size(), hipMemcpyDeviceToHost) == hipSuccess);
		dev->pool.release(d_out);
		if (!ok)
			return -StromError_HipInternal;
	}
	/* numeric sums too wide for the 64-bit form leave as two partial rows */
	const cl_long P17 = 100000000000000000L;
	struct spill { cl_uint rec; int resno; cl_ulong image; };
	std::vector<spill> spills;
	for (cl_uint r = 0; r < ngroups; r++)
	{
		const gpupreagg_export_rec *rec = (const gpupreagg_export_rec *)(recs.data() + reclen * r);
		cl_uint		flags = rec->flags;
		const cl_ulong *vals = rec->body + nkeys;
		for (size_t a = 0; a < naggs; a++)
		{
			const strom_preagg_target &t = sess->targets[sess->agg_resno[a]];
			cl_ulong	img;
			if (t.type_oid != STROM_NUMERICOID || t.kind == STROM_PREAGG_NROWS || !(flags & (2u << a)))
				continue;
			cl_long v = (cl_long)vals[a];
			if (!fixed_to_numeric(v, t.scale, &img))
			{
				if (!fixed_to_numeric((v / P17) * P17, t.scale, &img))
					return -StromError_DataStoreOutOfRange;
				spills.push_back(spill{r, sess->agg_resno[a], img});
			}
		}
	}
	size_t	nrows_out = (size_t)ngroups + spills.size();
	size_t	need = STROMALIGN(KDS_HEAD_LENGTH(ncols) + KDS_TUPSLOT_STRIDE(ncols) * nrows_out);
	if (!dest)
		return (long)need;
	if (destlen < need)
		return -StromError_DataStoreNoSpace;
	fetch_init_head(sess, dest, need, nrows_out);
	auto put_keys = [&](const gpupreagg_export_rec *rec, Datum *values, cl_char *isnull)
	{
		cl_uint		knull = rec->knull;
		const cl_ulong *kimg = rec->body;
		for (size_t k = 0; k < nkeys; k++)
		{
			int		resno = sess->key_resno[k];
			const strom_preagg_target &t = sess->targets[resno];
			if (knull & (1u << k))
			{
				isnull[resno] = 1;
				continue;
			}
			isnull[resno] = 0;
			cl_ulong raw = kimg[k];
			if (type_is_float(t.type_oid))
				raw = float_image_to_datum(t, raw, false);
			values[resno] = 0;
			memcpy(&values[resno], &raw, type_length(t.type_oid));
		}
	};
	cl_uint	row = 0;
	for (cl_uint r = 0; r < ngroups; r++, row++)
	{
		const gpupreagg_export_rec *rec = (const gpupreagg_export_rec *)(recs.data() + reclen * r);
		cl_uint		flags = rec->flags;
		const cl_ulong *vals = rec->body + nkeys;
		Datum	   *values = KERN_DATA_STORE_VALUES(dest, row);
		cl_char	   *isnull = KERN_DATA_STORE_ISNULL(dest, row);
		memset(values, 0, KDS_TUPSLOT_STRIDE(ncols));
		put_keys(rec, values, isnull);
		for (size_t a = 0; a < naggs; a++)
		{
			int		resno = sess->agg_resno[a];
			const strom_preagg_target &t = sess->targets[resno];
			cl_ulong raw = vals[a];
			if (t.kind == STROM_PREAGG_NROWS)
				values[resno] = raw;
			else if (!(flags & (2u << a)))
				isnull[resno] = 1;
			else if (t.type_oid == STROM_NUMERICOID)
			{
				cl_long v = (cl_long)raw;
				if (!fixed_to_numeric(v, t.scale, &raw))
					(void)fixed_to_numeric(v - (v / P17) * P17, t.scale, &raw);	/* high part: spill row */
				values[resno] = raw;
			}
			else if (type_is_float(t.type_oid))
				values[resno] = float_image_to_datum(t, raw, t.kind != STROM_PREAGG_PSUM);
			else
				memcpy(&values[resno], &raw, type_length(t.type_oid));
		}
	}
	for (const spill &sp : spills)
	{
		Datum	   *values = KERN_DATA_STORE_VALUES(dest, row);
		cl_char	   *isnull = KERN_DATA_STORE_ISNULL(dest, row);
		memset(values, 0, KDS_TUPSLOT_STRIDE(ncols));
		for (int i = 0; i < ncols; i++)
			isnull[i] = (sess->targets[i].kind != STROM_PREAGG_NROWS);	/* nrows = 0 */
		put_keys((const gpupreagg_export_rec *)(recs.data() + reclen * sp.rec), values, isnull);
		isnull[sp.resno] = 0;
		values[sp.resno] = sp.image;
		row++;
	}
	dest->nitems = row;
	return (long)row;
}

}	/* namespace */

/*
 * dense sessions: the partial rows formatted on the device (preagg_dense_export_rows) and copied
 * into the caller's buffer once.  *p_fallback: not this way (compacted slots, numeric partials --
 * their sums may leave as several rows --, an integer sum beyond int8): the host loop below.
 */
static long
gpupreagg_fetch_dense_device(strom_gpupreagg *sess, kern_data_store *dest, size_t destlen, bool *p_fallback)
{
	Device	   *dev = sess->dev;
	int			ncols = (int)sess->targets.size();
	cl_uint		N = sess->ctl.ngroups;

	*p_fallback = true;
	if (!sess->present.empty() || ncols > PREAGG_EXPORT_MAXCOLS || sess->key_resno.size() > GPUPREAGG_MAXKEYS || getenv("STROM_GPUPREAGG_FETCH_ON_HOST"))
		return 0;
	for (const strom_preagg_target &t : sess->targets)
		if (t.type_oid == STROM_NUMERICOID && t.kind != STROM_PREAGG_NROWS)
			return 0;
	int			errcode = 0;
	hipFunction_t fn = fixed_function(dev, "preagg_dense_export_rows", &errcode);
	if (!fn)
		return 0;
	size_t		stride = KDS_TUPSLOT_STRIDE(ncols);
	size_t		head_len = KDS_HEAD_LENGTH(ncols);
	std::lock_guard<std::mutex> g(sess->lock);
	(void)hipSetDevice(dev->hip_id);
	if (!sess->d_export_spec)
	{
		preagg_export_spec	spec;
		memset(&spec, 0, sizeof(spec));
		spec.ngroups = N;
		spec.ncols = (cl_uint)ncols;
		spec.stride = (cl_uint)stride;
		spec.nkeys = (cl_uint)sess->key_resno.size();
		for (size_t k = 0; k < sess->key_resno.size(); k++)
		{
			spec.key_min[k] = sess->ctl.key_min[k];
			spec.key_range[k] = sess->ctl.key_range[k];
			spec.key_stride[k] = std::max<cl_uint>(1, sess->ctl.key_stride[k]);
			auto &c = spec.col[sess->key_resno[k]];
			c.kind = 0;
			c.len = (cl_uint)type_length(sess->targets[sess->key_resno[k]].type_oid);
			c.which = (cl_uint)k;
		}
		for (size_t a = 0; a < sess->agg_resno.size(); a++)
		{
			const strom_preagg_target &t = sess->targets[sess->agg_resno[a]];
			auto &c = spec.col[sess->agg_resno[a]];
			bool	isfloat = type_is_float(t.type_oid);
			c.which = 1 + (cl_uint)a;
			c.vals_off = gpupreagg_table_offset(1 + (int)a, N);
			c.len = (cl_uint)(t.kind == STROM_PREAGG_NROWS ? 8 : type_length(t.type_oid));
			c.float4 = (t.type_oid == STROM_FLOAT4OID);
			if (t.kind == STROM_PREAGG_NROWS)
				c.kind = 1;
			else if (sess->is_intsum((int)a))
			{
				c.kind = 5;
				c.hi_off = sess->table_hi_offset((int)a, N);
			}
			else if (isfloat)
				c.kind = (t.kind == STROM_PREAGG_PSUM ? 3 : 4);
			else
				c.kind = 2;
		}
		sess->d_export_spec = (char *)dev->pool.alloc(sizeof(spec));
		if (!sess->d_export_spec ||
			hipMemcpy(sess->d_export_spec, &spec, sizeof(spec), hipMemcpyHostToDevice) != hipSuccess)
			return -StromError_OutOfMemory;
	}
	if (session_quiesce(sess) != hipSuccess)
		return -StromError_HipInternal;
	size_t		max_rows = (dest && destlen > head_len ? std::min<size_t>(N, (destlen - head_len) / stride) : 0);
	char	   *d_rows = (char *)dev->pool.alloc(stride * max_rows + 16);
	if (!d_rows)
		return -StromError_OutOfMemory;
	char	   *d_counter = d_rows + stride * max_rows;
	hipStream_t	stream = dev->streams[0];
	const void *a_table = sess->table;
	const void *a_spec = sess->d_export_spec;
	void	   *a_rows = d_rows, *a_cnt = d_counter;
	cl_uint		a_max = (cl_uint)max_rows;
	void	   *args[] = { &a_table, &a_spec, &a_rows, &a_max, &a_cnt };
	unsigned	grid = std::max(1u, std::min<unsigned>((N + 255) / 256, (unsigned)dev->prop.multiProcessorCount * 8));
	cl_uint		counter[2] = { 0, 0 };
	bool ok = (hipMemsetAsync(d_counter, 0, 16, stream) == hipSuccess &&
			   hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, stream, args, nullptr) == hipSuccess &&
			   hipMemcpyAsync(counter, d_counter, sizeof(counter), hipMemcpyDeviceToHost, stream) == hipSuccess &&
			   hipStreamSynchronize(stream) == hipSuccess);
	long		result;
	size_t		need = STROMALIGN(head_len + stride * (size_t)counter[0]);
	if (!ok)
		result = -StromError_HipInternal;
	else if (counter[1] != 0)
		result = 0;								/* a sum beyond int8: several rows, made on the host */
	else
	{
		*p_fallback = false;
		if (!dest)
			result = (long)need;
		else if (destlen < need)
			result = -StromError_DataStoreNoSpace;
		else
		{
			fetch_init_head(sess, dest, need, counter[0]);
			if (counter[0] > 0 &&
				hipMemcpy((char *)dest + head_len, d_rows, stride * (size_t)counter[0], hipMemcpyDeviceToHost) != hipSuccess)
				result = -StromError_HipInternal;
			else
			{
				dest->nitems = counter[0];
				result = (long)counter[0];
			}
		}
	}
	if (result < 0)
		*p_fallback = false;
	dev->pool.release(d_rows);
	return result;
}

/*
 * partial rows out: TUPSLOT, one row per group seen so far (plus, for a
 * numeric sum too wide for the 64-bit numeric form, one extra partial row
 * of the same group carrying the high part: partial rows add up, so the
 * final aggregate is unchanged)
 */
extern "C" long
strom_gpupreagg_fetch(strom_gpupreagg *sess, kern_data_store *dest, size_t destlen)
{
	if (sess && sess->hashed)
		return gpupreagg_fetch_hashed(sess, dest, destlen);
	if (!sess || !sess->has_domain)
		return -StromError_BadRequestMessage;
	{
		bool	fallback = false;
		long	r = gpupreagg_fetch_dense_device(sess, dest, destlen, &fallback);
		if (!fallback)
			return r;
	}
	Device *dev = sess->dev;
	int		ncols = (int)sess->targets.size();
	cl_uint	N = sess->ctl.ngroups;
	std::vector<char> host(sess->table_bytes);

	(void)hipSetDevice(dev->hip_id);
	if (session_quiesce(sess) != hipSuccess ||
		hipMemcpy(host.data(), sess->table, sess->table_bytes, hipMemcpyDeviceToHost) != hipSuccess)
		return -StromError_HipInternal;
	const cl_uint *gflags = (const cl_uint *)host.data();
	size_t	ngroups = 0;
	std::vector<numeric_spill> spills;
	std::vector<cl_ulong> pieces;
	for (cl_uint g = 0; g < N; g++)
	{
		if (!(gflags[g] & 1))
			continue;
		ngroups++;
		for (size_t a = 0; a < sess->agg_resno.size(); a++)
		{
			/* an integer sum (128 bits in the table) that does not fit its datum leaves as
			 * several partial rows: see sum_pieces */
			const strom_preagg_target &t = sess->targets[sess->agg_resno[a]];
			if (!sess->is_intsum((int)a) || !(gflags[g] & (2u << a)))
				continue;
			cl_ulong lo = ((const cl_ulong *)(host.data() + gpupreagg_table_offset(1 + (int)a, N)))[g];
			cl_long	 hi = ((const cl_long *)(host.data() + sess->table_hi_offset((int)a, N)))[g];
			int		rc = sum_pieces(t, lo, hi, pieces);
			if (rc != 0)
				return -rc;
			for (size_t k = 1; k < pieces.size(); k++)
				spills.push_back(numeric_spill{g, sess->agg_resno[a], pieces[k]});
		}
	}
	ngroups += spills.size();
	size_t	need = STROMALIGN(KDS_HEAD_LENGTH(ncols) + KDS_TUPSLOT_STRIDE(ncols) * ngroups);
	if (!dest)
		return (long)need;
	if (destlen < need)
		return -StromError_DataStoreNoSpace;
	memset(dest, 0, KDS_HEAD_LENGTH(ncols));
	dest->hostptr = (hostptr_t)(uintptr_t)&dest->hostptr;
	dest->length = (cl_uint)need;
	dest->ncols = ncols;
	dest->nrooms = (cl_uint)ngroups;
	dest->format = KDS_FORMAT_TUPSLOT;
	dest->tdtypeid = 2249;
	dest->tdtypmod = -1;
	for (int i = 0; i < ncols; i++)
	{
		const strom_preagg_target &t = sess->targets[i];
		int len = (t.kind == STROM_PREAGG_NROWS ? 8 : type_length(t.type_oid));
		dest->colmeta[i].attbyval = 1;
		dest->colmeta[i].attalign = (cl_char)len;
		dest->colmeta[i].attlen = (cl_short)len;
		dest->colmeta[i].attnum = (cl_short)(i + 1);
		dest->colmeta[i].attcacheoff = -1;
	}
	cl_uint	row = 0;
	for (cl_uint g = 0; g < N; g++)
	{
		if (!(gflags[g] & 1))
			continue;
		Datum	   *values = KERN_DATA_STORE_VALUES(dest, row);
		cl_char	   *isnull = KERN_DATA_STORE_ISNULL(dest, row);
		memset(values, 0, KDS_TUPSLOT_STRIDE(ncols));
		for (size_t k = 0; k < sess->key_resno.size(); k++)
		{
			int		resno = sess->key_resno[k];
			cl_uint	dense = (sess->present.empty() ? g : sess->present[g]);
			cl_uint	off = (dense / sess->ctl.key_stride[k]) % (sess->ctl.key_range[k] + 1);
			if (off == sess->ctl.key_range[k])
				isnull[resno] = 1;
			else
			{
				cl_long v = sess->ctl.key_min[k] + off;
				memcpy(&values[resno], &v, type_length(sess->targets[resno].type_oid));
			}
		}
		for (size_t a = 0; a < sess->agg_resno.size(); a++)
		{
			int		resno = sess->agg_resno[a];
			const strom_preagg_target &t = sess->targets[resno];
			const cl_ulong *vals = (const cl_ulong *)(host.data() + gpupreagg_table_offset(1 + (int)a, N));
			if (t.kind == STROM_PREAGG_NROWS)
				values[resno] = vals[g];
			else if (!(gflags[g] & (2u << a)))
				isnull[resno] = 1;
			else
			{
				cl_ulong raw = vals[g];
				if (t.type_oid == STROM_NUMERICOID && t.scale < 0)
					values[resno] = raw;			/* accumulated in the 64-bit form itself */
				else if (sess->is_intsum((int)a))
				{
					/* the first piece; the others went to spill rows above */
					cl_long	 hi = ((const cl_long *)(host.data() + sess->table_hi_offset((int)a, N)))[g];
					(void)sum_pieces(t, raw, hi, pieces);
					values[resno] = pieces[0];
				}
				else if (t.type_oid == STROM_NUMERICOID)
				{
					/* pmin / pmax of a fixed-point numeric: one int8 value */
					if (!fixed_to_numeric((cl_long)raw, t.scale, &raw))
						return -StromError_DataStoreOutOfRange;
					values[resno] = raw;
				}
				else if (type_is_float(t.type_oid))
				{
					if (t.kind != STROM_PREAGG_PSUM)
					{
						/* order-preserving key -> IEEE bits */
						raw = (raw & 0x8000000000000000UL) ? (raw & 0x7fffffffffffffffUL) : ~raw;
					}
					if (t.type_oid == STROM_FLOAT4OID)
					{
						double d; float f;
						memcpy(&d, &raw, 8);
						f = (float)d;
						raw = 0;
						memcpy(&raw, &f, 4);
					}
					values[resno] = raw;
				}
				else
					memcpy(&values[resno], &raw, type_length(t.type_oid));
			}
		}
		row++;
	}
	for (const numeric_spill &sp : spills)
	{
		Datum	   *values = KERN_DATA_STORE_VALUES(dest, row);
		cl_char	   *isnull = KERN_DATA_STORE_ISNULL(dest, row);
		memset(values, 0, KDS_TUPSLOT_STRIDE(ncols));
		for (int i = 0; i < ncols; i++)
			isnull[i] = (sess->targets[i].kind != STROM_PREAGG_NROWS);	/* nrows = 0 */
		for (size_t k = 0; k < sess->key_resno.size(); k++)
		{
			int		resno = sess->key_resno[k];
			cl_uint	dense = (sess->present.empty() ? sp.gid : sess->present[sp.gid]);
			cl_uint	off = (dense / sess->ctl.key_stride[k]) % (sess->ctl.key_range[k] + 1);
			if (off != sess->ctl.key_range[k])
			{
				cl_long v = sess->ctl.key_min[k] + off;
				isnull[resno] = 0;
				memcpy(&values[resno], &v, type_length(sess->targets[resno].type_oid));
			}
		}
		isnull[sp.resno] = 0;
		values[sp.resno] = sp.image;
		row++;
	}
	dest->nitems = row;
	return (long)row;
}

/* ================================================================== *
 * The reference's per-chunk message: pgstrom_gpupreagg {msg, dprog_key,
 * needs_grouping, num_groups, pds, pds_dest, kern_gpupreagg}
 * (opencl_gpupreagg.h:994-1003), served by clserv_process_gpupreagg
 * (gpupreagg.c:3849-4240).  One chunk in, the chunk's partial rows out in
 * kds_dest -- nothing is kept between requests.  Built from the session
 * machinery above: key range of the chunk -> dense table geometry (or the
 * hashed GROUP BY when the keys do not map to dense ids) -> fold -> fetch.
 * The steps have host decisions in between, so the request runs on the
 * device's worker thread; the submitter only queues.
 * ================================================================== */
namespace {

int
chunk_domain(strom_devprog_key key, Program *prog, Device *dev,
			 const strom_preagg_target *targets, int ntargets,
			 const kern_parambuf *kparams, strom_dstore *kds_dev,
			 const kern_row_map *krowmap, strom_preagg_domain *dom)
{
	int		nkeys = 0;
	memset(dom, 0, sizeof(*dom));
	for (int i = 0; i < ntargets; i++)
	{
		if (targets[i].kind != STROM_PREAGG_KEY)
			continue;
		if (type_is_float(targets[i].type_oid) || targets[i].type_oid == STROM_NUMERICOID)
			return StromError_DataStoreOutOfRange;		/* no dense ids for these */
		nkeys++;
	}
	if (nkeys > STROM_PREAGG_MAXKEYS)
		return StromError_DataStoreOutOfRange;
	dom->nkeys = nkeys;
	if (nkeys == 0)
		return 0;
	if (!program_accepts_format(prog, kds_dev->head.format))
		return StromError_BadRequestMessage;
	/*
	 * a COLUMN chunk whose group keys are plain columns: the zone maps bound the keys (of all
	 * rows -- a superset of the rows the qual keeps, which is all a dense domain needs): no pass
	 * over the chunk, no round trip (the key-range kernel and its wait were 165 us of a 325k-row
	 * message, profiles/r02_chunk_message_probe.txt).  No row map: its rows may be few.
	 */
	if (kds_dev->head.format == KDS_FORMAT_COLUMN && !krowmap && !getenv("STROM_GPUPREAGG_NO_ZONE_DOMAIN"))
	{
		const char *lst = strstr(prog->source.c_str(), "#define GPUPREAGG_KEYCOLS_LIST(X)");
		chunk_coldir dir;
		chunk_coldir_of(nullptr, kds_dev, nullptr, &dir);
		bool		ok = (lst != nullptr && dir.cd != nullptr);
		const char *eol = (lst ? strchr(lst, '\n') : nullptr);
		int			found = 0;
		for (const char *p = (ok ? strstr(lst, " X(") : nullptr); ok && p && (!eol || p < eol); p = strstr(p + 1, " X("))
		{
			int		kidx = -1, attno = 0;
			if (sscanf(p, " X(%d,%d)", &kidx, &attno) != 2 || kidx != found || kidx >= nkeys ||
				attno < 1 || attno > (int)dir.ncols)
			{
				ok = false;
				break;
			}
			const kern_coldir &c = dir.cd[attno - 1];
			if (c.stat_flags & KDS_COLSTAT_ISFLOAT)
				ok = false;
			else if (!(c.stat_flags & KDS_COLSTAT_MINMAX))
			{
				dom->key_min[kidx] = 0;			/* NULL keys only: the NULL slot alone */
				dom->key_range[kidx] = 0;
			}
			else
			{
				cl_ulong span = (cl_ulong)c.maxval - (cl_ulong)c.minval;
				if (c.maxval < c.minval || span >= 0xfffffffeUL)
					ok = false;
				dom->key_min[kidx] = c.minval;
				dom->key_range[kidx] = (cl_uint)span + 1;
			}
			found++;
		}
		if (ok && found == nkeys)
			return 0;
		memset(dom, 0, sizeof(*dom));
		dom->nkeys = nkeys;
	}
	if (strom_lookup_device_program(key, 1) != STROM_DEVPROG_READY)
		return StromError_ProgramBuildFailure;
	(void)hipSetDevice(dev->hip_id);
	hipStream_t stream = dev->pick_stream();
	int		errcode = 0;
	hipFunction_t fn = prog->get_function(dev, "gpupreagg_keyrange", &errcode);
	if (!fn)
		return errcode;
	gpupreagg_keyrange_t img;
	memset(&img, 0, sizeof(img));
	for (int k = 0; k < STROM_PREAGG_MAXKEYS; k++)
	{
		img.kmin[k] = INT64_MAX;
		img.kmax[k] = INT64_MIN;
	}
	size_t	kg_len = STROMALIGN(offsetof(kern_gpupreagg, kparams) + kparams->length);
	std::vector<char> kg(kg_len, 0);
	memcpy(kg.data() + offsetof(kern_gpupreagg, kparams), kparams, kparams->length);
	char   *d_kg = (char *)dev->pool.alloc(kg_len);
	char   *d_out = (char *)dev->pool.alloc(sizeof(img));
	void   *d_map = nullptr;
	int		rc = 0;
	do {
		if (!d_kg || !d_out)
		{
			rc = StromError_OutOfMemory;
			break;
		}
		if (hipMemcpyAsync(d_kg, kg.data(), kg_len, hipMemcpyHostToDevice, stream) != hipSuccess ||
			hipMemcpyAsync(d_out, &img, sizeof(img), hipMemcpyHostToDevice, stream) != hipSuccess)
		{
			rc = StromError_HipInternal;
			break;
		}
		cl_uint	nrows = kds_dev->head.nitems;
		const void *a_map = nullptr;
		if (krowmap && krowmap->nvalids >= 0)
		{
			size_t	len = offsetof(kern_row_map, rindex) + sizeof(cl_int) * (size_t)krowmap->nvalids;
			d_map = dev->pool.alloc(len);
			if (!d_map || hipMemcpyAsync(d_map, krowmap, len, hipMemcpyHostToDevice, stream) != hipSuccess)
			{
				rc = StromError_OutOfMemory;
				break;
			}
			a_map = d_map;
			nrows = (cl_uint)krowmap->nvalids;
		}
		const void *a_kg = d_kg;
		const void *a_kds = kds_dev->devptr;
		const void *a_toast = nullptr;
		void	   *a_out = d_out;
		void	   *args[] = { &a_kg, &a_kds, &a_toast, &a_map, &a_out };
		unsigned	grid = (unsigned)std::min<size_t>(((size_t)nrows + 255) / 256,
													  (size_t)dev->prop.multiProcessorCount * 8);
		if (grid > 0 &&
			hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, stream, args, nullptr) != hipSuccess)
		{
			rc = StromError_HipInternal;
			break;
		}
		if (hipMemcpyAsync(&img, d_out, sizeof(img), hipMemcpyDeviceToHost, stream) != hipSuccess)
			rc = StromError_HipInternal;
	} while (0);
	if (hipStreamSynchronize(stream) != hipSuccess && rc == 0)
		rc = StromError_HipInternal;
	if (d_kg) dev->pool.release(d_kg);
	if (d_out) dev->pool.release(d_out);
	if (d_map) dev->pool.release(d_map);
	if (rc != 0)
		return rc;
	for (int k = 0; k < nkeys; k++)
	{
		if (img.nvalues[k] == 0)
		{
			dom->key_min[k] = 0;		/* NULL keys only (or no row at all): the NULL slot alone */
			dom->key_range[k] = 0;
			continue;
		}
		/* (unsigned arithmetic: max - min of two int64 may not fit int64) */
		cl_ulong span = (cl_ulong)img.kmax[k] - (cl_ulong)img.kmin[k];
		if (span >= 0xfffffffeUL)
			return StromError_DataStoreOutOfRange;
		dom->key_min[k] = img.kmin[k];
		dom->key_range[k] = (cl_uint)span + 1;
	}
	return 0;
}

}	/* namespace */

/* the key domain the last per-chunk message of a program measured, widened by every later one
 * (strom_submit_gpupreagg_chunk: heap-page chunks have no zone maps) */
static std::mutex domain_hint_lock;
static std::map<strom_devprog_key, strom_preagg_domain> domain_hints;

static bool
domain_hint_get(strom_devprog_key key, strom_preagg_domain *dom)
{
	std::lock_guard<std::mutex> g(domain_hint_lock);
	auto it = domain_hints.find(key);
	if (it == domain_hints.end())
		return false;
	*dom = it->second;
	return true;
}

static void
domain_hint_put(strom_devprog_key key, const strom_preagg_domain &dom)
{
	std::lock_guard<std::mutex> g(domain_hint_lock);
	auto it = domain_hints.find(key);
	if (it == domain_hints.end() || it->second.nkeys != dom.nkeys)
	{
		if (domain_hints.size() > 4096)
			domain_hints.clear();					/* (a hint: forgetting costs one key-range pass) */
		domain_hints[key] = dom;
		return;
	}
	strom_preagg_domain &old = it->second;
	for (int k = 0; k < dom.nkeys && k < STROM_PREAGG_MAXKEYS; k++)
	{
		if (dom.key_range[k] == 0)
			continue;								/* NULL keys only: nothing to widen by */
		if (old.key_range[k] == 0)
		{
			old.key_min[k] = dom.key_min[k];
			old.key_range[k] = dom.key_range[k];
			continue;
		}
		__int128	lo = std::min<__int128>(old.key_min[k], dom.key_min[k]);
		__int128	hi = std::max<__int128>((__int128)old.key_min[k] + old.key_range[k], (__int128)dom.key_min[k] + dom.key_range[k]);
		if (hi - lo >= 0xfffffffeLL)
		{
			old = dom;								/* too wide to be a dense domain: start over */
			return;
		}
		old.key_min[k] = (int64_t)lo;
		old.key_range[k] = (uint32_t)(hi - lo);
	}
}

extern "C" int
strom_gpupreagg_chunk_domain(strom_devprog_key key,
							 const strom_preagg_target *targets, int ntargets,
							 const kern_parambuf *kparams,
							 const kern_data_store *kds, strom_dstore *kds_dev,
							 const kern_row_map *krowmap,
							 int dindex, strom_preagg_domain *domain_out)
{
	STROM_ABI_TRY
	Program *prog = lookup_program(key);
	Device *dev = get_device(dindex);
	if (!prog || !dev || !targets || ntargets < 1 || !kparams || !domain_out || (!kds) == (!kds_dev) ||
		(kds_dev && kds_dev->dindex != dindex))
		return (!dev ? StromError_ServerNotReady : StromError_BadRequestMessage);
	strom_dstore *tmp = nullptr;
	if (!kds_dev)
	{
		tmp = strom_dstore_upload(kds, dindex);
		if (!tmp)
			return StromError_OutOfMemory;
		kds_dev = tmp;
	}
	int rc = chunk_domain(key, prog, dev, targets, ntargets, kparams, kds_dev, krowmap, domain_out);
	if (tmp)
		strom_dstore_release(tmp);
	return rc;
	STROM_ABI_CATCH(StromError_OutOfMemory, (int *)nullptr)
}

extern "C" strom_task *
strom_submit_gpupreagg_chunk(strom_devprog_key key,
							 const strom_preagg_target *targets, int ntargets,
							 kern_gpupreagg *kgpreagg,
							 const kern_data_store *kds, strom_dstore *kds_dev,
							 kern_data_store *kds_dest, size_t dest_length,
							 int needs_grouping, double num_groups,
							 int dindex,
							 strom_done_cb done, void *arg, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	*p_errcode = 0;
	Program *prog = lookup_program(key);
	Device *dev = get_device(dindex);
	if (!prog || !dev || !targets || ntargets < 1 || !kgpreagg || !kds_dest ||
		(!kds) == (!kds_dev) || (kds_dev && kds_dev->dindex != dindex) ||
		kgpreagg->kparams.length < offsetof(kern_parambuf, poffset) ||
		dest_length < (size_t)KDS_HEAD_LENGTH(ntargets))
	{
		*p_errcode = (!dev ? StromError_ServerNotReady : StromError_BadRequestMessage);
		return nullptr;
	}
	int		nkeys = 0;
	for (int i = 0; i < ntargets; i++)
		nkeys += (targets[i].kind == STROM_PREAGG_KEY);
	if ((needs_grouping != 0) != (nkeys > 0))
	{
		/* the message says GROUP BY, the program has no key (or the reverse) */
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	std::vector<strom_preagg_target> tg(targets, targets + ntargets);
	strom_task_impl *task = task_create(dev, done, arg);
	device_run_async(dev, [=]() {
		const kern_parambuf *kparams = KERN_GPUPREAGG_PARAMBUF(kgpreagg);
		const kern_row_map *krowmap = KERN_GPUPREAGG_KROWMAP(kgpreagg);
		strom_dstore	   *tmp = nullptr, *src = kds_dev;
		strom_gpupreagg	   *sess = nullptr;
		strom_perfmon		pfm;
		int					rc = 0;
		memset(&pfm, 0, sizeof(pfm));
		if (krowmap->nvalids < 0)
			krowmap = nullptr;
		do {
			if (strom_lookup_device_program(key, 1) != STROM_DEVPROG_READY)
			{
				rc = StromError_ProgramBuildFailure;
				break;
			}
			if (!src)
			{
				src = tmp = strom_dstore_upload(kds, dindex);
				if (!tmp)
				{
					rc = StromError_OutOfMemory;
					break;
				}
			}
			strom_preagg_domain dom;
			/*
			 * The key domain.  A COLUMN chunk's zone maps give it for nothing (chunk_domain); heap
			 * pages have none, and the key-range pass over them -- a kernel and a wait -- is a third
			 * of such a message.  The chunks of one scan look alike, so the domain the PREVIOUS
			 * message of this program measured is tried first: a key outside it makes the fold answer
			 * DataStoreOutOfRange, the range is measured after all (and remembered, widened) and the
			 * chunk folded again.  A hint, not state: the answer never depends on it.
			 */
			bool		from_hint = false;
			if (src->head.format != KDS_FORMAT_COLUMN && !getenv("STROM_GPUPREAGG_NO_DOMAIN_HINT"))
				from_hint = domain_hint_get(key, &dom);
			if (from_hint)
				rc = 0;
			else
			{
				rc = chunk_domain(key, prog, dev, tg.data(), ntargets, kparams, src, krowmap, &dom);
				if (rc == 0 && src->head.format != KDS_FORMAT_COLUMN)
					domain_hint_put(key, dom);
			}
		fold_again:
			uint32_t hint = (num_groups > 0 && num_groups < 4e9 ? (uint32_t)num_groups : 0);
			if (rc == 0)
			{
				/*
				 * dense ids past ~1.6e5: the dense kernels split them over id-range roles that
				 * each read every row (1e5 ids: 1.4 ms per 1e8 rows, 64 roles at most), the
				 * hashed GROUP BY's partition plan takes 2.3 ms whatever the count
				 * (profiles/r02_dense_vs_hashed.txt)
				 */
				double	ids = 1.0;
				int		nk = 0;
				for (int i = 0; i < ntargets; i++)
				{
					if (tg[i].kind == STROM_PREAGG_KEY && nk < STROM_PREAGG_MAXKEYS)
						ids *= (double)dom.key_range[nk++];
				}
				if (ids > 160000.0 && !getenv("STROM_GPUPREAGG_CHUNK_DENSE_ONLY"))
				{
					double	bound = std::min(ids, std::max(1.0, (double)src->head.nitems / 8));
					int		rc2 = 0;
					sess = strom_gpupreagg_create_hashed(key, tg.data(), ntargets, kparams,
														 hint ? hint : (uint32_t)std::min(bound, 4.0e6), dindex, &rc2);
					/* (what the hashed kernels do not take -- 64-bit numeric partials -- stays dense) */
				}
			}
			if (rc == 0 && !sess)
				sess = strom_gpupreagg_create(key, tg.data(), ntargets, kparams, &dom, dindex, &rc);
			if (!sess && rc == StromError_DataStoreOutOfRange)
			{
				/* keys without dense ids (float / numeric / sparse): hashed GROUP BY */
				rc = 0;
				sess = strom_gpupreagg_create_hashed(key, tg.data(), ntargets, kparams, hint, dindex, &rc);
			}
			if (!sess)
			{
				if (rc == 0)
					rc = StromError_HipInternal;
				break;
			}
			strom_task *fold = strom_submit_gpupreagg(sess, nullptr, src, krowmap, nullptr, nullptr, &rc);
			if (!fold)
				break;
			rc = strom_task_wait(fold, &pfm);
			if (rc == StromError_DataStoreOutOfRange && from_hint)
			{
				/* a key outside the remembered domain: measure this chunk's, once */
				from_hint = false;
				strom_gpupreagg_release(sess);
				sess = nullptr;
				rc = chunk_domain(key, prog, dev, tg.data(), ntargets, kparams, src, krowmap, &dom);
				if (rc != 0)
					break;
				domain_hint_put(key, dom);
				goto fold_again;
			}
			if (rc != 0)
				break;					/* CpuReCheck: the chunk goes back whole (gpupreagg.c:2746-2750) */
			/* (one call: a kds_dest that is too small answers DataStoreNoSpace by itself) */
			long	n = strom_gpupreagg_fetch(sess, kds_dest, dest_length);
			if (n < 0)
				rc = (int)-n;
		} while (0);
		if (sess)
			strom_gpupreagg_release(sess);
		if (tmp)
			strom_dstore_release(tmp);
		kgpreagg->status = rc;			/* KERN_GPUPREAGG_DMARECV: the status word */
		task->pfm = pfm;
		task->pfm.enabled = perfmon_enabled();
		/* nothing of its own on a stream (every step above was waited for): it completes on
		 * the completer thread with this status, without the drain of all streams a request
		 * that failed in mid-launch needs (task_fail) */
		task->errcode = rc;
		task_enqueue(task);
	});
	return task;
	STROM_ABI_CATCH(nullptr, p_errcode)
}
