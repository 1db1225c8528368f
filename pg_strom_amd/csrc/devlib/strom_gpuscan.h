/*
 * strom_gpuscan.h -- GpuScan kernels (HIP, gfx950)
 *
 * Role in the reference: opencl_gpuscan.h:98-177 (gpuscan_qual +
 * gpuscan_writeback_row_error).  Per row i of the chunk:
 *     errcode = Success; rc = gpuscan_qual_eval(&errcode, ...);
 *     STROM_SET_ERROR(&errcode, rc is TRUE ? Success : RowFiltered);
 *     Success    -> results[] gets  +(i+1)
 *     CpuReCheck -> results[] gets  -(i+1)   (host re-evaluates the row)
 *     significant-> chunk errcode, first one wins
 * and kresults->nitems counts the entries written.  The reference leaves
 * the order of results[] undefined across work-groups; so does this.
 *
 * What is different is how a chunk is walked.  The generated code supplies
 *     STROM_KVAR_LIST(X)    X(attno, colidx, NAME)  one per referenced Var
 *     STROM_KPARAM_LIST(X)  X(index, NAME)          one per Const/Param
 *     gpuscan_qual_eval(errcode, KP, KV)
 * and this file supplies two kernels around it:
 *
 *   gpuscan_qual_column  KDS_FORMAT_COLUMN, no row map.  Persistent blocks
 *       walk tiles of BLOCK*4*QUADS rows; each thread fetches its quads with
 *       16-byte vector loads straight from the column arrays (no LDS on the
 *       read side: every byte is used exactly once), evaluates 4*QUADS rows
 *       in registers, and the survivors are compacted in row order with
 *       ballot+mbcnt (no LDS scan) into an LDS stage of STAGE entries.  The
 *       stage is flushed with one global atomic per flush -- a few thousand
 *       per 1e8-row chunk instead of one per work-group per 256 rows --
 *       and the flush itself is a contiguous coalesced store.
 *
 *   gpuscan_qual_column_resident  the same walk over a resident chunk: the
 *       request is the kernel argument, the cursor and the error word live
 *       in a ring slot, and the kernel publishes its result head itself
 *       (strom_kds.h: kern_gpuscan_column_args).
 *
 *   gpuscan_qual_generic  any format, optional kern_row_map.  Same
 *       compaction, rows fetched one datum at a time through kern_get_datum
 *       (this is the heap-tuple walk the reference does for every row).
 */
#ifndef STROM_GPUSCAN_DEVICE_H
#define STROM_GPUSCAN_DEVICE_H

#ifndef GPUSCAN_BLOCK
#define GPUSCAN_BLOCK		256
#endif
#ifndef GPUSCAN_QUADS
#define GPUSCAN_QUADS		1			/* 4 rows per thread and tile (swept: profiles/r01_gpuscan_tune.txt) */
#endif
#ifndef GPUSCAN_STAGE
#define GPUSCAN_STAGE		8192		/* LDS entries (32 KB) */
#endif
#define GPUSCAN_NWAVES		(GPUSCAN_BLOCK / STROM_WAVE)
#define GPUSCAN_TILE_ROWS	(GPUSCAN_BLOCK * 4 * GPUSCAN_QUADS)

/* ---- what the generated code declares -------------------------------- */
struct strom_kparams {
#define X(idx,NAME)	pg_##NAME##_t KPARAM_##idx;
	STROM_KPARAM_LIST(X)
#undef X
	int __dummy;
};
struct strom_kvars {
#define X(attno,colidx,NAME)	pg_##NAME##_t KVAR_##attno;
	STROM_KVAR_LIST(X)
#undef X
	int __dummy;
};
/* text / character(n) variables of a row taken from COLUMN arrays: offset -> address (strom_common.h) */
#ifndef STROM_KVARLENA_LIST
#define STROM_KVARLENA_LIST(X)
#endif
STROM_DEFINE_KVARS_FROM_COLUMN
#define STROM_KVARS_FINISH(KV)	((KV).__dummy = 0)
#include "strom_rowreader.h"	/* the reader of the any-format kernel */

STROM_DEVICE pg_bool_t
gpuscan_qual_eval(cl_int *errcode,
				  const strom_kparams &KP,
				  const strom_kvars &KV);

STROM_DEVICE void
gpuscan_load_kparams(strom_kparams &KP, const kern_parambuf *kparams, cl_int *errcode)
{
#define X(idx,NAME)	KP.KPARAM_##idx = pg_##NAME##_param(kparams, errcode, idx);
	STROM_KPARAM_LIST(X)
#undef X
	KP.__dummy = 0;
}

/* row status -> +1 pass, -1 recheck, 0 drop; significant errors accumulate */
STROM_DEVICE int
gpuscan_row_status(pg_bool_t rc, cl_int errcode, cl_int *chunk_error)
{
	STROM_SET_ERROR(&errcode, (!rc.isnull && rc.value != 0)
					? StromError_Success : StromError_RowFiltered);
	if (errcode == StromError_Success)
		return 1;
	if (errcode == StromError_CpuReCheck)
		return -1;
	if (StromErrorIsSignificant(errcode))
		STROM_SET_ERROR(chunk_error, errcode);
	return 0;
}

/* ---- LDS stage shared by both kernels ---------------------------------- */
template <int NENTRIES>
struct gpuscan_stage_t {
	cl_int		entries[NENTRIES];
	cl_uint		wave_total[GPUSCAN_QUADS][GPUSCAN_NWAVES];
	cl_uint		flush_base;
};
typedef gpuscan_stage_t<GPUSCAN_STAGE> gpuscan_stage;
/* the row-at-a-time kernel's stage: measured, a shallow stage (2048 entries,
 * twice the resident waves) is SLOWER than the deep one (630 vs 390 us per
 * 1e7 rows) -- more flushes mean more reservations on the one result cursor */
#ifndef GPUSCAN_GENERIC_STAGE
#define GPUSCAN_GENERIC_STAGE	GPUSCAN_STAGE
#endif
typedef gpuscan_stage_t<GPUSCAN_GENERIC_STAGE> gpuscan_generic_stage;

/*
 * One entry of results[]: written once and read elsewhere.  GPUSCAN_STORE_NT=1
 * (default): non-temporal stores keep them out of the L2 write-allocate path
 * of the read stream (+5 % at 10 % selectivity, +8 % at 49 %:
 * profiles/r01_gpuscan_tune_v2.txt).  0: plain stores.  2: write-through
 * (agent-scope relaxed atomic stores, sc1), which leave no dirty line for the
 * end of the kernel to write back.
 */
STROM_DEVICE void
gpuscan_store_result(cl_int *p, cl_int v)
{
#if !defined(GPUSCAN_STORE_NT) || GPUSCAN_STORE_NT == 1
	__builtin_nontemporal_store(v, p);
#elif GPUSCAN_STORE_NT == 2
	__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
	*p = v;
#endif
}

/* 'cursor' counts the entries of results[] (kern_resultbuf.nitems, or the low
 * half of the resident kernel's ring slot word) */
template <typename STAGE, typename CURSOR>
STROM_DEVICE void
gpuscan_stage_flush(STAGE &stage, CURSOR *cursor, cl_int *results, cl_uint nrooms, cl_uint fill)
{
	/* caller guarantees a barrier since the last write into the stage */
	if (fill == 0)
		return;
#if (defined(GPUSCAN_ABLATE) && GPUSCAN_ABLATE != 0) && !defined(STROM_DIAGNOSTIC_BUILD)
#error "GPUSCAN_ABLATE builds leave work out and give wrong results: measurement only (set STROM_DIAGNOSTIC_BUILD=1, as scripts/gpu_*_ablate* do)"
#endif
#if defined(GPUSCAN_ABLATE) && GPUSCAN_ABLATE == 2
	/* diagnostic build (wrong results): no reservation atomic */
	if (threadIdx.x == 0)
		stage.flush_base = (blockIdx.x * 7919u) % (nrooms - GPUSCAN_STAGE);
#else
	if (threadIdx.x == 0)
		stage.flush_base = (cl_uint)atomicAdd(cursor, (CURSOR)fill);
#endif
	__syncthreads();
	cl_uint		base = stage.flush_base;
	cl_int	   *dest = results + base;
#if !defined(GPUSCAN_ABLATE) || GPUSCAN_ABLATE != 1
	for (cl_uint i = threadIdx.x; i < fill; i += GPUSCAN_BLOCK)
		gpuscan_store_result(&dest[i], stage.entries[i]);
#else
	/* diagnostic build (wrong results): no result stores */
	if (fill == 0xffffffffu)
		dest[0] = stage.entries[0];
#endif
	__syncthreads();
}

/*
 * Compaction of one tile.  st[k][j] is the status of row
 * (tile_base + (k*BLOCK + tid)*4 + j).  Entries land in the stage in row
 * order: (k, wave, lane, j).  Returns the number of entries appended; the
 * value is identical in every thread.
 */
/* LANE_ROWS: st[k][j] belongs to row tile_base + (k*4 + j)*BLOCK + tid instead -- consecutive
 * lanes, consecutive rows (the row-at-a-time kernel: neighbouring lanes then walk neighbouring
 * heap tuples) */
template <bool LANE_ROWS = false, typename STAGE>
STROM_DEVICE cl_uint
gpuscan_stage_append(STAGE &stage, cl_uint fill,
					 cl_uint tile_base, const int (&st)[GPUSCAN_QUADS][4])
{
	cl_uint		lane = threadIdx.x & (STROM_WAVE - 1);
	cl_uint		wave = threadIdx.x / STROM_WAVE;
	cl_uint		my_prefix[GPUSCAN_QUADS];

#pragma unroll
	for (int k = 0; k < GPUSCAN_QUADS; k++)
	{
		cl_uint	prefix = 0, total = 0;
#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			strom_lanemask_t m = __ballot(st[k][j] != 0);
			prefix += strom_mbcnt(m);
			total += __popcll(m);
		}
		my_prefix[k] = prefix;
		if (lane == 0)
			stage.wave_total[k][wave] = total;
	}
	__syncthreads();

	cl_uint		appended = 0;
#pragma unroll
	for (int k = 0; k < GPUSCAN_QUADS; k++)
	{
		cl_uint	before = 0, all = 0;
#pragma unroll
		for (int w = 0; w < GPUSCAN_NWAVES; w++)
		{
			cl_uint	t = stage.wave_total[k][w];
			before += (w < (int)wave ? t : 0);
			all += t;
		}
		cl_uint	pos = fill + appended + before + my_prefix[k];
		cl_uint	row0 = tile_base + (k * GPUSCAN_BLOCK + threadIdx.x) * 4;
#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			if (st[k][j] != 0)
			{
				cl_int	rowid = (LANE_ROWS
								 ? (cl_int)(tile_base + (k * 4 + j) * GPUSCAN_BLOCK + threadIdx.x + 1)
								 : (cl_int)(row0 + j + 1));
				stage.entries[pos++] = (st[k][j] > 0 ? rowid : -rowid);
			}
		}
		appended += all;
	}
	/* the next append rewrites wave_total[]; entries[] are read by flush */
	__syncthreads();
	return appended;
}

/* ====================================================================== *
 * COLUMN format, streaming
 * ====================================================================== */
struct gpuscan_column_tile {
#define X(attno,colidx,NAME)											\
	pg_##NAME##_base_t	v_##attno[GPUSCAN_QUADS][4];						\
	cl_uint				nn_##attno[GPUSCAN_QUADS];
	STROM_KVAR_LIST(X)
#undef X
	int __dummy;
};

/* returns the entries still in the stage (a barrier has passed since they were
 * written); the chunk's error is written back */
template <typename CURSOR>
STROM_DEVICE cl_uint
gpuscan_column_body(gpuscan_stage &stage,
					const kern_parambuf *kparams,
					const kern_data_store *kds,
					CURSOR *cursor, cl_int *results, cl_uint nrooms, cl_int *errword)
{
	const kern_coldir *coldir = KERN_DATA_STORE_COLDIR(kds);
	cl_uint		nitems = kds->nitems;
	cl_uint		ntiles = (nitems + GPUSCAN_TILE_ROWS - 1) / GPUSCAN_TILE_ROWS;
	cl_int		chunk_error = StromError_Success;
	cl_int		param_error = StromError_Success;
	cl_uint		fill = 0;
	strom_kparams KP;

	gpuscan_load_kparams(KP, kparams, &param_error);

	/* column base pointers, hoisted */
#define X(attno,colidx,NAME)													\
	const char *col_##attno = (const char *)kds + coldir[colidx].values_off;	\
	const cl_uint *nul_##attno = (coldir[colidx].nulls_off != 0					\
		? (const cl_uint *)((const char *)kds + coldir[colidx].nulls_off) : NULL);
	STROM_KVAR_LIST(X)
#undef X
	bool		any_nulls = false;		/* wave-uniform: picks the bitmap-free loader */
#define X(attno,colidx,NAME)	any_nulls = any_nulls || (nul_##attno != NULL);
	STROM_KVAR_LIST(X)
#undef X

	for (cl_uint tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
	{
		cl_uint		tile_base = tile * GPUSCAN_TILE_ROWS;
		bool		full_tile = (tile_base + GPUSCAN_TILE_ROWS <= nitems);
		gpuscan_column_tile T;
		int			st[GPUSCAN_QUADS][4];

		/* issue every load of the tile before the first use */
		if (full_tile && !any_nulls)
		{
#pragma unroll
			for (int k = 0; k < GPUSCAN_QUADS; k++)
			{
				cl_uint	row0 = tile_base + (k * GPUSCAN_BLOCK + threadIdx.x) * 4;
#define X(attno,colidx,NAME)													\
				strom_column_load_quad<pg_##NAME##_base_t, true, true>(col_##attno, nul_##attno,	\
														   row0, nitems,				\
														   T.v_##attno[k], T.nn_##attno[k]);
				STROM_KVAR_LIST(X)
#undef X
			}
		}
		else if (full_tile)
		{
#pragma unroll
			for (int k = 0; k < GPUSCAN_QUADS; k++)
			{
				cl_uint	row0 = tile_base + (k * GPUSCAN_BLOCK + threadIdx.x) * 4;
#define X(attno,colidx,NAME)													\
				strom_column_load_quad<pg_##NAME##_base_t, true>(col_##attno, nul_##attno,	\
														   row0, nitems,				\
														   T.v_##attno[k], T.nn_##attno[k]);
				STROM_KVAR_LIST(X)
#undef X
			}
		}
		else
		{
#pragma unroll
			for (int k = 0; k < GPUSCAN_QUADS; k++)
			{
				cl_uint	row0 = tile_base + (k * GPUSCAN_BLOCK + threadIdx.x) * 4;
#define X(attno,colidx,NAME)													\
				strom_column_load_quad<pg_##NAME##_base_t, false>(col_##attno, nul_##attno,	\
														   row0, nitems,				\
														   T.v_##attno[k], T.nn_##attno[k]);
				STROM_KVAR_LIST(X)
#undef X
			}
		}
		if (fill + GPUSCAN_TILE_ROWS > GPUSCAN_STAGE)
		{
			gpuscan_stage_flush(stage, cursor, results, nrooms, fill);
			fill = 0;
		}
#pragma unroll
		for (int k = 0; k < GPUSCAN_QUADS; k++)
		{
			cl_uint	row0 = tile_base + (k * GPUSCAN_BLOCK + threadIdx.x) * 4;
#pragma unroll
			for (int j = 0; j < 4; j++)
			{
				strom_kvars	KV;
				cl_int		errcode = param_error;
#define X(attno,colidx,NAME)													\
				KV.KVAR_##attno = pg_##NAME##_make(T.v_##attno[k][j],				\
												   !((T.nn_##attno[k] >> j) & 1));
				STROM_KVAR_LIST(X)
#undef X
				KV.__dummy = 0;
				strom_kvars_from_column(KV, kds, &errcode);
				pg_bool_t rc = gpuscan_qual_eval(&errcode, KP, KV);
				st[k][j] = (row0 + j < nitems
							? gpuscan_row_status(rc, errcode, &chunk_error) : 0);
			}
		}
		fill += gpuscan_stage_append(stage, fill, tile_base, st);
	}
	kern_writeback_error_status(errword, chunk_error);
	return fill;
}

/* the request head in device memory (host chunks, the copied path) */
extern "C" __global__ void
__launch_bounds__(GPUSCAN_BLOCK)
gpuscan_qual_column(kern_gpuscan *kgpuscan, const kern_data_store *kds)
{
	__shared__ gpuscan_stage stage;
	kern_resultbuf *kresults = KERN_GPUSCAN_RESULTBUF(kgpuscan);

	cl_uint		fill = gpuscan_column_body(stage, KERN_GPUSCAN_PARAMBUF(kgpuscan), kds, &kresults->nitems,
										   kresults->results, kresults->nrooms, &kresults->errcode);
	gpuscan_stage_flush(stage, &kresults->nitems, kresults->results, kresults->nrooms, fill);
}

/*
 * resident chunk: the parambuf is the kernel argument, and the cursor and the
 * error word live in a ring slot.  The slot's cursor word counts reserved
 * entries in its low half and finished work-groups in its high half, so a
 * work-group's last reservation is also its ticket: the one that draws the
 * last ticket knows nitems without another atomic, publishes the result head
 * -- into the device kern_resultbuf (row maps and chained operators read it
 * there) and into the request's pinned host words -- and leaves the slot zero
 * for its next request.
 */
extern "C" __global__ void
__launch_bounds__(GPUSCAN_BLOCK)
gpuscan_qual_column_resident(kern_gpuscan_column_args args)
{
	__shared__ gpuscan_stage stage;
	__shared__ bool	last;
	kern_gpuscan_slot *slot = args.slot;
	cl_int	   *results = args.kresults->results;
	cl_uint		fill = gpuscan_column_body(stage, (const kern_parambuf *)args.kparams, args.kds,
										   &slot->cursor, results, args.res_head[1], &slot->errcode);
	/*
	 * __syncthreads() alone waits for no vector-memory counter on this chip.  So every wave
	 * first waits until its own memory operations are acknowledged -- the error word's
	 * compare-and-swap above all, which may be issued without a return -- and only then
	 * meets the barrier: the work-group's error word and reservations are performed before
	 * its ticket is drawn.  What the last work-group reads are atomics at the device's
	 * coherence point, so no agent-scope release fence is needed (on this chip one writes
	 * back the XCD's L2, once per work-group: measured 650 instead of 200 us per 1e8-row
	 * chunk).  Same wait as STROM_PUBLISH_STATE (strom_common.h), same formal fallback.
	 */
#if STROM_FORMAL_PUBLISH
	__threadfence();
#else
	__builtin_amdgcn_s_waitcnt(0x0f70);		/* vmcnt(0) in the gfx9 encoding */
#endif
	__syncthreads();
	if (threadIdx.x == 0)
	{
		cl_ulong	old = atomicAdd(&slot->cursor, (1UL << 32) + fill);
		stage.flush_base = (cl_uint)old;
		last = ((cl_uint)(old >> 32) == gridDim.x - 1);
	}
	__syncthreads();
	cl_int	   *dest = results + stage.flush_base;
	for (cl_uint i = threadIdx.x; i < fill; i += GPUSCAN_BLOCK)
		gpuscan_store_result(&dest[i], stage.entries[i]);
	if (threadIdx.x == 0 && last)
	{
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
		cl_uint		nitems = stage.flush_base + fill;
		cl_int		errcode = __hip_atomic_load(&slot->errcode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		cl_uint	   *head = (cl_uint *)args.kresults;

		head[0] = args.res_head[0];			/* nrels */
		head[1] = args.res_head[1];			/* nrooms */
		head[2] = nitems;
		head[3] = (cl_uint)errcode;
		head[4] = args.res_head[4];			/* has_rechecks, all_visible */
		__hip_atomic_store(&args.host_slot[0], nitems, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		__hip_atomic_store(&args.host_slot[1], (cl_uint)errcode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		__hip_atomic_store(&slot->cursor, (cl_ulong)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__hip_atomic_store(&slot->errcode, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

/* ====================================================================== *
 * any format, optional row map: one datum at a time
 * ====================================================================== */
template <bool IS_COLUMN>
__device__ __forceinline__ void
gpuscan_qual_generic_body(kern_gpuscan *kgpuscan,
					 const kern_data_store *kds,
					 const kern_data_store *ktoast,
					 const kern_row_map *krowmap,
					 gpuscan_generic_stage &stage)
{
	const kern_parambuf *kparams = KERN_GPUSCAN_PARAMBUF(kgpuscan);
	kern_resultbuf *kresults = KERN_GPUSCAN_RESULTBUF(kgpuscan);
	STROM_ROW_READER_MAP(kds, krowmap);
	const bool	use_map = rr_use_map;
	const cl_uint nrows = rr_nrows;
	cl_uint		ntiles = (nrows + GPUSCAN_TILE_ROWS - 1) / GPUSCAN_TILE_ROWS;
	cl_int		chunk_error = StromError_Success;
	cl_int		param_error = StromError_Success;
	cl_uint		fill = 0;
	strom_kparams KP;

	gpuscan_load_kparams(KP, kparams, &param_error);
	STROM_ROW_READER(IS_COLUMN, kds, ktoast);		/* fixed per launch (strom_rowreader.h) */

	for (cl_uint tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
	{
		cl_uint		tile_base = tile * GPUSCAN_TILE_ROWS;
		int			st[GPUSCAN_QUADS][4];

		if (fill + GPUSCAN_TILE_ROWS > GPUSCAN_GENERIC_STAGE)
		{
			gpuscan_stage_flush(stage, &kresults->nitems, kresults->results, kresults->nrooms, fill);
			fill = 0;
		}
#pragma unroll
		for (int k = 0; k < GPUSCAN_QUADS; k++)
		{
#pragma unroll
			for (int j = 0; j < 4; j++)
			{
				/*
				 * consecutive lanes, consecutive rows: with a quad of rows per lane (the
				 * streaming kernel's layout) a wave's 64 lanes reach for heap tuples 4 rows
				 * apart -- 80 cache lines per load of a 40-byte-tuple table instead of 20
				 */
				cl_uint		r = tile_base + (k * 4 + j) * GPUSCAN_BLOCK + threadIdx.x;

				st[k][j] = 0;
				if (r < nrows)
				{
					strom_kvars	KV;
					cl_int		errcode = param_error;
					STROM_ROW_LOAD_ROW(KV, errcode, STROM_ROW_INDEX(r));
					pg_bool_t rc = gpuscan_qual_eval(&errcode, KP, KV);
					st[k][j] = gpuscan_row_status(rc, errcode, &chunk_error);
				}
			}
		}
		/*
		 * with a row map the reported id is the position in the map's
		 * input order translated back to the chunk's row: patch below
		 */
		if (!use_map)
			fill += gpuscan_stage_append<true>(stage, fill, tile_base, st);
		else
		{
			cl_uint	before = fill;
			cl_uint	n = gpuscan_stage_append<true>(stage, fill, tile_base, st);
			/* translate map positions -> chunk rows, in place */
			for (cl_uint i = before + threadIdx.x; i < before + n; i += GPUSCAN_BLOCK)
			{
				cl_int	e = stage.entries[i];
				cl_int	pos = (e > 0 ? e : -e) - 1;
				cl_int	rowid = krowmap->rindex[pos] + 1;
				stage.entries[i] = (e > 0 ? rowid : -rowid);
			}
			__syncthreads();
			fill += n;
		}
	}
	gpuscan_stage_flush(stage, &kresults->nitems, kresults->results, kresults->nrooms, fill);
	kern_writeback_error_status(&kresults->errcode, chunk_error);
}

extern "C" __global__ void
__launch_bounds__(GPUSCAN_BLOCK)
gpuscan_qual_generic(kern_gpuscan *kgpuscan,
					 const kern_data_store *kds,
					 const kern_data_store *ktoast,
					 const kern_row_map *krowmap)
{
	__shared__ gpuscan_generic_stage stage;

	/* the chunk format is decided once per launch, not once per datum */
	if (kds->format == KDS_FORMAT_COLUMN)
		gpuscan_qual_generic_body<true>(kgpuscan, kds, ktoast, krowmap, stage);
	else
		gpuscan_qual_generic_body<false>(kgpuscan, kds, ktoast, krowmap, stage);
}

#endif	/* STROM_GPUSCAN_DEVICE_H */
