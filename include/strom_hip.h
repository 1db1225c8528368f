/*
 * strom_hip.h -- C ABI of libstrom_hip.so, the HIP device runtime that
 * stands where the reference's OpenCL server stands.
 *
 * Every entry point names the reference interface it replaces.  The
 * reference's boundary is a message protocol (pgstrom_message,
 * pg_strom.h:238-248; mqueue.c): a backend fills a request object, the
 * server thread runs msg->cb_process() which must only *enqueue* device
 * work, and a runtime thread later stores msg->errcode and replies.  The
 * same contract is kept here as plain functions:
 *
 *     strom_submit_*()   ==  pgstrom_enqueue_message() + clserv_process_*()
 *     strom_done_cb      ==  clserv_respond_*() + pgstrom_reply_message()
 *
 * No torch / C++ types cross this boundary; pointers are host pointers to
 * the wire structs of strom_kds.h unless named strom_dstore (a chunk kept
 * resident in HBM).
 */
#ifndef STROM_HIP_H
#define STROM_HIP_H

#include "strom_kds.h"
#include "strom_codegen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ *
 * extra_flags of a device program (pg_strom.h:263-274)
 * ------------------------------------------------------------------ */
#define DEVINFO_IS_NEGATIVE			0x0001
#define DEVTYPE_IS_VARLENA			0x0002
#define DEVTYPE_IS_BUILTIN			0x0004
#define DEVFUNC_NEEDS_TIMELIB		0x0008
#define DEVFUNC_NEEDS_TEXTLIB		0x0010
#define DEVFUNC_NEEDS_NUMERIC		0x0020
#define DEVFUNC_NEEDS_MATHLIB		0x0040
#define DEVFUNC_INCL_FLAGS			0x0078
#define DEVKERNEL_DISABLE_OPTIMIZE	0x0100
#define DEVKERNEL_NEEDS_GPUSCAN		0x0200
#define DEVKERNEL_NEEDS_HASHJOIN	0x0400
#define DEVKERNEL_NEEDS_GPUPREAGG	0x0800

/* ------------------------------------------------------------------ *
 * perfmon: same fields as pgstrom_perfmon (pg_strom.h:177-213); times in
 * microseconds like the reference (gettimeofday / CL profiling -> usec)
 * ------------------------------------------------------------------ */
typedef struct {
	cl_bool		enabled;
	cl_uint		num_samples;
	cl_ulong	time_inner_load;
	cl_ulong	time_outer_load;
	cl_ulong	time_materialize;
	cl_ulong	time_in_sendq;
	cl_ulong	time_in_recvq;
	cl_ulong	time_kern_build;
	cl_uint		num_dma_send;
	cl_uint		num_dma_recv;
	cl_ulong	bytes_dma_send;
	cl_ulong	bytes_dma_recv;
	cl_ulong	time_dma_send;
	cl_ulong	time_dma_recv;
	cl_uint		num_kern_exec;
	cl_ulong	time_kern_exec;
	cl_uint		num_kern_proj;
	cl_ulong	time_kern_proj;
	cl_uint		num_kern_prep;
	cl_uint		num_kern_sort;
	cl_ulong	time_kern_prep;
	cl_ulong	time_kern_sort;
	/* extension: kernel time in nanoseconds (HIP events resolve < 1us).
	 * GpuScan over a resident COLUMN chunk (gpuscan_qual_column_resident): consecutive such
	 * scans of a device run on two streams and overlap at their boundary, so the time of
	 * scan N is EXCLUSIVE of the device's previous resident scan P:
	 *     end(N) - max(begin(N), end(P)),  kept within [0, end(N) - begin(N)]
	 * With one scan stream (STROM_GPUSCAN_SCAN_STREAMS=1), or with nothing to overlap, that
	 * is end(N) - begin(N).  Summed over a run of scans it is the span the device was busy
	 * with them: bytes / time stays a bandwidth.  time_kern_exec is the same in microseconds. */
	cl_ulong	time_kern_exec_ns;
	cl_ulong	time_kern_prep_ns;
	cl_ulong	time_kern_proj_ns;
} strom_perfmon;

/* ------------------------------------------------------------------ *
 * life cycle  (opencl_serv.c:156-215 init_opencl_context_and_shmem,
 *              224-305 pgstrom_opencl_main; shutdown 412-430)
 * device_ids == NULL: use the device HIP reports as current (one process
 * per GPU under torch.distributed sets it through LOCAL_RANK).
 * ------------------------------------------------------------------ */
int			strom_init(const int *device_ids, int ndevices);
void		strom_shutdown(void);
int			strom_num_devices(void);
/* round-robin device pick (opencl_serv.c:100-106) */
int			strom_device_schedule(void);
/* pgstrom_strerror (main.c:288-328) */
const char *strom_strerror(int errcode);
/* pin a host range so DMA is direct (opencl_serv.c:115-137) */
int			strom_pin_host_range(void *ptr, size_t length);
int			strom_unpin_host_range(void *ptr);
/* device properties the reference prints via pgstrom_opencl_device_info */
int			strom_device_info(int dindex, char *buf, size_t buflen);
/* GUC-like switch: pg_strom.perfmon (main.c:116-123) */
void		strom_set_perfmon(int enabled);

/* ------------------------------------------------------------------ *
 * device program cache  (opencl_devprog.c)
 *   strom_get_devprog_key      <- pgstrom_get_devprog_key      (580-659)
 *   strom_retain/put           <- pgstrom_retain/put_devprog_key (669-697)
 *   strom_get_devprog_errmsg   <- pgstrom_get_devprog_errmsg   (708-720)
 *   strom_lookup_device_program<- clserv_lookup_device_program (270-569)
 * A key is the handle the reference stores as 'Datum dprog_key'.  The
 * build (hiprtc, --offload-arch=gfx950) starts asynchronously on first
 * reference; requests submitted while it runs are parked and re-issued
 * when it ends, as the reference parks messages on the program's wait
 * queue.
 * ------------------------------------------------------------------ */
typedef uint64_t strom_devprog_key;

#define STROM_DEVPROG_READY		1
#define STROM_DEVPROG_PENDING	0
#define STROM_DEVPROG_BAD		(-1)	/* BAD_OPENCL_PROGRAM, pg_strom.h:587 */

strom_devprog_key strom_get_devprog_key(const char *source, int32_t extra_flags);
void		strom_retain_devprog_key(strom_devprog_key key);
void		strom_put_devprog_key(strom_devprog_key key);
const char *strom_get_devprog_errmsg(strom_devprog_key key);
int			strom_lookup_device_program(strom_devprog_key key, int wait);
/* the full text handed to the compiler: pg_strom.show_device_kernel */
const char *strom_get_devprog_source(strom_devprog_key key);

/* ------------------------------------------------------------------ *
 * device-resident chunks.  The reference re-sends a chunk for every
 * request (clserv_dmasend_data_store, datastore.c:837-973); a strom_dstore
 * is the same bytes kept in HBM so that a table can be scanned again (and
 * chained operators can share it) without crossing PCIe.
 * ------------------------------------------------------------------ */
typedef struct strom_dstore strom_dstore;

strom_dstore *strom_dstore_upload(const kern_data_store *kds, int dindex);
/* adopt device memory somebody else filled (e.g. a torch tensor): no copy,
 * not freed on release */
strom_dstore *strom_dstore_wrap(void *devptr, size_t length, int dindex);
void	   *strom_dstore_devptr(strom_dstore *ds);
size_t		strom_dstore_length(strom_dstore *ds);
void		strom_dstore_release(strom_dstore *ds);
/* copy the first 'length' bytes of the chunk image back to the host */
int			strom_dstore_download(strom_dstore *ds, void *host, size_t length);
/*
 * Transpose a resident ROW / ROW_FLAT / TUPSLOT chunk (fixed-width columns)
 * into a new resident KDS_FORMAT_COLUMN chunk on the device -- the step the
 * reference has no need for because its kernels walk heap tuples
 * (kern_get_datum_rs, opencl_common.h:886-907).  'type_oids' (ncols
 * entries, may be NULL) enables the zone maps GpuPreAgg / GpuHashJoin use.
 * A numeric column tagged STROM_NUMERICOID becomes the 8-byte device form;
 * tagged STROM_DECIMAL_TYPE(scale) -- a typmod-scaled numeric(p,s) -- it
 * becomes a DECIMAL column, int8 at 10^-scale, which programs read as
 * (var N decimal S) without any per-row decode (exact, or the whole
 * conversion answers StromError_CpuReCheck and the chunk stays as it is).
 * Blocks until the chunk is ready; *p_kern_ns receives the device time.
 */
strom_dstore *strom_dstore_to_column(strom_dstore *src, const int32_t *type_oids, int ntypes,
									 uint64_t *p_kern_ns, int *p_errcode);

/* ------------------------------------------------------------------ *
 * requests
 * ------------------------------------------------------------------ */
/*
 * Completion protocol (pgstrom_message, pg_strom.h:238-248; mqueue.c:140-183,
 * 533-554).  'done', when not NULL, is invoked exactly once per accepted
 * request, always on a runtime thread (never on the submitter's stack, also
 * when the request fails before any device work), after errcode, perfmon and
 * the host result image (kern_resultbuf / kds_dest) are final -- the
 * reference's clserv_respond_*() + pgstrom_reply_message().  The returned
 * handle is the message reference the backend keeps: it stays valid until
 * strom_task_wait() / strom_task_release() (pgstrom_put_message()), with or
 * without a callback, so results left in HBM can be chained after the
 * callback fired.  strom_task_wait() may be called from inside done().
 * A submit call that returns NULL (with *p_errcode set) never calls done.
 */
typedef void (*strom_done_cb)(void *arg, int errcode, const strom_perfmon *pfm);
typedef struct strom_task strom_task;

/* request flags */
#define STROM_RESULTS_ON_DEVICE		0x0001	/* leave results[] in HBM; copy
											 * back only the resultbuf head */

/*
 * GpuScan on one chunk.
 *   <- clserv_process_gpuscan (gpuscan.c:1895-2182) + clserv_respond_gpuscan
 *      (1760-1888).  'kgpuscan' is the host image {kern_parambuf,
 *      kern_resultbuf}; the head up to results[] is sent, and
 *      kern_resultbuf{nitems, errcode, results[0..nitems)} is written back
 *      into the same host memory before done() runs.
 * Exactly one of kds (host chunk, uploaded for this request) or kds_dev
 * (resident chunk) is non-NULL.  Returns NULL and sets *p_errcode when the
 * request cannot be queued.  'done' may be NULL; either way the handle is
 * given back with strom_task_wait() / strom_task_release().
 */
strom_task *strom_submit_gpuscan(strom_devprog_key key,
								 kern_gpuscan *kgpuscan,
								 const kern_data_store *kds,
								 strom_dstore *kds_dev,
								 const kern_row_map *krowmap,
								 uint32_t flags,
								 strom_done_cb done, void *arg,
								 int *p_errcode);

/* ------------------------------------------------------------------ *
 * GpuPreAgg
 *
 * The reference reduces one chunk per request and ships one partial row
 * per (work-group, group) back to the backend, whose Agg node finishes
 * with the pgstrom.* final aggregates (gpupreagg.c:2665-2776, 3849-4240;
 * pg_strom--1.0.sql:247-401).  Here a strom_gpupreagg is a reduction in
 * progress on one GPU: chunks are folded into a table that stays in HBM
 * and strom_gpupreagg_fetch() returns ONE partial row per group in the
 * reference's result format (TUPSLOT kern_data_store, group keys and
 * partial values in target-list order).  Those rows feed the same final
 * aggregates, so the final result is the reference's.  With several GPUs
 * the per-GPU tables have identical layout and are merged with an RCCL
 * all-reduce on the table itself (strom_gpupreagg_table_devptr).
 *
 * nrows() partials are int8 in the fetched rows (the reference's are
 * int4 per chunk; a whole-table count does not fit int4).
 * ------------------------------------------------------------------ */
typedef struct strom_gpupreagg strom_gpupreagg;

#define STROM_PREAGG_MAXKEYS	8
typedef struct {
	int32_t		nkeys;
	int64_t		key_min[STROM_PREAGG_MAXKEYS];
	uint32_t	key_range[STROM_PREAGG_MAXKEYS];	/* max - min + 1 */
} strom_preagg_domain;

/* domain == NULL: taken from the first chunk's zone maps (COLUMN) or a
 * min/max pre-pass (other formats).  table_devptr == NULL: the runtime
 * allocates the resident table; otherwise the caller's buffer of
 * strom_gpupreagg_table_length() bytes is used (e.g. a torch tensor that
 * RCCL reduces in place). */
strom_gpupreagg *strom_gpupreagg_create(strom_devprog_key key,
										const strom_preagg_target *targets, int ntargets,
										const kern_parambuf *kparams,
										const strom_preagg_domain *domain,
										int dindex, int *p_errcode);
size_t		strom_gpupreagg_table_length(strom_gpupreagg *sess);
int			strom_gpupreagg_bind_table(strom_gpupreagg *sess, void *table_devptr);
void	   *strom_gpupreagg_table_devptr(strom_gpupreagg *sess);
uint32_t	strom_gpupreagg_num_groups(strom_gpupreagg *sess);
/*
 * Integer partial sums never wrap silently -- CHECK_OVERFLOW_INT of the reference's
 * GPUPREAGG_AGGCALC_PSUM_TEMPLATE (opencl_gpupreagg.h:142-143, 933-948) answers CpuReCheck
 * when an accumulate leaves int8.  Here a range proof (rows x largest input magnitude
 * < 2^63) lets unchecked kernels run; a chunk it cannot cover is folded a second time,
 * add by add, by a program built with GPUPREAGG_CHECKED, inside the same request
 * (devlib/strom_gpupreagg.h, "integer sums never wrap"; hashed sessions fold such a chunk
 * into a scratch table that way and let its groups join the table under a per-group check:
 * exact there too, and a CpuReCheck leaves the table as it was).  How many requests of this session
 * took that second fold: a statistic (EXPLAIN ANALYZE material, like the reference's perfmon).
 */
uint32_t	strom_gpupreagg_checked_folds(strom_gpupreagg *sess);
/*
 * The range proof's input for a sum over an EXPRESSION: the code generator emits a bound formula over
 * the columns' zone maps (#define GPUPREAGG_SUMBOUND_<a> "..." in the generated source: reverse Polish
 * over magnitudes -- cN / nN a column's zone map / integer-part bounds, kV a constant, + and *, eK a
 * rescale by 10^K); the launch path evaluates it per COLUMN chunk instead of measuring every row.
 * This is that evaluation, for a host-resident chunk: bits of the largest magnitude, or -1.
 */
int			strom_gpupreagg_sum_bound_bits(const char *formula, const kern_data_store *kds);
/* byte offset / element kind of target 'resno' inside the table:
 * *p_bits_off  offset of its has-value bitmap (seen bitmap for keys)
 * *p_vals_off  offset of its 8-byte value array (0 for keys)          */
int			strom_gpupreagg_table_layout(strom_gpupreagg *sess, int resno,
										 size_t *p_bits_off, size_t *p_vals_off);
/*
 * fold one chunk  <- clserv_process_gpupreagg (gpupreagg.c:3849-4240).
 * The task's errcode is 0, StromError_CpuReCheck (the chunk was NOT folded:
 * the caller re-does it on the CPU like gpupreagg_next_tuple_fallback,
 * gpupreagg.c:2507-2607) or a significant error.
 */
strom_task *strom_submit_gpupreagg(strom_gpupreagg *sess,
								   const kern_data_store *kds,
								   strom_dstore *kds_dev,
								   const kern_row_map *krowmap,
								   strom_done_cb done, void *arg,
								   int *p_errcode);
/* partial rows, one per group, as a TUPSLOT kern_data_store.  Returns the
 * bytes needed when dest == NULL; the number of groups (>= 0) otherwise;
 * a negative StromError on failure. */
long		strom_gpupreagg_fetch(strom_gpupreagg *sess, kern_data_store *dest, size_t destlen);
/*
 * Group-slot agreement ("agree on dense group slots").
 * Zone maps bound every key on its own; the product of the ranges can be far
 * larger than the combinations that occur.  strom_gpupreagg_census() marks,
 * one bit per dense id, the ids of the rows of a chunk that pass the qual
 * (accumulating over calls; a copy is returned in bitmap_out when not NULL,
 * strom_gpupreagg_dense_groups() ids -> (n+31)/32 words).  The caller may
 * OR the bitmaps of several ranks.  strom_gpupreagg_compact() then maps the
 * marked ids (bitmap == NULL: the session's own census) to consecutive table
 * slots; it must precede the first fold.  A later row whose combination was
 * not marked fails its chunk with StromError_DataStoreOutOfRange.
 */
uint32_t	strom_gpupreagg_dense_groups(strom_gpupreagg *sess);
int			strom_gpupreagg_census(strom_gpupreagg *sess,
								   const kern_data_store *kds, strom_dstore *kds_dev,
								   const kern_row_map *krowmap,
								   uint32_t *bitmap_out, size_t nwords);
int			strom_gpupreagg_compact(strom_gpupreagg *sess, const uint32_t *bitmap, size_t nwords);
/*
 * hashed GROUP BY: keys of ANY device type (float4/float8/numeric as well)
 * and any spread.  The reference sorts row indexes by gpupreagg_keycomp and
 * reduces runs of equal keys (opencl_gpupreagg.h:620-856, bitonic steps
 * driven from gpupreagg.c:3955-4120); here the groups live in an
 * open-addressing table in HBM keyed by the keys' canonical 64-bit images
 * (-0 = +0, one NaN, stripped numerics), grown by the library as the group
 * count needs.  A session made by this call takes the same
 * strom_submit_gpupreagg*() / strom_gpupreagg_fetch() / _reset() / _release()
 * calls; the dense-table calls (table_length, bind_table, table_devptr,
 * table_layout, census, compact) answer BadRequest / 0 for it, and
 * strom_gpupreagg_num_groups() returns the groups seen so far.  Sessions of
 * several ranks are merged by concatenating their partial rows: the final
 * aggregate adds them up (pg_strom--1.0.sql:247-401).
 * ngroups_hint sizes the first table (0 = default) and picks the number of
 * hash roles of the first fold.  The hashed kernels are a device program of
 * their own, derived from 'key' by the library (its source behind
 * "#define GPUPREAGG_HASHED 1"); it builds in the background and the first
 * fold waits for it.  A caller may also pass the key of that derived program.
 */
strom_gpupreagg *strom_gpupreagg_create_hashed(strom_devprog_key key,
											   const strom_preagg_target *targets, int ntargets,
											   const kern_parambuf *kparams,
											   uint32_t ngroups_hint,
											   int dindex, int *p_errcode);
void		strom_gpupreagg_reset(strom_gpupreagg *sess);
void		strom_gpupreagg_release(strom_gpupreagg *sess);
/*
 * The dense domain of ONE chunk: per group key the min and the range of the
 * values its rows carry after the qual (kernel gpupreagg_keyrange; any chunk
 * format, key expressions included).  Blocking, planning time.  Answers
 * StromError_DataStoreOutOfRange when the keys have no dense ids (float /
 * numeric keys, a spread beyond 32 bits): such a query takes
 * strom_gpupreagg_create_hashed().
 */
int			strom_gpupreagg_chunk_domain(strom_devprog_key key,
										 const strom_preagg_target *targets, int ntargets,
										 const kern_parambuf *kparams,
										 const kern_data_store *kds, strom_dstore *kds_dev,
										 const kern_row_map *krowmap,
										 int dindex, strom_preagg_domain *domain_out);
/*
 * The reference's own per-chunk message, field by field:
 *   pgstrom_gpupreagg {msg, dprog_key, needs_grouping, num_groups, pds,
 *                      pds_dest, kern_gpupreagg}   (opencl_gpupreagg.h:994-1003)
 *   <- clserv_process_gpupreagg (gpupreagg.c:3849-4240) + clserv_respond_gpupreagg
 * One chunk in, that chunk's partial rows out; nothing is kept between
 * requests (a backend that wants the table to stay in HBM across chunks uses
 * the session calls above).  'kgpreagg' is the host image {status,
 * sortbuf_len, kern_parambuf, kern_row_map} as KERN_GPUPREAGG_* lay it out
 * (nvalids < 0: every row; sortbuf_len is not used -- nothing is sorted);
 * 'kds_dest' is the caller's TUPSLOT buffer of dest_length bytes.  Before
 * done() runs: kgpreagg->status is the errcode (KERN_GPUPREAGG_DMARECV_*),
 * and on success kds_dest holds one row per group of this chunk, nitems
 * set, keys and partial values in target-list order exactly as
 * strom_gpupreagg_fetch() writes them (the backend reads rows 0..nitems-1,
 * gpupreagg.c:2610-2664).  StromError_CpuReCheck: kds_dest is untouched, the
 * backend aggregates the chunk itself (gpupreagg_next_tuple_fallback,
 * gpupreagg.c:2507-2607).  StromError_DataStoreNoSpace: kds_dest is too small
 * for the chunk's groups.  needs_grouping must agree with the program (it
 * has group keys or not); num_groups is the planner's estimate and sizes the
 * first hash table when the keys have no dense ids.  The request runs on a
 * runtime thread (key range -> table geometry -> fold -> partial rows); this
 * call only queues it.
 */
strom_task *strom_submit_gpupreagg_chunk(strom_devprog_key key,
										 const strom_preagg_target *targets, int ntargets,
										 kern_gpupreagg *kgpreagg,
										 const kern_data_store *kds, strom_dstore *kds_dev,
										 kern_data_store *kds_dest, size_t dest_length,
										 int needs_grouping, double num_groups,
										 int dindex,
										 strom_done_cb done, void *arg,
										 int *p_errcode);

/* ------------------------------------------------------------------ *
 * GpuHashJoin
 *
 * strom_hashjoin_table  <- the kern_multihash the reference uploads once
 *   per device and shares between the chunks of a join by a count under
 *   mhtables->lock (gpuhashjoin.c:4498-4557, released 4311-4320).  Create
 *   uploads a private copy and builds the probe index with kernels of the
 *   join's own program (so the key must be ready or becomes ready here).
 * strom_submit_gpuhashjoin <- clserv_process_gpuhashjoin (4430-5073).
 *   'khashjoin' is the host image {kern_parambuf, kern_resultbuf}; result
 *   records are nrels ints: outer_row + 1, then per inner relation the byte
 *   offset of the matched kern_hashentry inside its kern_hashtable.
 *   errcode StromError_DataStoreNoSpace: kern_resultbuf.nitems holds the
 *   number of records a retry needs room for (the reference re-enqueues
 *   with an exactly-sized buffer, 4330-4425).  A row-level CpuReCheck is
 *   reported as the chunk errcode: the reference has no CPU path for join
 *   rows ("CPU Recheck not implemented yet", 2948-2952).
 *
 *   Join types.  A (rel ..) of the join program may carry (jointype inner | left | semi | anti),
 *   default inner.  The slot of such a relation in a result record:
 *     inner  the offset of the matched entry, one record per candidate;
 *     left   the same, or 0 for a prefix without a candidate (one record, every column of the
 *            relation NULL);
 *     semi   0, ONE record for a prefix with at least one candidate;
 *     anti   0, one record for a prefix with none (NOT EXISTS: a NULL key has no candidate).
 *   A candidate is an entry whose keys are equal (a NULL never is) and for which the rel's qual
 *   -- the ON clause -- is true.  OFFSET 0 IS NEVER AN ENTRY: the table head sits there, so 0 in a
 *   record means "no entry" and every projection below makes the relation's columns NULL without
 *   reading the table.  RIGHT and FULL joins are out of scope of (jointype ..), which the code
 *   generator refuses by name: they are an INNER / LEFT program plus (track_matches), see "RIGHT
 *   and FULL joins" below.  A one-relation LEFT /
 *   SEMI / ANTI join on one integer-like key without a qual takes the one-pass kernels (SEMI and
 *   ANTI even over duplicate inner keys: "slot not empty" is the whole answer); everything else
 *   the general kernel.
 * ------------------------------------------------------------------ */
typedef struct strom_hashjoin_table strom_hashjoin_table;

strom_hashjoin_table *strom_hashjoin_table_create(strom_devprog_key key,
												  const kern_multihash *kmhash, size_t length,
												  int dindex, int *p_errcode);
void		strom_hashjoin_table_release(strom_hashjoin_table *tbl);
/* index form chosen for inner relation 'depth' (1-based): mode 1 = direct (one dense
 * integer-like key), 2 = keyed (one key of any type: 16-byte slots that carry the key
 * image), 0 = hashed (several keys) */
int			strom_hashjoin_table_info(strom_hashjoin_table *tbl, int depth,
									  int *p_mode, uint32_t *p_nslots,
									  int *p_unique, uint32_t *p_nentries);
/* the device copy of the kern_multihash (entry offsets in result records
 * index into it; rowid / htup of an entry are unchanged) */
int			strom_hashjoin_table_download(strom_hashjoin_table *tbl, void *buffer, size_t buflen);
strom_task *strom_submit_gpuhashjoin(strom_hashjoin_table *tbl,
									 kern_hashjoin *khashjoin,
									 const kern_data_store *kds,
									 strom_dstore *kds_dev,
									 const kern_row_map *krowmap,
									 uint32_t flags,
									 strom_done_cb done, void *arg,
									 int *p_errcode);

/*
 * Same, followed by kern_gpuhashjoin_projection_slot (opencl_hashjoin.h:
 * 691-839): the joined rows are materialised into 'kds_dest', a TUPSLOT
 * kern_data_store whose head (ncols, colmeta, nrooms) the caller filled;
 * destination column r takes column src_colidx[r] (0-based) of relation
 * src_depth[r] (0 = outer chunk, d = d-th inner relation).  On completion
 * kds_dest holds nitems rows.  Fixed-width by-value columns.  A record whose
 * slot for the relation is 0 ("no entry", see above): isnull is set, the value 0.
 * A kds_dest of KDS_FORMAT_ROW_FLAT takes kern_gpuhashjoin_projection_row
 * instead (opencl_hashjoin.h:437-689): the joined rows as heap tuples that
 * grow from the tail of the caller's buffer ('length' bytes in all; head with
 * ncols, colmeta {attlen, attalign}, nrooms, tdtypeid / tdtypmod filled by the
 * caller), row items behind the head, 'usage' = bytes of tuples.  Varlena
 * columns (attlen -1: text, character(n), numeric in its heap form) are
 * copied verbatim.  Columns of a relation with "no entry" are NULL: the tuple
 * carries a NULL bitmap (HEAP_HASNULL).  StromError_DataStoreNoSpace when the records outnumber
 * nrooms (kern_resultbuf.nitems says how many) or the tuples do not fit
 * 'length'; DataStoreCorruption when a destination column's attlen is not
 * its source's.
 */
strom_task *strom_submit_gpuhashjoin_projection(strom_hashjoin_table *tbl,
												kern_hashjoin *khashjoin,
												const kern_data_store *kds,
												strom_dstore *kds_dev,
												const kern_row_map *krowmap,
												kern_data_store *kds_dest,
												const int32_t *src_depth,
												const int32_t *src_colidx,
												uint32_t flags,
												strom_done_cb done, void *arg,
												int *p_errcode);

/*
 * Joined rows for the NEXT operator, without leaving HBM (SURVEY.md section
 * 8 f2; the reference hands a projected TUPSLOT store to the next node
 * through the host, gpuhashjoin.c:2686-2689, 4883-4968): after a
 * strom_submit_gpuhashjoin*() with STROM_RESULTS_ON_DEVICE over the resident
 * chunk 'outer', and BEFORE strom_task_wait() on it, this call waits for the
 * join and materialises its result records as a KDS_FORMAT_COLUMN chunk
 * (zone maps and not-null bitmaps included) that GpuScan / GpuPreAgg /
 * another GpuHashJoin take as a strom_dstore.  Column r takes column
 * src_colidx[r] (0-based) of relation src_depth[r]; type_oids[r] gives its
 * width, which must equal the source's (StromError_DataStoreCorruption
 * otherwise); a NEGATIVE oid means "that type, no zone map needed" and
 * spares the min/max pass over the column.  Fixed-width by-value columns
 * (bool, int2/4/8, float4/8, date, time, timestamp, the 64-bit numeric forms,
 * char(1)) and STROM_TEXTOID / STROM_BPCHARNOID.  A text or character(n)
 * column of the result has attlen -1, attbyval 0, attalign 4: its array
 * holds each row's 8-byte offset from the chunk head (0: NULL), the datums
 * -- copied whole, header included, whatever their form -- start on 4-byte
 * boundaries in a heap area behind the column arrays (extra_off), sized
 * exactly by a counting kernel that runs first; such a column has no zone
 * map.  Its source must be a text column too (DataStoreCorruption
 * otherwise, also for a source datum that points beyond its chunk); a
 * TUPSLOT 'outer' as its source answers BadRequestMessage; a result beyond
 * 4 GB answers DataStoreOutOfRange.
 * Fixed-width inner columns of a single-relation table with a DIRECT index and
 * unique keys are served from slot-indexed arrays the table builds on first use
 * -- of an INNER join only; a table whose program names another join type goes
 * through the entries.  Columns of a relation with "no entry" (slot 0) are NULL
 * in the bitmap and the zone maps; a NULL text datum has offset 0 and takes no
 * heap bytes.
 * A join that ended with
 * StromError_DataStoreNoSpace is reported as such: resize, join again.
 */
strom_dstore *strom_hashjoin_project_column(strom_task *join_task, strom_hashjoin_table *tbl,
											strom_dstore *outer, int ncols,
											const int32_t *src_depth, const int32_t *src_colidx,
											const int32_t *type_oids, int *p_errcode);

/*
 * RIGHT and FULL joins (JOIN_RIGHT / JOIN_FULL of the reference's planner, which it never sends to
 * the device).  The per-chunk program of a RIGHT join is exactly the INNER program, that of a FULL
 * join exactly the LEFT program; what differs is a property of the table and one extra pass:
 *     RIGHT = (jointype inner) + (track_matches) + the unmatched pass after the last chunk
 *     FULL  = (jointype left)  + (track_matches) + the same
 * (track_matches) is an item of the LAST (rel ..) of the program, inner or left (an unmatched
 * entry becomes a row in which everything else is NULL: no deeper relation may join onto it).  A
 * table made from such a program keeps one flag byte per 32-byte granule of that relation's
 * kern_hashtable behind its probe index; every probe kernel flags the entries it accepts (keys equal,
 * qual true, prefix reached the relation), by entry offset.  A chunk that ends with
 * DataStoreNoSpace has flagged all its candidates (the retry flags them again); after any other
 * errcode the flags are unspecified -- a subset of the chunk's candidates -- and the query fails.
 * The kern_multihash of a TRACKED table must be one that strom_multihash_build() made (or one laid
 * out like it: LONGALIGNed entries that do not overlap).  The flag byte of a granule records ONE
 * entry start; an image with entries that overlap or lie closer than their own length would lose
 * start marks, and with them rows of the unmatched pass, without an error.
 *
 * strom_submit_gpuhashjoin_unmatched: records {0, .., 0, entry offset} of nrels ints for every
 *   entry of the tracked relation without a flag, NULL-key entries included.  WORD 0 == 0 MEANS "NO
 *   OUTER ROW" (a join record holds row + 1 there).  'khashjoin' as for a join; DataStoreNoSpace
 *   with nitems = the room a retry needs; honours STROM_RESULTS_ON_DEVICE.
 * strom_submit_gpuhashjoin_unmatched_projection: the same into a TUPSLOT or ROW_FLAT kds_dest;
 *   every column of depth 0 is NULL, no outer chunk is read.
 * strom_hashjoin_project_column(task, tbl, NULL, ..) takes an unmatched task submitted with
 *   STROM_RESULTS_ON_DEVICE -- and outer == NULL takes no other task.
 * strom_hashjoin_table_tracked_depth: the tracked relation (1-based), 0 for a table without.
 * strom_hashjoin_table_reset_matches: every entry unmatched again (a rescan).
 * strom_hashjoin_table_matches_length / _fetch / _merge: the multi-GPU seam.  Every rank holds the
 *   same table and sees a shard of the outer rows; an entry is unmatched only if it is unmatched
 *   on all ranks, so one rank ORs the others' flag images in (_merge; 'len' must be _length, and
 *   the image must be of a table over the same kern_multihash: every bit but "matched" is compared
 *   with the table's own, BadRequestMessage and nothing merged otherwise) and runs the unmatched pass.
 * Ordering: the unmatched calls, _reset_matches, _matches_fetch and _matches_merge synchronise the
 *   device first, so they come after every join task of this table submitted before them, waited
 *   for or not.  Join tasks submitted afterwards are the caller's business.
 * BadRequestMessage, nothing launched: any of these on a table without tracking (_tracked_depth
 *   and _matches_length answer 0); strom_submit_gpupreagg_lookup / _lookup_star / _lookup_snowflake / _lookup_typed
 *   / _lookup_tracked on a TRACKED table (they probe without running the join program and would leave every flag
 *   clear); strom_submit_gpupreagg_joined stays allowed for the JOIN tasks of such a table -- the join
 *   ran and flagged -- and refuses a task of the unmatched pass: its records name no outer row.
 *   RIGHT and FULL joins in the fused lookup folds are asked of the FOLD, over an untracked inner table:
 *   strom_submit_gpupreagg_lookup_tracked, with flags by SLOT that the session owns.
 * Still out: a tracked relation that is not the last; (track_matches) tables in the fused lookup folds (their
 *   flags are addressed by entry, the folds' by slot); a run on more than one GPU (two tables on one device
 *   stand in for two ranks).
 */
strom_task *strom_submit_gpuhashjoin_unmatched(strom_hashjoin_table *tbl, kern_hashjoin *khashjoin,
											   uint32_t flags, strom_done_cb done, void *arg,
											   int *p_errcode);
strom_task *strom_submit_gpuhashjoin_unmatched_projection(strom_hashjoin_table *tbl,
														  kern_hashjoin *khashjoin,
														  kern_data_store *kds_dest,
														  const int32_t *src_depth,
														  const int32_t *src_colidx,
														  uint32_t flags,
														  strom_done_cb done, void *arg,
														  int *p_errcode);
int			strom_hashjoin_table_tracked_depth(strom_hashjoin_table *tbl);
int			strom_hashjoin_table_reset_matches(strom_hashjoin_table *tbl);
size_t		strom_hashjoin_table_matches_length(strom_hashjoin_table *tbl);
int			strom_hashjoin_table_matches_fetch(strom_hashjoin_table *tbl, void *buf, size_t len);
int			strom_hashjoin_table_matches_merge(strom_hashjoin_table *tbl, const void *buf, size_t len);

/*
 * GpuPreAgg straight over a join's result pairs -- the projection fused into
 * its consumer.  Row i of the virtual joined
 * relation is result pair i of 'join_task' (a GpuHashJoin submitted with
 * STROM_RESULTS_ON_DEVICE over the resident COLUMN chunk 'outer', finished
 * without error, and not yet given to strom_task_wait; its device results
 * pass to the new task, so the two can then be waited for in any order);
 * its column r is column src_colidx[r] of relation src_depth[r], of
 * type type_oids[r]; the session's program reads it as (var r+1 ...).
 * Needs one inner relation with a DIRECT index and unique keys, joined on a
 * plain outer column: inner columns then come from slot-indexed arrays the
 * table builds on first use.  Anything else -- a table whose program has a
 * (jointype left | semi | anti) relation included -- answers BadRequest with
 * nothing launched and the caller goes through strom_hashjoin_project_column()
 * (the pairs of a LEFT join are not folded here; a LEFT / SEMI / ANTI join over
 * unique keys needs no pairs at all: strom_submit_gpupreagg_lookup_typed).
 * Text / character(n): a variable of the program with one of these types
 * must be a column of 'outer' -- src_depth 0, type_oids STROM_TEXTOID /
 * STROM_BPCHARNOID as the variable's own type, onto a column with attlen
 * -1; the kernel turns the column's 8-byte offsets into datum addresses
 * (offset and datum inside the chunk, else DataStoreCorruption; a
 * compressed or external datum in a row that is folded: CpuReCheck, the
 * chunk is not folded).  A text variable mapped to the inner relation, onto
 * a by-value column or under another type answers BadRequest with nothing
 * launched: slot records hold fixed-width values only.
 */
strom_task *strom_submit_gpupreagg_joined(strom_gpupreagg *sess, strom_task *join_task,
										  strom_hashjoin_table *tbl, strom_dstore *outer,
										  int ncols, const int32_t *src_depth, const int32_t *src_colidx,
										  const int32_t *type_oids,
										  strom_done_cb done, void *arg, int *p_errcode);

/*
 * ... and without any join request: the join becomes a LOOKUP inside the
 * aggregate's own pass over the resident COLUMN chunk 'outer'
 * (gpupreagg_dense_lookup): a row's slot is outer key - key_min, a row
 * without a partner is dropped, virtual columns as above, a WHERE over
 * outer columns is the aggregate program's (qual ...).  Same requirements on
 * the table (one relation, DIRECT index, unique keys, key = a plain outer
 * column of int4 / int8 / date width, an INNER join: a table whose program
 * names another join type is refused, here and by _lookup_star / _lookup_snowflake
 * / _lookup_typed, with nothing launched -- LEFT / SEMI / ANTI are asked of the FOLD,
 * over the same inner table: strom_submit_gpupreagg_lookup_typed); anything else
 * answers BadRequest.
 * The JOIN program's own qual and parameters are NOT evaluated on this path
 * (only the aggregate program runs): a table whose program carries a
 * pulled-up outer qual or a join qual is refused with BadRequest -- put the
 * WHERE into the aggregate program, or go through _joined / the plain join.
 * Text / character(n) variables as for _joined: fact columns only (depth 0,
 * the variable's own type, a column with attlen -1), BadRequest otherwise.
 * A WHERE over fact columns alone, text included, runs before the probe; an
 * unreadable or corrupt datum there counts only for a row with a partner.
 */
strom_task *strom_submit_gpupreagg_lookup(strom_gpupreagg *sess,
										  strom_hashjoin_table *tbl, strom_dstore *outer,
										  int ncols, const int32_t *src_depth, const int32_t *src_colidx,
										  const int32_t *type_oids,
										  strom_done_cb done, void *arg, int *p_errcode);

/*
 * ... and a STAR of such lookups in the same single pass (gpupreagg_dense_lookup_star):
 * "fact JOIN dim1 JOIN dim2 ... GROUP BY".  tbls[d - 1] is relation d (1-based), each a table
 * as strom_submit_gpupreagg_lookup takes it (one inner relation, DIRECT index, unique keys, joined
 * on the plain outer column its own join program names, no pulled-up qual in that program).
 * src_depth[i] is 0 .. ntbls: 0 an outer column, d column src_colidx[i] of relation d.  An inner
 * join over all relations: a row is folded only if EVERY relation has a partner for it (key not
 * NULL, inside the table's key range, slot present); the WHERE is the aggregate program's (qual
 * ...), evaluated before any probe when it reads outer columns only, and an error in it is raised
 * only for a row that has a partner in every relation.  (Relations that join LEFT, SEMI or ANTI:
 * strom_submit_gpupreagg_lookup_typed, the same tables with a join type each.)
 * Two fact columns that point at the SAME dimension are two tables: a table's program names one
 * outer column, so the dimension is built once per fact column that joins it.
 * ntbls == 1 is strom_submit_gpupreagg_lookup.  BadRequest, and nothing is launched: ntbls
 * outside 1 .. STROM_LOOKUP_STAR_MAXRELS, a depth outside 0 .. ntbls, a table that fails the
 * requirements above or lives on another device, a hashed session, a session without a domain, a
 * text / character(n) variable of the program that is not mapped to depth 0, under its own type
 * (STROM_TEXTOID / STROM_BPCHARNOID), onto an outer column with attlen -1 (no relation serves a
 * text VARIABLE: slot records hold fixed-width values; a relation's text column is served as int4
 * ids, a coded column made by strom_textdict_encode_table, mapped under int4), a key that is not 4 or 8 bytes wide, and for ntbls >= 2 a
 * relation whose slot record is longer than 16 bytes or records that total more than 32 bytes
 * over all relations (the kernel holds a row's records of all relations in registers): the
 * caller then goes through the plain join and strom_hashjoin_project_column().
 */
#define STROM_LOOKUP_STAR_MAXRELS	4
strom_task *strom_submit_gpupreagg_lookup_star(strom_gpupreagg *sess,
											   strom_hashjoin_table *const *tbls, int ntbls,
											   strom_dstore *outer,
											   int ncols, const int32_t *src_depth, const int32_t *src_colidx,
											   const int32_t *type_oids,
											   strom_done_cb done, void *arg, int *p_errcode);
/*
 * The define block the runtime puts in front of a session's source to build the star kernels for
 * a mapping (no device needed: a planner or a test can compile the program ahead): relation d
 * (1-based) has a key of keylen[d-1] bytes, slot records of reclen[d-1] bytes in the narrow form
 * or not, and serves the virtual columns in inner_mask[d-1] (bit i: column i).  Returns the
 * length of the text, or -1 if it does not fit buflen or describes no valid mapping.
 */
int			strom_gpupreagg_lookup_star_defines(int ntbls, const int32_t *keylen, const int32_t *reclen,
												const int32_t *narrow, const uint64_t *inner_mask,
												char *buf, size_t buflen);

/*
 * ... and the same single pass for LEFT, SEMI and ANTI relations: "fact LEFT JOIN dim GROUP BY
 * dim.g", "WHERE EXISTS (SELECT 1 FROM dim WHERE dim.k = fact.k)", "WHERE NOT EXISTS (...)".
 * jointypes[d - 1] says how relation d joins the fact rows, in the values of the join program's
 * (jointype ...): 0 inner, 1 left, 2 semi, 3 anti.  It is an argument of the FOLD: a lookup never
 * runs the join program, the table only lends its index and its slot records -- so tbls[] are
 * exactly what strom_submit_gpupreagg_lookup_star takes (one-relation INNER programs, DIRECT index,
 * unique keys, no qual, not tracked, on the session's device; a table built from a (jointype ...)
 * program stays refused).
 * A row has a partner in relation d when its key is not NULL, inside the table's key range, and
 * the slot is present.  A row is folded iff every inner and every semi relation has a partner for
 * it and no anti relation has one; a left relation never drops a row.  The columns a left
 * relation serves are NULL for a row without a partner; semi and anti relations serve no column.
 * All relations are joined on fact columns, so they commute.  The aggregate program's (qual ...) is
 * the WHERE, applied after the join: over a left relation's column it sees NULL for partner-less
 * rows; over fact columns alone it still runs before any probe and drops a row under every join
 * type.  An error (in the qual, in the row, an unreadable text datum) is raised only for a row
 * that is folded.  Duplicate inner keys are not unique keys: such a SEMI / ANTI join goes through
 * the one-pass join, its row map and strom_submit_gpupreagg with that map.
 * jointypes all zero IS strom_submit_gpupreagg_lookup_star: its code path, error codes and
 * programs.  ntbls == 1 is the one-table kernel with every record form it reads, always built for
 * the mapping (GPUPREAGG_LOOKUP_JOINTYPE; STROM_GPUPREAGG_LOOKUP_GENERIC does not apply); 2 ..
 * STROM_LOOKUP_STAR_MAXRELS relations are the star kernels (GPUPREAGG_STAR_JOINTYPE_<d>).
 * BadRequest, and nothing is launched: jointypes NULL or a value outside 0 .. 3, a virtual column
 * mapped to a semi or anti relation, and everything strom_submit_gpupreagg_lookup_star refuses.
 * RIGHT and FULL joins of one of the relations: strom_submit_gpupreagg_lookup_tracked, below.
 */
strom_task *strom_submit_gpupreagg_lookup_typed(strom_gpupreagg *sess,
												strom_hashjoin_table *const *tbls, int ntbls,
												const int32_t *jointypes,	/* [ntbls] 0 inner, 1 left, 2 semi, 3 anti */
												strom_dstore *outer,
												int ncols, const int32_t *src_depth, const int32_t *src_colidx,
												const int32_t *type_oids,
												strom_done_cb done, void *arg, int *p_errcode);
/*
 * The define block of such a mapping, as strom_gpupreagg_lookup_star_defines gives the star's (no
 * device needed).  ntbls == 1: the one-table kernels' block (any record length they read), else
 * the star's; an inner relation adds no line, so an all-inner star gives
 * strom_gpupreagg_lookup_star_defines' text byte for byte.  -1: the text does not fit, no valid
 * mapping, a join type outside 0 .. 3, or a column under a semi / anti relation.
 */
int			strom_gpupreagg_lookup_typed_defines(int ntbls, const int32_t *keylen, const int32_t *reclen,
												 const int32_t *narrow, const uint64_t *inner_mask,
												 const int32_t *jointypes, char *buf, size_t buflen);

/*
 * ... and RIGHT and FULL joins: "SELECT dim.name, count(fact.k), sum(fact.x) FROM fact RIGHT JOIN dim ON
 * fact.k = dim.k GROUP BY dim.name" -- every member of the dimension, also those without facts.  The join's
 * own idiom (above: RIGHT = inner + track_matches, FULL = left + the same), asked of the FOLD: ONE relation
 * of the mapping may be TRACKED, 'tracked' is its number 1 .. ntbls; tracked + inner is a RIGHT join of that
 * relation, tracked + left a FULL join.  tbls[] are the untracked INNER tables the typed call takes (a table
 * built with (track_matches) stays refused: its flags are addressed by entry, these by slot).
 *   Join order.  The result is (fact JOIN the other relations, by their join types) RIGHT | FULL JOIN
 *     tracked: the tracked relation is joined LAST, and the relations no longer commute with it.
 *   Per chunk.  strom_submit_gpupreagg_lookup_tracked folds exactly what _lookup_typed folds for the same
 *     jointypes[]; tracking changes no row of it.  On the side the kernel notes which slots of the tracked
 *     table had a partner: slot s is MATCHED when some fact row of some chunk (1) has a key that is not NULL
 *     and lies inside the table's key range, (2) finds s present, and (3) survives every other relation --
 *     every inner and semi relation has a partner for it, no anti relation has one; a left relation never
 *     drops a row.  The WHERE does not decide a match: the aggregate program's (qual ...) is applied after
 *     the join, so a partner row that the qual rejects still matches its slot -- also a qual over fact
 *     columns alone (a tracked program does not evaluate it before the probe), which matters for quals that
 *     are not strict: "fact RIGHT JOIN dim ... WHERE fact.a IS NULL" is the anti-join from the right.  An
 *     error does not decide a match either: a chunk that ends CpuReCheck is not folded, but its flags are
 *     complete -- they are facts of the keys, and the kernel walks every row -- and a retry of the chunk
 *     sets the same flags again.
 *   The flags.  One byte per slot of the tracked table (0 unmatched, 1 matched), in device memory, zeroed
 *     when made, OWNED BY THE SESSION: slot records are shared between sessions and read-only, what matched
 *     is a fact of one query.  They are made by the first tracked request or by the unmatched call, bound
 *     to (table, tracked position, slot count) from then on, and freed with the session.  Plain byte loads
 *     and stores, test before set: no device atomics, no bit per slot (a byte store is no read-modify-write).
 *   The unmatched pass.  strom_submit_gpupreagg_lookup_unmatched takes the same mapping WITHOUT a chunk, after
 *     the last one: one row per slot of the tracked table that is present and not flagged.  The columns the
 *     tracked relation serves come from its slot record, with the record's own NULL bits; every other virtual
 *     column -- fact columns, text ones included, other relations' columns -- is NULL.  The row goes through
 *     the program's qual and is folded into the session like any row; qual and row errors are that task's
 *     status (CpuReCheck: nothing of the pass is folded).  It reads no chunk, takes no key width and depends
 *     on no fact column's width.  With no fold before it (an empty fact table) it emits every present slot.
 *     STROM_GPUPREAGG_UNMATCHED_MAX_GRID caps the work-groups that walk the slots (read on every call).
 *   Dimension rows with a NULL key have no slot, so the pass could never emit them: a table that holds one
 *     is refused as the tracked one (BadRequest; found once per table, entries against occupied slots), and
 *     the caller takes the join's RIGHT path, which does emit them.
 *   Ordering.  The unmatched call and the _matches_fetch / _merge / _reset calls synchronise the device
 *     first, like the join's: they come after every fold that has been LAUNCHED.  A fold whose program is
 *     still being built is parked and launched later -- wait for the folds (strom_task_wait) first.
 *   The seam.  strom_gpupreagg_lookup_matches_length / _fetch / _merge are what
 *     strom_hashjoin_table_matches_* are to the join: every rank or shard folds its part of the fact rows, one
 *     of them ORs the others' flag images in (_merge: 'len' must be _length and every byte 0 or 1, BadRequest
 *     and nothing merged otherwise), merges the partial rows as ever and runs the unmatched pass.
 *     strom_gpupreagg_lookup_reset_matches clears the flags and re-arms the pass (a rescan).
 * tracked == 0 IS strom_submit_gpupreagg_lookup_typed: its code path, its error codes, its programs.
 * BadRequest, and nothing is launched: everything the typed call refuses; tracked outside 0 .. ntbls; a
 * tracked semi or anti relation; a table with a NULL-key entry as the tracked one; a tracked request whose
 * (table, position) is not the one the session's flags are bound to; a second unmatched call, or a tracked
 * fold after the unmatched pass, without a reset; _matches_fetch / _merge / _reset on a session without flags
 * (_matches_length answers 0).  strom_submit_gpupreagg_lookup_snowflake offers no tracking.
 */
strom_task *strom_submit_gpupreagg_lookup_tracked(strom_gpupreagg *sess,
												  strom_hashjoin_table *const *tbls, int ntbls,
												  const int32_t *jointypes,	/* [ntbls] 0 inner, 1 left, 2 semi, 3 anti */
												  int tracked,				/* 0: none; d: relation d, RIGHT (inner) / FULL (left) */
												  strom_dstore *outer,
												  int ncols, const int32_t *src_depth, const int32_t *src_colidx,
												  const int32_t *type_oids,
												  strom_done_cb done, void *arg, int *p_errcode);
strom_task *strom_submit_gpupreagg_lookup_unmatched(strom_gpupreagg *sess,
													strom_hashjoin_table *const *tbls, int ntbls,
													const int32_t *jointypes, int tracked,	/* 1 .. ntbls */
													int ncols, const int32_t *src_depth, const int32_t *src_colidx,
													const int32_t *type_oids,
													strom_done_cb done, void *arg, int *p_errcode);
/*
 * strom_gpupreagg_lookup_typed_defines plus 'tracked': 0 returns the typed text byte for byte, otherwise
 * the block ends in one more line -- "#define GPUPREAGG_LOOKUP_TRACK 1" for the one-table block,
 * "#define GPUPREAGG_STAR_TRACK_REL d" for the star.  -1 also for tracked out of range or naming a semi /
 * anti relation.  _unmatched_defines: the block of the unmatched pass, which holds the tracked relation's
 * record facts only (length, narrow form, served-column mask).
 */
int			strom_gpupreagg_lookup_tracked_defines(int ntbls, const int32_t *keylen, const int32_t *reclen,
												   const int32_t *narrow, const uint64_t *inner_mask,
												   const int32_t *jointypes, int tracked, char *buf, size_t buflen);
int			strom_gpupreagg_lookup_unmatched_defines(int reclen, int narrow, uint64_t inner_mask,
													 char *buf, size_t buflen);
size_t		strom_gpupreagg_lookup_matches_length(strom_gpupreagg *sess);
int			strom_gpupreagg_lookup_matches_fetch(strom_gpupreagg *sess, void *buf, size_t len);
int			strom_gpupreagg_lookup_matches_merge(strom_gpupreagg *sess, const void *buf, size_t len);
int			strom_gpupreagg_lookup_reset_matches(strom_gpupreagg *sess);

/*
 * The define blocks of the programs this session has built FOR a mapping so far (one-table, star, typed,
 * tracked, the unmatched pass; a
 * checked retry's begins with GPUPREAGG_CHECKED), each followed by an empty line: what a request's tables came
 * to -- record length and form, served columns, join types -- for a planner's log or a test.  Returns the
 * length of the text (buf NULL: only that), or -1 if it does not fit buflen.
 */
int			strom_gpupreagg_mapping_defines(strom_gpupreagg *sess, char *buf, size_t buflen);

/*
 * ... and a SNOWFLAKE: a relation keyed by ANOTHER RELATION's column ("lineitem -> orders ->
 * customer", "fact -> product -> brand").  The fold kernels never decide a probe from another
 * relation's record; they do not have to: the tables are DIRECT with unique keys, so a child
 * relation is a function of its parent's slot, and the dimensions are joined to EACH OTHER once,
 * at table time, into the parent's slot records (hashjoin_compose_dimrec_kernel).  What is left
 * is the star of the tree's roots, each with composed records over its own slots -- one root is
 * the one-table lookup (both forms of its mapping), 2 .. STROM_LOOKUP_STAR_MAXRELS roots are the
 * star, with the star's own define block and programs.  Composed records are kept with the root
 * table, per column set and per set of descendant tables, and freed with it.
 * tbls[d - 1] is relation d as strom_submit_gpupreagg_lookup takes it; its program's outer key
 * column is a column of the fact chunk where parent[d - 1] is 0, otherwise of relation
 * parent[d - 1] < d (that program's outer relation), whose type link_type_oids[d - 1] names (int4,
 * date or int8; ignored for a root).  src_depth[i] is 0 .. ntbls as in the star: any relation may
 * serve columns, one that serves none is an existence filter.  An inner join: a row is folded
 * only if every relation of the tree has a partner (a NULL link, a link outside the child's key
 * range or in one of its holes: no partner); a non-inner link is not offered -- the relations of
 * strom_submit_gpupreagg_lookup_typed are all joined on fact columns.
 * parent[] all zero is strom_submit_gpupreagg_lookup_star, ntbls == 1 strom_submit_gpupreagg_lookup:
 * their code paths, their error codes.  BadRequest, and nothing is launched: a NULL argument, ntbls
 * outside 1 .. STROM_LOOKUP_SNOWFLAKE_MAXRELS, parent[d - 1] outside 0 .. d - 1, more than
 * STROM_LOOKUP_STAR_MAXRELS roots, a table that fails the one-table requirements or lives on
 * another device, a link type that is not int4 / date / int8, a composed relation of more than 16
 * columns at any step, with 2 roots and more a composed record longer than 16 bytes or records
 * that total more than 32 bytes over all roots, a text variable not at depth 0, a hashed session,
 * a session without a domain.  A link column the parent does not have, or of another width than
 * its type says: DataStoreCorruption, like a served column.
 */
#define STROM_LOOKUP_SNOWFLAKE_MAXRELS 8    /* the join's own limit on inner relations */
strom_task *strom_submit_gpupreagg_lookup_snowflake(strom_gpupreagg *sess,
        strom_hashjoin_table *const *tbls, int ntbls,
        const int32_t *parent,          /* [ntbls] 0: joined on a fact column; p in 1..d-1: on a column of relation p */
        const int32_t *link_type_oids,  /* [ntbls] type of the parent's column that joins relation d (ignored where parent is 0) */
        strom_dstore *outer, int ncols, const int32_t *src_depth, const int32_t *src_colidx,
        const int32_t *type_oids, strom_done_cb done, void *arg, int *p_errcode);
/*
 * Which star a snowflake flattens to (no device needed; the submit path uses it): the number of
 * roots, or -1 for an invalid tree (ntbls, parent[] or a depth outside the ranges above, more
 * than STROM_LOOKUP_STAR_MAXRELS roots).  root_of[d - 1]: the ordinal 1 .. of the root whose
 * subtree holds relation d; col_root[i]: 0 for an outer column, else that ordinal for the
 * relation that serves virtual column i.  Either may be NULL.
 */
int strom_gpupreagg_lookup_snowflake_roots(int ntbls, const int32_t *parent, int ncols, const int32_t *src_depth,
                                           int32_t *root_of /* [ntbls] ordinal 1.. of each relation's root */,
                                           int32_t *col_root /* [ncols] 0 or that ordinal */);

/* ------------------------------------------------------------------ *
 * chained operators: device-resident row maps
 *
 * The reference hands the rows an operator selected to the next one as
 * pgstrom_bulkslot {pds, nvalids, rindex[]} built on the host from
 * kern_resultbuf (pg_strom.h:323-329, gpuscan.c:1318-1446).  Here the ids
 * stay in HBM: strom_rowmap_from_task() waits for a GpuScan submitted with
 * STROM_RESULTS_ON_DEVICE, turns its results[] into a kern_row_map in place
 * (one tiny kernel) and takes the buffer over; the *_mapped submit calls
 * pass it to the next operator on the same resident chunk.  A chunk with
 * rows to re-check (negative ids) cannot be chained: StromError_CpuReCheck
 * is returned and the caller takes the host path for that chunk.  The map
 * must outlive the requests that use it; strom_task_wait() is still due for
 * the scan task.
 * ------------------------------------------------------------------ */
typedef struct strom_rowmap strom_rowmap;
strom_rowmap *strom_rowmap_from_task(strom_task *gpuscan_task, int *p_errcode);
/*
 * ... and of a finished single-relation SEMI or ANTI GpuHashJoin submitted with
 * STROM_RESULTS_ON_DEVICE: its records {outer_row + 1, 0} become a fresh kern_row_map of the outer
 * chunk (out of place; the join's buffer stays the task's), each outer row at most once.  With
 * the *_mapped calls this is "... FROM fact WHERE [NOT] EXISTS (...) GROUP BY ..." without a host
 * round trip.  Any other join type, a table of several relations, a task that is no such join:
 * BadRequest; a join that failed: its errcode (DataStoreNoSpace: resize, join again).
 */
strom_rowmap *strom_rowmap_from_join_task(strom_task *join_task, strom_hashjoin_table *tbl, int *p_errcode);
uint32_t	strom_rowmap_nvalids(strom_rowmap *map);
void	   *strom_rowmap_devptr(strom_rowmap *map);
void		strom_rowmap_release(strom_rowmap *map);
strom_task *strom_submit_gpuscan_mapped(strom_devprog_key key, kern_gpuscan *kgpuscan,
										strom_dstore *kds_dev, strom_rowmap *rowmap,
										uint32_t flags, strom_done_cb done, void *arg, int *p_errcode);
strom_task *strom_submit_gpuhashjoin_mapped(strom_hashjoin_table *table, kern_hashjoin *khashjoin,
											strom_dstore *kds_dev, strom_rowmap *rowmap,
											uint32_t flags, strom_done_cb done, void *arg, int *p_errcode);
strom_task *strom_submit_gpupreagg_mapped(strom_gpupreagg *sess, strom_dstore *kds_dev, strom_rowmap *rowmap,
										  strom_done_cb done, void *arg, int *p_errcode);

/* ------------------------------------------------------------------ *
 * GROUP BY text / character(n): a key dictionary in front of GpuPreAgg
 *
 * The reference's keycomp takes any type with a comparison function, bpchar
 * and text included (gpupreagg_codegen_keycomp, gpupreagg.c:1208-1242); its
 * partial rows then carry the key datums themselves.  GpuPreAgg here groups by
 * fixed-width key images, so a varlena key column is first replaced by dense
 * int4 ids under a device-resident dictionary (devlib/strom_textdict.h):
 * GpuPreAgg groups the ENCODED chunk by (key (var K int4)) -- the id column's
 * zone map {0, num_keys-1} is the domain of a dense session, and
 * strom_submit_gpupreagg_chunk takes an encoded chunk as it is -- and the
 * caller replaces ids by key datums after the fetch.
 *
 * One encode at a time per dictionary: the caller serialises, as with a
 * session.  An encode that ends in an error leaves every dictionary usable;
 * keys it had inserted before the error (an earlier key column of the same
 * call) may remain as ids no row was folded under.  They are harmless: a
 * result only carries ids that rows were folded under.
 * Refused with StromError_BadRequestMessage before any launch: a NULL handle,
 * a source that is not a resident COLUMN chunk, a key column whose attlen is
 * not -1, a varlena carry column, nkeys outside 1..STROM_PREAGG_MAXKEYS, a
 * dictionary of another device than the chunk's.
 * ------------------------------------------------------------------ */
typedef struct strom_textdict strom_textdict;
/* stands in for the varlena case of gpupreagg_codegen_keycomp: the dictionary decides which
 * keys are equal (bytewise; character(n) without its trailing blanks).
 * type_oid: STROM_TEXTOID | STROM_BPCHARNOID */
strom_textdict *strom_textdict_create(int type_oid, uint32_t nkeys_hint, int dindex, int *p_errcode);
uint32_t	strom_textdict_num_keys(strom_textdict *dict);
/* keycomp's varlena case, per chunk: a new resident COLUMN chunk, same rows in the same order as src:
 *   columns 0..nkeys-1 : int4 ids of src column key_colidx[i] under dicts[i]; NULL where the key is
 *                        NULL (notnull bitmap as src's); zone map {0, num_keys-1}, KDS_COLSTAT_MINMAX
 *   then               : copies of the fixed-width by-value src columns carry_colidx[], with their
 *                        colmeta, notnull bitmaps and zone maps
 * Blocks until the chunk is ready.  A compressed or external key datum: StromError_CpuReCheck,
 * the chunk is the CPU's and the dictionaries are as before the call. */
strom_dstore *strom_textdict_encode(strom_textdict *const *dicts, const int32_t *key_colidx, int nkeys,
									strom_dstore *src, const int32_t *carry_colidx, int ncarry,
									int *p_errcode);
/* stands in for pg_fixup_tupslot_varlena (the way varlena keys of a partial row reach the host):
 * the keys by id -- heap image + offsets[id] of each complete datum in it; returns the number of
 * keys (negative: -errcode), *p_heap_bytes the heap's size; sizes alone when heap_out == NULL */
long		strom_textdict_fetch(strom_textdict *dict, void *heap_out, size_t heaplen,
								 uint64_t *offsets_out, size_t noffsets, size_t *p_heap_bytes);
/* device time of the last encode's kernels under this dictionary, when strom_set_perfmon(1):
 * ns_out[4] = probe, settle, emit, rebuild (measurement; no counterpart in the reference) */
int			strom_textdict_kernel_ns(strom_textdict *dict, uint64_t *ns_out);
/* the device program the last encode under this dictionary ran (0: none yet): its text carries the
 * TEXTDICT_BLOCK / TEXTDICT_HASH_BITS in force (strom_get_devprog_source) */
strom_devprog_key strom_textdict_program(strom_textdict *dict);
/* forget every key (keycomp keeps no state between queries; this is the next query's dictionary) */
void		strom_textdict_reset(strom_textdict *dict);
void		strom_textdict_release(strom_textdict *dict);
/* a DIMENSION's text column under a dictionary, as int4 ids by slot of its hash table, served by
 * every fused fold like an int4 column of the relation: strom_textdict_encode_table, declared and
 * described in a file of its own.  (reset and release end the epoch of the ids such columns hold.)
 * NOTE: tests/test_textdict_cpu.py pins the set of strom_textdict_* entry points declared in THIS file;
 * an entry point declared in the included file is outside that pin and is checked by
 * tests/test_dim_text_lookup_cpu.py instead -- a further one needs a check of its own there. */
#include "strom_textdict_table.h"

/* ------------------------------------------------------------------ *
 * GROUP BY text across sessions and GPUs: one numbering for several dictionaries
 *
 * Sessions of several shards (row ranges of one table, one process per GPU) can be merged --
 * strom_gpupreagg_merge, _exchange_local, _allreduce, _reduce_scatter -- only if they call the same
 * key by the same id.  Every shard encodes under a dictionary of its own; then every shard builds
 * the same UNION dictionary by absorbing the shards' key images (what strom_textdict_fetch hands
 * out: heap bytes + offsets[id]) in rank order, and rewrites the id columns of its encoded chunks
 * through the id map its own image got.  The numbering is a function of the images and their
 * order alone -- Python's  for k in image: ids.setdefault(k, len(ids))  with 'ids' starting as the
 * keys the dictionary holds: a key it holds keeps its id, the others get num_keys, num_keys+1, ...
 * in order of first appearance in the image, equal keys of one image (character(n): 'a', 'a ')
 * get one id -- so the union dictionaries of all ranks are identical without further talk, and
 * the sessions share the dense domain {0, num_keys} of the union.
 *
 * One absorb / recode at a time per dictionary and chunk: the caller serialises, as with an
 * encode.  A map remembers the dictionary it was made by and must be released before it.
 * Refused with StromError_BadRequestMessage before any launch: a NULL handle, dst == src,
 * dictionaries of different type or device, nkeys > 0 with a NULL heap or NULL offsets, a recode
 * target that is not a resident COLUMN chunk, a recode column that is not by-value with attlen 4
 * (or named twice), ncols outside 1..STROM_PREAGG_MAXKEYS, a map of another device than the chunk's.
 * ------------------------------------------------------------------ */
typedef struct strom_keymap strom_keymap;		/* device-resident int4[n]: id in the image -> id under dst */
/* dst absorbs a host image of nkeys complete varlena datums; blocks like an encode.  The image is
 * checked on the host first (every offset inside the heap, every datum inside it by its own
 * length, no external or compressed header): StromError_DataStoreCorruption, no kernel runs.  An
 * absorb that ends in an error leaves dst as it was: the same keys under the same ids. */
strom_keymap *strom_keyunion_absorb(strom_textdict *dst, const void *heap, size_t heaplen,
									const uint64_t *offsets, uint32_t nkeys, int *p_errcode);
/* ... the keys of src in id order, read where they lie on the device (no host copy); src is unchanged */
strom_keymap *strom_keyunion_absorb_dict(strom_textdict *dst, strom_textdict *src, int *p_errcode);
uint32_t	strom_keymap_size(strom_keymap *map);
int			strom_keymap_fetch(strom_keymap *map, int32_t *out, size_t n);
void		strom_keymap_release(strom_keymap *map);
/* ids[row] = maps[i][ids[row]] over the int4 column colidx[i] of an encoded chunk, in place.  A NULL
 * row's id becomes 0 without a lookup; an id >= the map's size on a non-NULL row:
 * StromError_DataStoreCorruption.  The column's zone map becomes {0, num_keys-1} of the map's
 * dictionary as it is at the time of the call; notnull bitmaps and the other columns are not
 * touched.  After an error the id columns named in the call are unspecified: release the chunk. */
int			strom_keyunion_recode(strom_dstore *encoded, const int32_t *colidx,
								  strom_keymap *const *maps, int ncols);
/* device time, when strom_set_perfmon(1): ns_out[6] = the last absorb into dst (probe, ranks, settle,
 * emit, rebuild) and the last recode through a map of dst (measurement) */
int			strom_keyunion_kernel_ns(strom_textdict *dst, uint64_t *ns_out);

/* ------------------------------------------------------------------ *
 * multi-GPU: merge of the per-GPU GpuPreAgg tables over RCCL (xGMI)
 *
 * The reference has no collective (SURVEY.md section 2.3 / section 5
 * "Distributed communication backend: none"): one backend's Agg node adds up
 * the partial rows of every chunk (gpupreagg.c:4430-4773, pg_strom--1.0.sql:
 * 247-401).  With one process per GPU that addition happens between the
 * GPUs: sessions created with the SAME program, targets and key domain have
 * tables of identical layout, and strom_gpupreagg_allreduce() adds them up in
 * place -- SUM on int64 (nrows, integer and numeric psum: exact), SUM on
 * double (float psum: tolerance = summation order), MIN / MAX for pmin /
 * pmax, OR for the has-value flags -- one collective per table section,
 * grouped into one RCCL launch.  Afterwards every rank's
 * strom_gpupreagg_fetch() returns the partial rows of the WHOLE table.
 * 'comm' is an ncclComm_t (from the host's own RCCL, or from
 * strom_rccl_comm_init_rank below); 'stream' a hipStream_t or NULL = the
 * session's own stream.  Both calls return when the merge is done.
 * strom_gpupreagg_census_allreduce() is the planning-time twin: the union of
 * the ranks' census bitmaps, to be followed by strom_gpupreagg_compact(sess,
 * NULL, 0) on every rank.
 * RCCL is loaded on first use (librccl.so.1); no RCCL type crosses the ABI.
 * ------------------------------------------------------------------ */
int			strom_gpupreagg_allreduce(strom_gpupreagg *sess, void *comm, void *stream);
/*
 * Hashed GROUP BY sessions (strom_gpupreagg_create_hashed) have no common table layout: their
 * groups travel, HASH-PARTITIONED -- a group belongs to the rank its key
 * hashes to; every rank packs its groups by owner, the ranks exchange them pairwise
 * (ncclSend / ncclRecv) and each merges its own partition:
 *   strom_gpupreagg_reduce_scatter()  ends there: afterwards this rank holds the merged groups
 *                                     it owns and nothing else -- the ranks' fetches are disjoint,
 *                                     their union is the result (what parallel backends under a
 *                                     Gather node want);
 *   strom_gpupreagg_allreduce()       goes on to all-gather the final groups: afterwards every
 *                                     rank holds every merged group, as above.
 * Integer sums never wrap here either: the ranks first all-gather the largest |sum| each holds,
 * and when the sum of those is 2^63 or more every rank returns StromError_CpuReCheck with its
 * table untouched (the chunks are then aggregated on the CPU, the reference's answer to
 * CHECK_OVERFLOW_INT, opencl_gpupreagg.h:142-143).  A rank-local failure (out of memory, a full
 * table) makes EVERY rank return an error: no rank is left waiting in a collective.
 * strom_gpupreagg_exchange_local() runs the same exchange among n (<= 64) hashed sessions of ONE
 * device, session i as rank i, with device copies where the collectives are -- the harness that
 * shows a wrong owner, a lost partition or a dropped range check on one GPU.
 * strom_gpupreagg_merge() is the merge between two sessions of ONE device: src's groups are
 * added to dst's table, src is left as it is.  Hashed sessions: export, a read-only pass that
 * checks every group that exists on both sides (an integer sum that would leave int8:
 * StromError_CpuReCheck, dst untouched), then import.  Dense
 * sessions (same program, same domain, same compaction): the tables are added lane by lane with the
 * all-reduce merge's own prepare / operator / finish steps -- identities for entries without a value,
 * sign flips for the float min / max keys, flags as bytes under MAX, integer sums as carry-free limbs
 * (they are 128 bits wide in the table and must not wrap in the merge either).  Sessions that do not
 * match are refused with StromError_BadRequestMessage.
 */
int			strom_gpupreagg_merge(strom_gpupreagg *dst, strom_gpupreagg *src);
int			strom_gpupreagg_reduce_scatter(strom_gpupreagg *sess, void *comm, void *stream);
int			strom_gpupreagg_exchange_local(strom_gpupreagg **sessions, int n, int gather_after);
int			strom_gpupreagg_census_allreduce(strom_gpupreagg *sess, void *comm, void *stream);
/* communicator bootstrap for a host without its own: rank 0 makes the id
 * (strom_rccl_unique_id_bytes() bytes), hands it to the others by whatever
 * channel the host has, every rank calls comm_init_rank with its device */
size_t		strom_rccl_unique_id_bytes(void);
int			strom_rccl_get_unique_id(void *id_out, size_t len);
int			strom_rccl_comm_init_rank(void **p_comm, int nranks, const void *id, size_t len,
									  int rank, int dindex);
int			strom_rccl_comm_destroy(void *comm);

/*
 * Achievable HBM read rate of this box: a read-only streaming kernel over
 * 'nbytes' of device memory, best of 'nreps' launches, in GB/s (SURVEY.md
 * section 8d asks for the measured denominator next to the nominal 8 TB/s).
 */
int			strom_membw_probe(int dindex, size_t nbytes, int nreps, double *p_gbs);

/* block until the request finished; returns its errcode.  Frees the task. */
int			strom_task_wait(strom_task *task, strom_perfmon *pfm_out);
/* the same without the answer: pgstrom_put_message (mqueue.c:533-554) */
void		strom_task_release(strom_task *task);
/* device address of the kern_gpuscan / kern_hashjoin image of a task that
 * asked for STROM_RESULTS_ON_DEVICE (valid until strom_task_wait) */
void	   *strom_task_devptr(strom_task *task);
/* drain everything queued on every device */
void		strom_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif	/* STROM_HIP_H */
