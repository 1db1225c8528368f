/*
 * textdict.cpp -- text / character(n) group keys as dense int4 ids (devlib/strom_textdict.h)
 *
 * The reference's keycomp compares varlena keys through their type's comparison function
 * (gpupreagg_codegen_keycomp, gpupreagg.c:1208-1242).  Here the keys of a resident COLUMN chunk
 * are replaced by their ids in a device-resident dictionary BEFORE GpuPreAgg sees the chunk; the
 * encoded chunk groups by (key (var K int4)) on the dense path, its zone map {0, num_keys-1}
 * being the domain.  The ids are turned back into datums after the fetch (strom_textdict_fetch).
 *
 * One encode, per key column:
 *   probe -> read {status, nnew, nnull, heap_need} (the one small copy) ->
 *     NoSpace (no place found, or the claims took the table past half full), heap or entries short:
 *                                      grow, rebuild, probe again (the probe is idempotent for
 *                                      the keys that have entries; claims are dropped by the rebuild)
 *     another error:                   rebuild at the same size, return it: the dictionary is as before
 *     else:                            settle, emit, rebuild larger if the load passed 1/2
 */
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "runtime.h"

using namespace strom;

struct strom_textdict {
	int			type_oid = 0;
	int			dindex = 0;
	bool		blank_padded = false;
	cl_uint		nkeys = 0;
	cl_uint		nslots = 0;
	cl_uint		entries_cap = 0;
	size_t		heap_size = 0, heap_usage = 0;
	cl_ulong   *slots = nullptr;
	textdict_entry *entries = nullptr;
	char	   *heap = nullptr;
	textdict_ctl *ctl = nullptr;
	cl_uint		nkeys_hint = 0;
	/* device time of the last encode's kernels, when the perfmon is on: probe, settle, emit, rebuild */
	uint64_t	kern_ns[4] = {0, 0, 0, 0};
	/* ... of the last absorb's (probe, ranks, settle, emit, rebuild) and of the last recode through one of
	 * this dictionary's maps */
	uint64_t	union_ns[6] = {0, 0, 0, 0, 0, 0};
	/* the program the last encode ran: TEXTDICT_BLOCK / TEXTDICT_HASH_BITS are part of its text */
	strom_devprog_key program = 0;
	/* who this dictionary is to the tables that hold coded columns under it (textdict_encode_table_slots):
	 * a number no other dictionary of the process gets, and the count of its resets.  Ids are only
	 * good under the (serial, epoch) they were made under. */
	uint64_t	serial = 0;
	uint64_t	epoch = 1;
};

namespace {

/* serial -> epoch of every living dictionary: what a table asks by NUMBER, so that a coded column
 * whose dictionary was reset or released is found stale without touching the handle */
std::mutex &
epoch_lock(void)
{
	static std::mutex &m = *new std::mutex();
	return m;
}

std::map<uint64_t, uint64_t> &
epoch_registry(void)
{
	static std::map<uint64_t, uint64_t> &r = *new std::map<uint64_t, uint64_t>();
	return r;
}

enum { K_PROBE = 0, K_SETTLE, K_EMIT, K_REBUILD,
	   K_TOFFSETS, K_TPROBE, K_TSETTLE, K_TEMIT,
	   K_UPROBE, K_UCOUNT, K_UOFFSETS, K_USETTLE, K_UEMIT, K_RECODE, K_NFUNCS };
enum { U_PROBE = 0, U_RANKS, U_SETTLE, U_EMIT, U_REBUILD, U_RECODE };
const char *const kernel_names[K_NFUNCS] = {
	"textdict_probe", "textdict_settle", "textdict_emit", "textdict_rebuild",
	"textdict_table_offsets", "textdict_table_probe", "textdict_table_settle", "textdict_table_emit",
	"keyunion_probe", "keyunion_count", "keyunion_offsets", "keyunion_settle", "keyunion_emit", "keyunion_recode" };

/* the fixed program; the two knobs are part of its text (as build() pre-builds it) */
std::string
textdict_source(void)
{
	std::string s;
	for (const char *name : {"TEXTDICT_BLOCK", "TEXTDICT_HASH_BITS"})
	{
		const char *v = getenv((std::string("STROM_") + name).c_str());
		if (v && *v)
			s += std::string("#define ") + name + " " + std::to_string(atoi(v)) + "\n";
	}
	return s + "#include \"strom_kds.h\"\n#include \"strom_common.h\"\n#include \"strom_textlib.h\"\n"
		"#include \"strom_textdict.h\"\n";
}

unsigned
textdict_block(void)
{
	const char *v = getenv("STROM_TEXTDICT_BLOCK");
	int		b = (v && *v) ? atoi(v) : 256;
	return (b >= 64 && b <= 1024 && b % 64 == 0) ? (unsigned)b : 0;	/* 0: the program does not build either */
}

Program *
textdict_program(int *p_errcode, strom_devprog_key *p_key)
{
	/* one reference per variant is kept for the life of the process */
	static std::mutex &lock = *new std::mutex();
	static std::map<std::string, strom_devprog_key> &keys = *new std::map<std::string, strom_devprog_key>();
	std::string src = textdict_source();
	strom_devprog_key key;
	{
		std::lock_guard<std::mutex> g(lock);
		auto it = keys.find(src);
		if (it == keys.end())
			it = keys.emplace(src, strom_get_devprog_key(src.c_str(), 0)).first;
		key = it->second;
	}
	*p_key = key;
	if (textdict_block() == 0 || strom_lookup_device_program(key, 1) != STROM_DEVPROG_READY)
	{
		*p_errcode = StromError_ProgramBuildFailure;
		return nullptr;
	}
	return lookup_program(key);
}

cl_uint
pow2_at_least(size_t n)
{
	size_t	p = 16;
	while (p < n && p < ((size_t)1 << 31))
		p <<= 1;
	return (cl_uint)p;
}

struct Encoder {
	Device	   *dev;
	hipStream_t	stream;
	hipFunction_t fn[K_NFUNCS];
	unsigned	block;
	unsigned	max_grid;
	bool		timed;
	uint64_t   *rebuild_ns;		/* where a rebuild's device time goes: the encode's or the absorb's account */

	/* the fixed program's kernels first..last for this device, and the launch geometry */
	int open(Device *device, int first, int last, strom_devprog_key *p_progkey);

	unsigned grid_for(size_t n) const
	{
		return (unsigned)std::max<size_t>(1, std::min<size_t>((n + block - 1) / block, max_grid));
	}

	int launch(uint64_t *acc, int which, unsigned grid, void **args)
	{
		hipEvent_t	ev0 = nullptr, ev1 = nullptr;
		if (timed && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess))
			return StromError_HipInternal;
		if (timed)
			(void)hipEventRecord(ev0, stream);
		hipError_t	rc = hipModuleLaunchKernel(fn[which], grid, 1, 1, block, 1, 1, 0, stream, args, nullptr);
		if (timed)
		{
			float	ms = 0;
			(void)hipEventRecord(ev1, stream);
			if (rc == hipSuccess && hipEventSynchronize(ev1) == hipSuccess &&
				hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess)
				*acc += (uint64_t)((double)ms * 1e6);
			(void)hipEventDestroy(ev0);
			(void)hipEventDestroy(ev1);
		}
		return rc == hipSuccess ? 0 : hip_errcode(rc, "textdict kernel");
	}

	textdict_args base_args(strom_textdict *dict) const
	{
		textdict_args a;
		memset(&a, 0, sizeof(a));
		a.slots = (cl_ulong)(uintptr_t)dict->slots;
		a.entries = (cl_ulong)(uintptr_t)dict->entries;
		a.heap = (cl_ulong)(uintptr_t)dict->heap;
		a.ctl = (cl_ulong)(uintptr_t)dict->ctl;
		a.heap_usage = dict->heap_usage;
		a.heap_size = dict->heap_size;
		a.nslots = dict->nslots;
		a.nkeys = dict->nkeys;
		a.blank_padded = dict->blank_padded ? 1 : 0;
		return a;
	}

	int read_ctl(strom_textdict *dict, textdict_ctl *out)
	{
		if (hipMemcpyAsync(out, dict->ctl, sizeof(*out), hipMemcpyDeviceToHost, stream) != hipSuccess ||
			hipStreamSynchronize(stream) != hipSuccess)
			return StromError_HipInternal;
		return 0;
	}

	/* entries -> a cleared slot array of 'nslots' words (the dictionary's own when the size stays) */
	int rebuild(strom_textdict *dict, cl_uint nslots)
	{
		if (nslots != dict->nslots || !dict->slots)
		{
			cl_ulong   *fresh = (cl_ulong *)dev->pool.alloc(sizeof(cl_ulong) * (size_t)nslots);
			if (!fresh)
				return StromError_OutOfMemory;
			/* the old array may still be read by a queued kernel: the stream is in order, and the
			 * pool hands memory out again only to work queued later or synchronised with */
			if (hipStreamSynchronize(stream) != hipSuccess)
			{
				dev->pool.release(fresh);
				return StromError_HipInternal;
			}
			if (dict->slots)
				dev->pool.release(dict->slots);
			dict->slots = fresh;
			dict->nslots = nslots;
		}
		if (hipMemsetAsync(dict->slots, 0, sizeof(cl_ulong) * (size_t)dict->nslots, stream) != hipSuccess ||
			hipMemsetAsync(dict->ctl, 0, sizeof(textdict_ctl), stream) != hipSuccess)
			return StromError_HipInternal;
		if (dict->nkeys == 0)
			return 0;
		textdict_args a = base_args(dict);
		void	   *args[] = { &a };
		int			rc = launch(rebuild_ns, K_REBUILD, grid_for(dict->nkeys), args);
		textdict_ctl ctl;
		if (rc == 0)
			rc = read_ctl(dict, &ctl);
		if (rc == 0 && ctl.status != 0)
			rc = ctl.status;
		return rc;
	}

	/* room for 'need' bytes / entries, what is there copied over */
	template <typename T>
	int grow(T **p_buf, size_t used, size_t need)
	{
		T	   *fresh = (T *)dev->pool.alloc(sizeof(T) * need);
		if (!fresh)
			return StromError_OutOfMemory;
		if ((used > 0 && hipMemcpyAsync(fresh, *p_buf, sizeof(T) * used, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
			hipStreamSynchronize(stream) != hipSuccess)
		{
			dev->pool.release(fresh);
			return StromError_HipInternal;
		}
		if (*p_buf)
			dev->pool.release(*p_buf);
		*p_buf = fresh;
		return 0;
	}

	/* one key column of a chunk: ids into out_values / out_notnull; *p_nnull = its NULL rows */
	int encode_column(strom_textdict *dict, strom_dstore *src, cl_uint colidx, cl_uint *row_slot,
					  textdict_newkey *newkeys, void *out_values, void *out_notnull, cl_uint *p_nnull)
	{
		const void *a_src = src->devptr;
		return encode_rows(dict, K_PROBE, &a_src, src->head.nitems, colidx, row_slot, newkeys,
						   out_values, out_notnull, p_nnull);
	}

	/*
	 * the host policy of an encode, for both sources of rows: the kernels 'first' (probe), first + 1
	 * (settle), first + 2 (emit) take (*src_arg, textdict_args) -- a chunk and its rows, or a
	 * textdict_table_args and the table's slots
	 */
	int encode_rows(strom_textdict *dict, int first, void *src_arg, cl_uint nrows, cl_uint colidx, cl_uint *row_slot,
					textdict_newkey *newkeys, void *out_values, void *out_notnull, cl_uint *p_nnull)
	{
		void	   *a_src_p = src_arg;
		textdict_ctl ctl;
		int			rc;

		for (int turn = 0; ; turn++)
		{
			textdict_args a = base_args(dict);
			a.row_slot = (cl_ulong)(uintptr_t)row_slot;
			a.newkeys = (cl_ulong)(uintptr_t)newkeys;
			a.colidx = colidx;
			void	   *args[] = { a_src_p, &a };

			if (hipMemsetAsync(dict->ctl, 0, sizeof(textdict_ctl), stream) != hipSuccess)
				return StromError_HipInternal;
			if ((rc = launch(&dict->kern_ns[K_PROBE], first, grid_for(nrows), args)) != 0 || (rc = read_ctl(dict, &ctl)) != 0)
				return rc;
			size_t	keys_after = (size_t)dict->nkeys + ctl.nnew;
			/* no place found, or the claims took the table past half full; a row error goes first */
			bool	nospace = (ctl.status == StromError_DataStoreNoSpace || (ctl.status == 0 && ctl.toofull != 0));
			bool	heap_short = (dict->heap_usage + ctl.heap_need > dict->heap_size);
			bool	entries_short = (keys_after > dict->entries_cap);

			if (ctl.status != 0 && !nospace)
			{
				/* the claims of this call leave the table; the entries were never touched */
				rc = rebuild(dict, dict->nslots);
				return rc != 0 ? rc : ctl.status;
			}
			if (!nospace && !heap_short && !entries_short)
				break;
			if (turn >= 40 || keys_after >= ((size_t)1 << 29))
			{
				(void)rebuild(dict, dict->nslots);
				return StromError_DataStoreNoSpace;
			}
			if (heap_short)
			{
				size_t	need = std::max(dict->heap_usage + (size_t)ctl.heap_need, 2 * dict->heap_size);
				if ((rc = grow(&dict->heap, dict->heap_usage, need)) != 0)
					return rc;
				dict->heap_size = need;
			}
			if (entries_short)
			{
				size_t	need = std::max(keys_after, 2 * (size_t)dict->entries_cap);
				if ((rc = grow(&dict->entries, dict->nkeys, need)) != 0)
					return rc;
				dict->entries_cap = (cl_uint)need;
			}
			/* a table that ran full has told of the keys it could hold only: eight times the slots
			 * then, so that a dictionary begun without a hint reaches any size in a few turns */
			cl_uint	nslots = pow2_at_least(4 * keys_after);
			if (nospace)
				nslots = std::max(nslots, pow2_at_least(8 * (size_t)dict->nslots));
			nslots = std::max(nslots, dict->nslots);
			if ((rc = rebuild(dict, nslots)) != 0)
				return rc;
		}
		/* the counters move only when settle and emit have been seen to end clean: until then the
		 * dictionary is what the entries below 'nkeys' say */
		cl_uint		nnew = ctl.nnew, nnull = ctl.nnull;
		cl_ulong	heap_need = ctl.heap_need;
		rc = 0;
		if (nnew > 0)
		{
			textdict_args a = base_args(dict);
			a.newkeys = (cl_ulong)(uintptr_t)newkeys;
			a.colidx = colidx;
			a.nnew = nnew;
			void	   *args[] = { a_src_p, &a };
			rc = launch(&dict->kern_ns[K_SETTLE], first + 1, grid_for(nnew), args);
		}
		if (rc == 0)
		{
			textdict_args a = base_args(dict);
			a.nkeys = dict->nkeys + nnew;
			a.row_slot = (cl_ulong)(uintptr_t)row_slot;
			a.out_values = (cl_ulong)(uintptr_t)out_values;
			a.out_notnull = (cl_ulong)(uintptr_t)out_notnull;
			void	   *args[] = { a_src_p, &a };
			if ((rc = launch(&dict->kern_ns[K_EMIT], first + 2, grid_for(nrows), args)) == 0 && (rc = read_ctl(dict, &ctl)) == 0)
				rc = ctl.status;				/* settle or emit met a word no launch writes */
		}
		if (rc != 0)
		{
			/* back to the keys before the call: their entries and heap bytes were not touched */
			(void)hipStreamSynchronize(stream);
			(void)rebuild(dict, dict->nslots);
			return rc;
		}
		dict->nkeys += nnew;
		dict->heap_usage += heap_need;
		*p_nnull = nnull;
		if (2 * (size_t)dict->nkeys > dict->nslots)
			return rebuild(dict, pow2_at_least(4 * (size_t)dict->nkeys));
		return 0;
	}
};

int
Encoder::open(Device *device, int first, int last, strom_devprog_key *p_progkey)
{
	int		errcode = 0;
	Program *prog = textdict_program(&errcode, p_progkey);

	dev = device;
	stream = device->streams[0];
	timed = perfmon_enabled();
	rebuild_ns = nullptr;
	for (int i = first; prog && i <= last; i++)
		if (!(fn[i] = prog->get_function(device, kernel_names[i], &errcode)))
			prog = nullptr;
	if (!prog)
		return errcode ? errcode : StromError_ProgramBuildFailure;
	block = textdict_block();
	max_grid = (unsigned)device->prop.multiProcessorCount * 8;
	if (const char *v = getenv("STROM_TEXTDICT_MAX_GRID"))		/* tests: grid strides on small chunks */
		if (atoi(v) > 0)
			max_grid = (unsigned)atoi(v);
	return 0;
}

void
textdict_free(Device *dev, strom_textdict *dict)
{
	for (void *p : { (void *)dict->slots, (void *)dict->entries, (void *)dict->heap, (void *)dict->ctl })
		if (p)
			dev->pool.release(p);
	dict->slots = nullptr;
	dict->entries = nullptr;
	dict->heap = nullptr;
	dict->ctl = nullptr;
}

/* empty tables sized by the hint */
int
textdict_allocate(Device *dev, strom_textdict *dict)
{
	dict->nkeys = 0;
	dict->heap_usage = 0;
	dict->nslots = pow2_at_least(4 * (size_t)dict->nkeys_hint);
	dict->entries_cap = std::max<cl_uint>(dict->nkeys_hint, 4);
	dict->heap_size = 16 * (size_t)dict->entries_cap;
	dict->slots = (cl_ulong *)dev->pool.alloc(sizeof(cl_ulong) * (size_t)dict->nslots);
	dict->entries = (textdict_entry *)dev->pool.alloc(sizeof(textdict_entry) * (size_t)dict->entries_cap);
	dict->heap = (char *)dev->pool.alloc(dict->heap_size);
	dict->ctl = (textdict_ctl *)dev->pool.alloc(sizeof(textdict_ctl));
	if (!dict->slots || !dict->entries || !dict->heap || !dict->ctl)
		return StromError_OutOfMemory;
	(void)hipSetDevice(dev->hip_id);
	if (hipMemsetAsync(dict->slots, 0, sizeof(cl_ulong) * (size_t)dict->nslots, dev->streams[0]) != hipSuccess ||
		hipMemsetAsync(dict->ctl, 0, sizeof(textdict_ctl), dev->streams[0]) != hipSuccess ||
		hipStreamSynchronize(dev->streams[0]) != hipSuccess)
		return StromError_HipInternal;
	return 0;
}

}	/* namespace */

extern "C" strom_textdict *
strom_textdict_create(int type_oid, uint32_t nkeys_hint, int dindex, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	*p_errcode = 0;
	if ((type_oid != STROM_TEXTOID && type_oid != STROM_BPCHARNOID) || nkeys_hint > (1u << 28))
	{
		*p_errcode = StromError_BadRequestMessage;
		return nullptr;
	}
	Device *dev = get_device(dindex);
	if (!dev)
	{
		*p_errcode = StromError_ServerNotReady;
		return nullptr;
	}
	strom_textdict *dict = new strom_textdict();
	dict->type_oid = type_oid;
	dict->dindex = dindex;
	dict->blank_padded = (type_oid == STROM_BPCHARNOID);
	dict->nkeys_hint = nkeys_hint;
	if ((*p_errcode = textdict_allocate(dev, dict)) != 0)
	{
		textdict_free(dev, dict);
		delete dict;
		return nullptr;
	}
	{
		static uint64_t next_serial = 0;
		std::lock_guard<std::mutex> g(epoch_lock());
		dict->serial = ++next_serial;
		epoch_registry()[dict->serial] = dict->epoch;
	}
	return dict;
	STROM_ABI_CATCH(nullptr, p_errcode)
}

extern "C" uint32_t
strom_textdict_num_keys(strom_textdict *dict)
{
	return dict ? dict->nkeys : 0;
}

extern "C" void
strom_textdict_reset(strom_textdict *dict)
{
	Device *dev = dict ? get_device(dict->dindex) : nullptr;
	if (!dev)
		return;
	(void)hipSetDevice(dev->hip_id);
	{
		/* the ids of every coded column made so far name keys that are about to go */
		std::lock_guard<std::mutex> g(epoch_lock());
		epoch_registry()[dict->serial] = ++dict->epoch;
	}
	dict->nkeys = 0;
	dict->heap_usage = 0;
	(void)hipMemsetAsync(dict->slots, 0, sizeof(cl_ulong) * (size_t)dict->nslots, dev->streams[0]);
	(void)hipStreamSynchronize(dev->streams[0]);
}

extern "C" void
strom_textdict_release(strom_textdict *dict)
{
	if (!dict)
		return;
	{
		std::lock_guard<std::mutex> g(epoch_lock());
		epoch_registry().erase(dict->serial);
	}
	Device *dev = get_device(dict->dindex);
	if (dev)
	{
		(void)hipSetDevice(dev->hip_id);
		(void)hipStreamSynchronize(dev->streams[0]);
		textdict_free(dev, dict);
	}
	delete dict;
}

extern "C" int
strom_textdict_kernel_ns(strom_textdict *dict, uint64_t *ns_out)
{
	if (!dict || !ns_out)
		return StromError_BadRequestMessage;
	memcpy(ns_out, dict->kern_ns, sizeof(dict->kern_ns));
	return 0;
}

extern "C" strom_devprog_key
strom_textdict_program(strom_textdict *dict)
{
	return dict ? dict->program : 0;
}

extern "C" long
strom_textdict_fetch(strom_textdict *dict, void *heap_out, size_t heaplen,
					 uint64_t *offsets_out, size_t noffsets, size_t *p_heap_bytes)
{
	STROM_ABI_TRY
	if (!dict)
		return -(long)StromError_BadRequestMessage;
	if (p_heap_bytes)
		*p_heap_bytes = dict->heap_usage;
	if (!heap_out)
		return (long)dict->nkeys;
	Device *dev = get_device(dict->dindex);
	if (!dev)
		return -(long)StromError_ServerNotReady;
	if (heaplen < dict->heap_usage || noffsets < dict->nkeys || !offsets_out)
		return -(long)StromError_DataStoreNoSpace;
	(void)hipSetDevice(dev->hip_id);
	std::vector<textdict_entry> entries(dict->nkeys);
	if ((dict->heap_usage > 0 &&
		 hipMemcpy(heap_out, dict->heap, dict->heap_usage, hipMemcpyDeviceToHost) != hipSuccess) ||
		(dict->nkeys > 0 &&
		 hipMemcpy(entries.data(), dict->entries, sizeof(textdict_entry) * dict->nkeys,
				   hipMemcpyDeviceToHost) != hipSuccess))
		return -(long)StromError_HipInternal;
	for (cl_uint id = 0; id < dict->nkeys; id++)
	{
		if (entries[id].off >= dict->heap_usage)
			return -(long)StromError_SanityCheckViolation;
		offsets_out[id] = entries[id].off;
	}
	return (long)dict->nkeys;
	STROM_ABI_CATCH(-(long)StromError_OutOfMemory, (int *)nullptr)
}

extern "C" strom_dstore *
strom_textdict_encode(strom_textdict *const *dicts, const int32_t *key_colidx, int nkeys,
					  strom_dstore *src, const int32_t *carry_colidx, int ncarry, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	*p_errcode = StromError_BadRequestMessage;
	if (!dicts || !key_colidx || nkeys < 1 || nkeys > STROM_PREAGG_MAXKEYS || !src || ncarry < 0 ||
		ncarry > 64 || (ncarry > 0 && !carry_colidx))
		return nullptr;
	for (int i = 0; i < nkeys; i++)
		if (!dicts[i] || dicts[i]->dindex != src->dindex)
			return nullptr;
	if (src->head.format != KDS_FORMAT_COLUMN || src->head.ncols < 1 || src->head.ncols > 1600)
		return nullptr;
	Device *dev = get_device(src->dindex);
	if (!dev)
	{
		*p_errcode = StromError_ServerNotReady;
		return nullptr;
	}
	int		src_ncols = (int)src->head.ncols;
	cl_uint	nrows = src->head.nitems;
	for (int i = 0; i < nkeys; i++)
		if (key_colidx[i] < 0 || key_colidx[i] >= src_ncols)
			return nullptr;
	for (int i = 0; i < ncarry; i++)
		if (carry_colidx[i] < 0 || carry_colidx[i] >= src_ncols)
			return nullptr;
	(void)hipSetDevice(dev->hip_id);
	/* the source's column metadata and directory */
	std::vector<char> shead(KDS_COLUMN_HEAD_LENGTH(src_ncols), 0);
	if (shead.size() > src->length)
		return nullptr;
	if (hipMemcpy(shead.data(), src->devptr, shead.size(), hipMemcpyDeviceToHost) != hipSuccess)
	{
		*p_errcode = StromError_HipInternal;
		return nullptr;
	}
	const kern_data_store *skds = (const kern_data_store *)shead.data();
	const kern_coldir *scd = KERN_DATA_STORE_COLDIR(skds);
	size_t	varwidth = sizeof(cl_ulong) * (size_t)nrows;
	size_t	bitmap_len = sizeof(cl_uint) * (((size_t)nrows + 31) / 32);
	for (int i = 0; i < nkeys; i++)
	{
		const kern_coldir *cd = &scd[key_colidx[i]];
		if (skds->colmeta[key_colidx[i]].attlen != -1)
			return nullptr;							/* not a varlena column */
		if ((size_t)cd->values_off + varwidth > src->length ||
			(cd->nulls_off != 0 && (size_t)cd->nulls_off + bitmap_len > src->length))
		{
			*p_errcode = StromError_DataStoreCorruption;
			return nullptr;
		}
	}
	for (int i = 0; i < ncarry; i++)
	{
		const kern_coldir *cd = &scd[carry_colidx[i]];
		int		attlen = skds->colmeta[carry_colidx[i]].attlen;
		if (!(attlen == 1 || attlen == 2 || attlen == 4 || attlen == 8))
			return nullptr;							/* varlena columns are not carried */
		if ((size_t)cd->values_off + (size_t)attlen * nrows > src->length ||
			(cd->nulls_off != 0 && (size_t)cd->nulls_off + bitmap_len > src->length))
		{
			*p_errcode = StromError_DataStoreCorruption;
			return nullptr;
		}
	}
	*p_errcode = 0;
	Encoder	enc;
	strom_devprog_key progkey = 0;
	if ((*p_errcode = enc.open(dev, K_PROBE, K_REBUILD, &progkey)) != 0)
		return nullptr;

	/* the encoded chunk: id columns (bitmap room always laid out, named in the directory only
	 * when the column has a NULL), then the carried columns as they are */
	int		ncols = nkeys + ncarry;
	std::vector<char> hbuf(KDS_COLUMN_HEAD_LENGTH(ncols), 0);
	kern_data_store *head = (kern_data_store *)hbuf.data();
	head->ncols = ncols;
	kern_coldir *cd = KERN_DATA_STORE_COLDIR(head);
	std::vector<size_t> nulls_at(ncols, 0);
	size_t	off = hbuf.size();
	for (int c = 0; c < ncols; c++)
	{
		const kern_colmeta *scm = (c < nkeys ? nullptr : &skds->colmeta[carry_colidx[c - nkeys]]);
		int		attlen = (scm ? scm->attlen : 4);
		head->colmeta[c].attbyval = 1;
		head->colmeta[c].attalign = (cl_char)attlen;
		head->colmeta[c].attlen = (cl_short)attlen;
		head->colmeta[c].attnum = (cl_short)(c + 1);
		head->colmeta[c].attcacheoff = -1;
		cd[c].values_off = (cl_uint)off;
		off += KDS_COLUMN_VALUES_LENGTH(attlen, nrows);
		if (c < nkeys || scd[carry_colidx[c - nkeys]].nulls_off != 0)
		{
			nulls_at[c] = off;
			off += KDS_COLUMN_NULLS_LENGTH(nrows);
		}
		if (off > 0xffffffffUL)
		{
			*p_errcode = StromError_DataStoreOutOfRange;
			return nullptr;
		}
	}
	head->hostptr = 0;
	head->length = (cl_uint)off;
	head->usage = 0;
	head->nitems = nrows;
	head->nrooms = nrows;
	head->format = KDS_FORMAT_COLUMN;
	head->tdtypeid = skds->tdtypeid;
	head->tdtypmod = skds->tdtypmod;

	char	   *d_dst = (char *)dev->pool.alloc(off);
	cl_uint	   *d_row_slot = (cl_uint *)dev->pool.alloc(sizeof(cl_uint) * std::max<size_t>(nrows, 1));
	textdict_newkey *d_newkeys = (textdict_newkey *)dev->pool.alloc(sizeof(textdict_newkey) * std::max<size_t>(nrows, 1));
	strom_dstore *result = nullptr;
	do {
		if (!d_dst || !d_row_slot || !d_newkeys)
		{
			*p_errcode = StromError_OutOfMemory;
			break;
		}
		std::vector<cl_uint> nnull(nkeys, 0);
		for (int i = 0; i < nkeys && *p_errcode == 0; i++)
		{
			memset(dicts[i]->kern_ns, 0, sizeof(dicts[i]->kern_ns));
			dicts[i]->program = progkey;
			enc.rebuild_ns = &dicts[i]->kern_ns[K_REBUILD];
			*p_errcode = enc.encode_column(dicts[i], src, (cl_uint)key_colidx[i], d_row_slot, d_newkeys,
										   d_dst + cd[i].values_off, d_dst + nulls_at[i], &nnull[i]);
		}
		if (*p_errcode != 0)
			break;
		for (int c = 0; c < ncols; c++)
		{
			if (c < nkeys)
			{
				/* the ids' domain: what a dense session of GpuPreAgg is opened with */
				cl_uint		nk = dicts[c]->nkeys;
				cd[c].nulls_off = (nnull[c] > 0 ? (cl_uint)nulls_at[c] : 0);
				cd[c].stat_flags = (nk > 0 && nnull[c] < nrows ? KDS_COLSTAT_MINMAX : 0);
				cd[c].minval = 0;
				cd[c].maxval = (nk > 0 ? (cl_long)nk - 1 : 0);
				continue;
			}
			const kern_coldir *from = &scd[carry_colidx[c - nkeys]];
			size_t		width = (size_t)head->colmeta[c].attlen * nrows;
			cd[c].nulls_off = (cl_uint)nulls_at[c];
			cd[c].stat_flags = from->stat_flags;
			cd[c].minval = from->minval;
			cd[c].maxval = from->maxval;
			if ((width > 0 &&
				 hipMemcpyAsync(d_dst + cd[c].values_off, (const char *)src->devptr + from->values_off, width,
								hipMemcpyDeviceToDevice, enc.stream) != hipSuccess) ||
				(nulls_at[c] != 0 && bitmap_len > 0 &&
				 hipMemcpyAsync(d_dst + nulls_at[c], (const char *)src->devptr + from->nulls_off, bitmap_len,
								hipMemcpyDeviceToDevice, enc.stream) != hipSuccess))
			{
				*p_errcode = StromError_HipInternal;
				break;
			}
		}
		if (*p_errcode != 0)
			break;
		if (hipMemcpyAsync(d_dst, hbuf.data(), hbuf.size(), hipMemcpyHostToDevice, enc.stream) != hipSuccess ||
			hipStreamSynchronize(enc.stream) != hipSuccess)
		{
			*p_errcode = StromError_HipInternal;
			break;
		}
		result = new strom_dstore{d_dst, off, src->dindex, true, {}};
		memcpy(&result->head, head, offsetof(kern_data_store, colmeta));
	} while (0);
	if (!result)
		(void)hipStreamSynchronize(enc.stream);
	if (d_row_slot) dev->pool.release(d_row_slot);
	if (d_newkeys) dev->pool.release(d_newkeys);
	if (!result && d_dst) dev->pool.release(d_dst);
	return result;
	STROM_ABI_CATCH(nullptr, p_errcode)
}

/* ------------------------------------------------------------------ *
 * a dimension's text column as a coded column (devlib/strom_textdict.h: textdict_table_*), the
 * dictionary's half of strom_textdict_encode_table (gpuhashjoin.cpp owns the table and the arrays)
 * ------------------------------------------------------------------ */
int
strom::textdict_identity(strom_textdict *dict, int *p_dindex, uint64_t *p_serial, uint64_t *p_epoch)
{
	if (!dict)
		return StromError_BadRequestMessage;
	*p_dindex = dict->dindex;
	*p_serial = dict->serial;
	*p_epoch = dict->epoch;
	return 0;
}

bool
strom::textdict_epoch_is_current(uint64_t serial, uint64_t epoch)
{
	std::lock_guard<std::mutex> g(epoch_lock());
	auto	it = epoch_registry().find(serial);
	return it != epoch_registry().end() && it->second == epoch;
}

/*
 * One encode over the slots of a table: offsets (every datum checked; an error ends the call before
 * the dictionary is touched) -> the policy of an encode of a chunk (Encoder::encode_rows), its rows
 * being the table's slots.  d_ids / d_isnull: tbl_nslots long, the caller's.
 */
int
strom::textdict_encode_table_slots(strom_textdict *dict, const void *d_kmhash, const void *d_index,
								   cl_uint tbl_nslots, int colidx, void *d_ids, void *d_isnull)
{
	Device *dev = dict ? get_device(dict->dindex) : nullptr;
	if (!dev)
		return dict ? StromError_ServerNotReady : StromError_BadRequestMessage;
	if (tbl_nslots < 1 || tbl_nslots > (1u << 31))
		return StromError_BadRequestMessage;
	(void)hipSetDevice(dev->hip_id);
	Encoder	enc;
	strom_devprog_key progkey = 0;
	int		rc = enc.open(dev, K_REBUILD, K_TEMIT, &progkey);
	if (rc != 0)
		return rc;
	cl_ulong   *d_datum_off = (cl_ulong *)dev->pool.alloc(sizeof(cl_ulong) * (size_t)tbl_nslots);
	cl_uint	   *d_row_slot = (cl_uint *)dev->pool.alloc(sizeof(cl_uint) * (size_t)tbl_nslots);
	textdict_newkey *d_newkeys = (textdict_newkey *)dev->pool.alloc(sizeof(textdict_newkey) * (size_t)tbl_nslots);
	rc = (!d_datum_off || !d_row_slot || !d_newkeys) ? StromError_OutOfMemory : 0;
	if (rc == 0)
	{
		textdict_table_args t;
		textdict_args a = enc.base_args(dict);
		textdict_ctl ctl;
		void	   *args[] = { &t, &a };
		cl_uint		nnull = 0;

		memset(&t, 0, sizeof(t));
		t.kmhash = (cl_ulong)(uintptr_t)d_kmhash;
		t.hjidx = (cl_ulong)(uintptr_t)d_index;
		t.datum_off = (cl_ulong)(uintptr_t)d_datum_off;
		t.out_ids = (cl_ulong)(uintptr_t)d_ids;
		t.out_isnull = (cl_ulong)(uintptr_t)d_isnull;
		t.tbl_nslots = tbl_nslots;
		t.colidx = colidx;
		memset(dict->kern_ns, 0, sizeof(dict->kern_ns));
		dict->program = progkey;
		enc.rebuild_ns = &dict->kern_ns[K_REBUILD];
		/* (the offsets pass is part of finding the rows' keys: its time goes to the probe's account) */
		if (hipMemsetAsync(dict->ctl, 0, sizeof(textdict_ctl), enc.stream) != hipSuccess)
			rc = StromError_HipInternal;
		else if ((rc = enc.launch(&dict->kern_ns[K_PROBE], K_TOFFSETS, enc.grid_for(tbl_nslots), args)) == 0 &&
				 (rc = enc.read_ctl(dict, &ctl)) == 0)
			rc = ctl.status;
		if (rc == 0)
			rc = enc.encode_rows(dict, K_TPROBE, &t, tbl_nslots, (cl_uint)colidx, d_row_slot, d_newkeys,
								 nullptr, nullptr, &nnull);
	}
	(void)hipStreamSynchronize(enc.stream);
	if (d_datum_off) dev->pool.release(d_datum_off);
	if (d_row_slot) dev->pool.release(d_row_slot);
	if (d_newkeys) dev->pool.release(d_newkeys);
	return rc;
}

/* ------------------------------------------------------------------ *
 * union of dictionaries (devlib/strom_textdict.h: keyunion_*)
 *
 * One absorb:
 *   probe -> read {status, nnew, toofull} -> NoSpace: grow, rebuild, probe again; another error:
 *   rebuild at the same size and return it, as an encode does
 *   count, offsets -> read the totals (the one other small copy) -> room for entries and heap
 *   settle, emit -> read status -> the counters move
 * ------------------------------------------------------------------ */
struct strom_keymap {
	strom_textdict *dst = nullptr;
	int			dindex = 0;
	cl_uint		n = 0;
	cl_int	   *ids = nullptr;			/* device: int4[n] */
	cl_int	   *status = nullptr;		/* device: the word a recode reports through */
};

namespace {

void
keymap_free(Device *dev, strom_keymap *map)
{
	if (map->ids) dev->pool.release(map->ids);
	if (map->status) dev->pool.release(map->status);
	delete map;
}

/* the image lies on the device: heap[heaplen], key i at the offset found at offsets + i * stride */
strom_keymap *
absorb_image(Device *dev, strom_textdict *dst, const char *d_heap, size_t heaplen,
			 const void *d_offsets, cl_uint stride, cl_uint nimg, int *p_errcode)
{
	Encoder		enc;
	strom_devprog_key progkey = 0;
	int			rc;

	if ((*p_errcode = enc.open(dev, K_REBUILD, K_UEMIT, &progkey)) != 0)
		return nullptr;
	memset(dst->union_ns, 0, sizeof(uint64_t) * U_RECODE);
	enc.rebuild_ns = &dst->union_ns[U_REBUILD];
	dst->program = progkey;

	strom_keymap *map = new strom_keymap();
	map->dst = dst;
	map->dindex = dst->dindex;
	map->n = nimg;
	map->ids = (cl_int *)dev->pool.alloc(sizeof(cl_int) * std::max<size_t>(nimg, 1));
	map->status = (cl_int *)dev->pool.alloc(sizeof(cl_int));
	cl_uint		ntiles = (cl_uint)(((size_t)nimg + enc.block - 1) / enc.block);
	cl_uint	   *d_key_slot = (cl_uint *)dev->pool.alloc(sizeof(cl_uint) * std::max<size_t>(nimg, 1));
	keyunion_tile *d_tiles = (keyunion_tile *)dev->pool.alloc(sizeof(keyunion_tile) * ((size_t)ntiles + 1));
	bool		touched = false;			/* the slot array may hold claims of this call */

	auto args_of = [&](void) {
		keyunion_args a;
		memset(&a, 0, sizeof(a));
		a.slots = (cl_ulong)(uintptr_t)dst->slots;
		a.entries = (cl_ulong)(uintptr_t)dst->entries;
		a.heap = (cl_ulong)(uintptr_t)dst->heap;
		a.ctl = (cl_ulong)(uintptr_t)dst->ctl;
		a.img_heap = (cl_ulong)(uintptr_t)d_heap;
		a.img_offsets = (cl_ulong)(uintptr_t)d_offsets;
		a.img_heaplen = heaplen;
		a.key_slot = (cl_ulong)(uintptr_t)d_key_slot;
		a.tiles = (cl_ulong)(uintptr_t)d_tiles;
		a.map = (cl_ulong)(uintptr_t)map->ids;
		a.heap_usage = dst->heap_usage;
		a.heap_size = dst->heap_size;
		a.img_stride = stride;
		a.nimg = nimg;
		a.ntiles = ntiles;
		a.nslots = dst->nslots;
		a.nkeys = dst->nkeys;
		a.blank_padded = dst->blank_padded ? 1 : 0;
		return a;
	};

	rc = (!map->ids || !map->status || !d_key_slot || !d_tiles) ? StromError_OutOfMemory : 0;
	textdict_ctl ctl;
	keyunion_tile total;
	memset(&ctl, 0, sizeof(ctl));
	memset(&total, 0, sizeof(total));
	for (int turn = 0; rc == 0 && nimg > 0; turn++)
	{
		keyunion_args a = args_of();
		void	   *args[] = { &a };

		if (hipMemsetAsync(dst->ctl, 0, sizeof(textdict_ctl), enc.stream) != hipSuccess)
		{
			rc = StromError_HipInternal;
			break;
		}
		touched = true;
		if ((rc = enc.launch(&dst->union_ns[U_PROBE], K_UPROBE, enc.grid_for(nimg), args)) != 0 ||
			(rc = enc.read_ctl(dst, &ctl)) != 0)
			break;
		size_t	keys_after = (size_t)dst->nkeys + ctl.nnew;
		bool	nospace = (ctl.status == StromError_DataStoreNoSpace || (ctl.status == 0 && ctl.toofull != 0));

		if (ctl.status != 0 && !nospace)
		{
			rc = ctl.status;				/* a key of the image is broken: nothing of it stays */
			break;
		}
		if (!nospace)
			break;
		if (turn >= 40 || keys_after >= ((size_t)1 << 29))
		{
			rc = StromError_DataStoreNoSpace;
			break;
		}
		cl_uint	nslots = std::max(pow2_at_least(4 * keys_after), pow2_at_least(8 * (size_t)dst->nslots));
		rc = enc.rebuild(dst, nslots);		/* drops the claims; the next turn probes again */
	}
	if (rc == 0 && nimg > 0)
	{
		/* which keys are new, in image order, and what they need */
		keyunion_args a = args_of();
		void	   *args[] = { &a };

		if ((rc = enc.launch(&dst->union_ns[U_RANKS], K_UCOUNT, std::min(ntiles, enc.max_grid), args)) == 0 &&
			(rc = enc.launch(&dst->union_ns[U_RANKS], K_UOFFSETS, 1, args)) == 0 &&
			(hipMemcpyAsync(&total, d_tiles + ntiles, sizeof(total), hipMemcpyDeviceToHost, enc.stream) != hipSuccess ||
			 hipStreamSynchronize(enc.stream) != hipSuccess))
			rc = StromError_HipInternal;
		if (rc == 0 && (rc = enc.read_ctl(dst, &ctl)) == 0 && ctl.status != 0)
			rc = ctl.status;
		if (rc == 0 && total.count != ctl.nnew)
			rc = StromError_SanityCheckViolation;			/* every claim is one new key */
		size_t	keys_after = (size_t)dst->nkeys + total.count;
		if (rc == 0 && keys_after >= ((size_t)1 << 29))
			rc = StromError_DataStoreNoSpace;
		/* entries and heap are not what the slot words name: they grow without another probe */
		if (rc == 0 && keys_after > dst->entries_cap)
		{
			size_t	need = std::max(keys_after, 2 * (size_t)dst->entries_cap);
			if ((rc = enc.grow(&dst->entries, dst->nkeys, need)) == 0)
				dst->entries_cap = (cl_uint)need;
		}
		if (rc == 0 && dst->heap_usage + total.bytes > dst->heap_size)
		{
			size_t	need = std::max(dst->heap_usage + (size_t)total.bytes, 2 * dst->heap_size);
			if ((rc = enc.grow(&dst->heap, dst->heap_usage, need)) == 0)
				dst->heap_size = need;
		}
	}
	if (rc == 0 && nimg > 0)
	{
		keyunion_args a = args_of();
		void	   *args[] = { &a };

		if (total.count > 0)
			rc = enc.launch(&dst->union_ns[U_SETTLE], K_USETTLE, std::min(ntiles, enc.max_grid), args);
		a.nkeys = dst->nkeys + total.count;
		if (rc == 0 && (rc = enc.launch(&dst->union_ns[U_EMIT], K_UEMIT, enc.grid_for(nimg), args)) == 0 &&
			(rc = enc.read_ctl(dst, &ctl)) == 0)
			rc = ctl.status;
	}
	(void)hipStreamSynchronize(enc.stream);
	if (rc == 0)
	{
		dst->nkeys += total.count;
		dst->heap_usage += total.bytes;
		if (2 * (size_t)dst->nkeys > dst->nslots)
			rc = enc.rebuild(dst, pow2_at_least(4 * (size_t)dst->nkeys));
	}
	else if (touched && dst->slots)
		(void)enc.rebuild(dst, dst->nslots);	/* back to the keys before the call: entries below nkeys */
	if (d_key_slot) dev->pool.release(d_key_slot);
	if (d_tiles) dev->pool.release(d_tiles);
	if (rc != 0)
	{
		keymap_free(dev, map);
		*p_errcode = rc;
		return nullptr;
	}
	return map;
}

/* a host image before any launch: every datum inside the heap by its own length, with a header
 * the device reads in place */
bool
host_image_is_sound(const unsigned char *heap, size_t heaplen, const uint64_t *offsets, uint32_t nkeys)
{
	for (uint32_t i = 0; i < nkeys; i++)
	{
		uint64_t	off = offsets[i];
		if (off >= heaplen)
			return false;
		unsigned char b0 = heap[off];
		if (b0 == 0x01 || (b0 & 0x03) == 0x02)
			return false;
		uint64_t	size;
		if (b0 & 0x01)
			size = (b0 >> 1) & 0x7f;
		else
		{
			if (off + 4 > heaplen)
				return false;
			uint32_t w = (uint32_t)heap[off] | ((uint32_t)heap[off + 1] << 8) |
				((uint32_t)heap[off + 2] << 16) | ((uint32_t)heap[off + 3] << 24);
			size = (w >> 2) & 0x3fffffff;
		}
		if (size < ((b0 & 0x01) ? 1u : 4u) || off + size > heaplen)
			return false;
	}
	return true;
}

}	/* namespace */

extern "C" strom_keymap *
strom_keyunion_absorb(strom_textdict *dst, const void *heap, size_t heaplen,
					  const uint64_t *offsets, uint32_t nkeys, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	*p_errcode = StromError_BadRequestMessage;
	if (!dst || nkeys > (1u << 28) || (nkeys > 0 && (!heap || !offsets)))
		return nullptr;
	Device *dev = get_device(dst->dindex);
	if (!dev)
	{
		*p_errcode = StromError_ServerNotReady;
		return nullptr;
	}
	if (!host_image_is_sound((const unsigned char *)heap, heaplen, offsets, nkeys))
	{
		*p_errcode = StromError_DataStoreCorruption;
		return nullptr;
	}
	(void)hipSetDevice(dev->hip_id);
	*p_errcode = 0;
	char	   *d_heap = nullptr;
	uint64_t   *d_offsets = nullptr;
	if (nkeys > 0)
	{
		d_heap = (char *)dev->pool.alloc(heaplen);
		d_offsets = (uint64_t *)dev->pool.alloc(sizeof(uint64_t) * nkeys);
		if (!d_heap || !d_offsets)
			*p_errcode = StromError_OutOfMemory;
		else if (hipMemcpyAsync(d_heap, heap, heaplen, hipMemcpyHostToDevice, dev->streams[0]) != hipSuccess ||
				 hipMemcpyAsync(d_offsets, offsets, sizeof(uint64_t) * nkeys, hipMemcpyHostToDevice,
								dev->streams[0]) != hipSuccess ||
				 hipStreamSynchronize(dev->streams[0]) != hipSuccess)
			*p_errcode = StromError_HipInternal;
	}
	strom_keymap *map = nullptr;
	if (*p_errcode == 0)
		map = absorb_image(dev, dst, d_heap, heaplen, d_offsets, sizeof(uint64_t), nkeys, p_errcode);
	if (d_heap) dev->pool.release(d_heap);
	if (d_offsets) dev->pool.release(d_offsets);
	return map;
	STROM_ABI_CATCH(nullptr, p_errcode)
}

extern "C" strom_keymap *
strom_keyunion_absorb_dict(strom_textdict *dst, strom_textdict *src, int *p_errcode)
{
	STROM_ABI_TRY
	int		dummy;
	if (!p_errcode)
		p_errcode = &dummy;
	*p_errcode = StromError_BadRequestMessage;
	if (!dst || !src || dst == src || dst->type_oid != src->type_oid || dst->dindex != src->dindex)
		return nullptr;
	Device *dev = get_device(dst->dindex);
	if (!dev)
	{
		*p_errcode = StromError_ServerNotReady;
		return nullptr;
	}
	(void)hipSetDevice(dev->hip_id);
	*p_errcode = 0;
	/* src's heap and the 'off' words of its entries are the image, where they lie */
	return absorb_image(dev, dst, src->heap, src->heap_usage, &src->entries[0].off,
						sizeof(textdict_entry), src->nkeys, p_errcode);
	STROM_ABI_CATCH(nullptr, p_errcode)
}

extern "C" uint32_t
strom_keymap_size(strom_keymap *map)
{
	return map ? map->n : 0;
}

extern "C" int
strom_keymap_fetch(strom_keymap *map, int32_t *out, size_t n)
{
	if (!map || (!out && map->n > 0))
		return StromError_BadRequestMessage;
	if (n < map->n)
		return StromError_DataStoreNoSpace;
	Device *dev = get_device(map->dindex);
	if (!dev)
		return StromError_ServerNotReady;
	(void)hipSetDevice(dev->hip_id);
	if (map->n > 0 && hipMemcpy(out, map->ids, sizeof(cl_int) * map->n, hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_HipInternal;
	return 0;
}

extern "C" void
strom_keymap_release(strom_keymap *map)
{
	if (!map)
		return;
	Device *dev = get_device(map->dindex);
	if (dev)
	{
		(void)hipSetDevice(dev->hip_id);
		(void)hipStreamSynchronize(dev->streams[0]);
		keymap_free(dev, map);
	}
	else
		delete map;
}

extern "C" int
strom_keyunion_kernel_ns(strom_textdict *dst, uint64_t *ns_out)
{
	if (!dst || !ns_out)
		return StromError_BadRequestMessage;
	memcpy(ns_out, dst->union_ns, sizeof(dst->union_ns));
	return 0;
}

extern "C" int
strom_keyunion_recode(strom_dstore *encoded, const int32_t *colidx, strom_keymap *const *maps, int ncols)
{
	STROM_ABI_TRY
	if (!encoded || !colidx || !maps || ncols < 1 || ncols > STROM_PREAGG_MAXKEYS)
		return StromError_BadRequestMessage;
	if (encoded->head.format != KDS_FORMAT_COLUMN || encoded->head.ncols < 1 || encoded->head.ncols > 1600)
		return StromError_BadRequestMessage;
	int		chunk_ncols = (int)encoded->head.ncols;
	for (int i = 0; i < ncols; i++)
	{
		if (!maps[i] || maps[i]->dindex != encoded->dindex || colidx[i] < 0 || colidx[i] >= chunk_ncols)
			return StromError_BadRequestMessage;
		for (int j = 0; j < i; j++)
			if (colidx[j] == colidx[i])
				return StromError_BadRequestMessage;		/* a column is recoded once */
	}
	Device *dev = get_device(encoded->dindex);
	if (!dev)
		return StromError_ServerNotReady;
	(void)hipSetDevice(dev->hip_id);
	std::vector<char> hbuf(KDS_COLUMN_HEAD_LENGTH(chunk_ncols), 0);
	if (hbuf.size() > encoded->length)
		return StromError_BadRequestMessage;
	if (hipMemcpy(hbuf.data(), encoded->devptr, hbuf.size(), hipMemcpyDeviceToHost) != hipSuccess)
		return StromError_HipInternal;
	const kern_data_store *head = (const kern_data_store *)hbuf.data();
	kern_coldir *cd = KERN_DATA_STORE_COLDIR(head);
	cl_uint	nrows = encoded->head.nitems;
	size_t	bitmap_len = sizeof(cl_uint) * (((size_t)nrows + 31) / 32);
	for (int i = 0; i < ncols; i++)
	{
		const kern_colmeta *cm = &head->colmeta[colidx[i]];
		if (cm->attlen != 4 || !cm->attbyval)
			return StromError_BadRequestMessage;			/* not a column of int4 ids */
		if ((size_t)cd[colidx[i]].values_off + sizeof(cl_int) * (size_t)nrows > encoded->length ||
			(cd[colidx[i]].nulls_off != 0 && (size_t)cd[colidx[i]].nulls_off + bitmap_len > encoded->length))
			return StromError_DataStoreCorruption;
	}
	Encoder	enc;
	strom_devprog_key progkey = 0;
	int		rc = enc.open(dev, K_RECODE, K_RECODE, &progkey);
	if (rc != 0)
		return rc;
	for (int i = 0; i < ncols; i++)
		maps[i]->dst->union_ns[U_RECODE] = 0;
	for (int i = 0; i < ncols && rc == 0; i++)
	{
		strom_keymap *map = maps[i];
		const void *a_chunk = encoded->devptr;
		keyunion_recode_args a;
		memset(&a, 0, sizeof(a));
		a.map = (cl_ulong)(uintptr_t)map->ids;
		a.status = (cl_ulong)(uintptr_t)map->status;
		a.mapsize = map->n;
		a.colidx = (cl_uint)colidx[i];
		void	   *args[] = { &a_chunk, &a };
		cl_int		status = 0;

		if (hipMemsetAsync(map->status, 0, sizeof(cl_int), enc.stream) != hipSuccess)
			rc = StromError_HipInternal;
		else if ((rc = enc.launch(&map->dst->union_ns[U_RECODE], K_RECODE, enc.grid_for(nrows), args)) == 0)
		{
			if (hipMemcpyAsync(&status, map->status, sizeof(status), hipMemcpyDeviceToHost, enc.stream) != hipSuccess ||
				hipStreamSynchronize(enc.stream) != hipSuccess)
				rc = StromError_HipInternal;
			else
				rc = status;
		}
		/* the ids' new domain */
		kern_coldir *c = &cd[colidx[i]];
		cl_uint		nk = map->dst->nkeys;
		if (rc == 0 && nk > 0 && (c->stat_flags & KDS_COLSTAT_MINMAX) != 0)
		{
			c->minval = 0;
			c->maxval = (cl_long)nk - 1;
			if (hipMemcpy((char *)encoded->devptr + ((const char *)c - hbuf.data()), c, sizeof(*c),
						  hipMemcpyHostToDevice) != hipSuccess)
				rc = StromError_HipInternal;
		}
	}
	if (rc != 0)
		(void)hipStreamSynchronize(enc.stream);
	encoded->coldir.reset();				/* the host's snapshot of the zone maps is of the old ids */
	return rc;
	STROM_ABI_CATCH(StromError_OutOfMemory, (int *)nullptr)
}
