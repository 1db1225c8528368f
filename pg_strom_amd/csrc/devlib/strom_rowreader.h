/*
 * strom_rowreader.h
 *
 * The row reader of the row-at-a-time kernels: the kernels that take a chunk of
 * any format and an optional row map (gpuscan_qual_generic, gpuhashjoin_main,
 * gpupreagg_dense_generic / _census / _keyrange and the hashed GROUP BY's check,
 * fold and scatter passes).  How a row's variables are found is written here,
 * once.
 *
 * An operator's header includes this file after it has defined strom_kvars,
 * strom_kvars_from_column() and STROM_KVARS_FINISH(KV), its last step on a row's
 * assembled variables.
 *
 * The reader is a set of locals of the kernel body, declared by two statements,
 *
 *   STROM_ROW_READER_MAP(kds, krowmap);          rr_nrows loop positions, rr_use_map
 *   STROM_ROW_READER(IS_COLUMN, kds, ktoast);    format, column pointers
 *
 * and used per row through
 *
 *   STROM_ROW_INDEX(r)                           loop position -> row of the chunk
 *   STROM_ROW_LOAD_ROW(KV, errcode, kds_index);          the whole row, ready for the expressions
 *   STROM_ROW_LOAD(LIST, HOW, KV, errcode, kds_index);   the variables of LIST only, HOW = NT | CACHED
 *
 * - The chunk format is a compile-time choice (IS_COLUMN: the other accessor is
 *   not compiled in) plus ONE test, rr_row_family, made per launch.
 * - COLUMN: the column and NULL-bitmap pointers are taken from the chunk's
 *   directory once per launch and stay wave-uniform; no chunk header field is
 *   read per row.
 * - ROW / ROW_FLAT: the heap tuple is located once per row (row item -> page ->
 *   line pointer is a chain of dependent loads) and every variable is taken from
 *   it.  TUPSLOT: the per-datum accessor, pg_<T>_vref.
 * - errcode is the row's 'cl_int' error word: the row formats' accessors raise in it.
 * - Each STROM_ROW_LOAD locates the tuple of a ROW / ROW_FLAT chunk: a row's lists are
 *   loaded by one call (only the hash roles load two lists, and they read COLUMN chunks).
 */
#ifndef STROM_ROWREADER_DEVICE_H
#define STROM_ROWREADER_DEVICE_H

#define STROM_ROW_READER_MAP(kds, krowmap)												\
	const kern_row_map *const rr_krowmap = (krowmap);									\
	const bool	rr_use_map = (rr_krowmap != NULL && rr_krowmap->nvalids >= 0);			\
	const cl_uint rr_nrows = (rr_use_map ? (cl_uint)rr_krowmap->nvalids : (kds)->nitems)

#define STROM_ROW_INDEX(r)	(rr_use_map ? (cl_uint)rr_krowmap->rindex[r] : (cl_uint)(r))

#define STROM_ROW_READER_COLUMN_(attno,colidx,NAME)										\
	const char *col_##attno = (rr_is_column ? (const char *)rr_kds + rr_coldir[colidx].values_off : NULL);	\
	const cl_uint *nul_##attno = ((rr_is_column && rr_coldir[colidx].nulls_off != 0)	\
		? (const cl_uint *)((const char *)rr_kds + rr_coldir[colidx].nulls_off) : NULL);
#define STROM_ROW_READER(IS_COLUMN, kds, ktoast)										\
	const bool	rr_is_column = (IS_COLUMN);												\
	const kern_data_store *const rr_kds = (kds);										\
	const kern_data_store *const rr_ktoast = (ktoast);									\
	const cl_int rr_format = rr_kds->format;											\
	const bool	rr_row_family = (rr_format == KDS_FORMAT_ROW || rr_format == KDS_FORMAT_ROW_FLAT);	\
	const kern_coldir *const rr_coldir = KERN_DATA_STORE_COLDIR(rr_kds);				\
	STROM_KVAR_LIST(STROM_ROW_READER_COLUMN_)

/*
 * HOW a COLUMN chunk's values are loaded: NT, non-temporally (STROM_COLUMN_REF), or CACHED,
 * through the caches -- for rows that several work-groups of an XCD read one after the other
 * (the hash roles of the hashed GROUP BY)
 */
/* one variable from the located heap tuple; NULL where the tuple or the column is not there */
#define STROM_ROW_TUPLE_REF_(NAME, colidx)												\
	((rr_htup != NULL && (cl_uint)(colidx) < rr_kds->ncols)								\
	 ? pg_##NAME##_tupref(&rr_errcode, rr_kds->colmeta, rr_htup, colidx)				\
	 : pg_##NAME##_make(0, true))
#define STROM_ROW_REF_(COLUMN_REF,attno,colidx,NAME)									\
	rr_kv.KVAR_##attno = (rr_is_column													\
		? COLUMN_REF(NAME, col_##attno, nul_##attno, rr_index)							\
		: rr_row_family ? STROM_ROW_TUPLE_REF_(NAME, colidx)							\
		: pg_##NAME##_vref(rr_kds, rr_ktoast, &rr_errcode, colidx, rr_index));
#define STROM_ROW_REF_NT_(attno,colidx,NAME)		STROM_ROW_REF_(STROM_COLUMN_REF,attno,colidx,NAME)
#define STROM_ROW_REF_CACHED_(attno,colidx,NAME)	STROM_ROW_REF_(STROM_COLUMN_REF_CACHED,attno,colidx,NAME)
#define STROM_ROW_LOAD(LIST, HOW, KV, ERRCODE, kds_index)								\
	do {																				\
		strom_kvars &rr_kv = (KV);														\
		cl_int	   &rr_errcode = (ERRCODE);												\
		const cl_uint rr_index = (kds_index);											\
		const HeapTupleHeaderData *rr_htup = NULL;										\
		if (!rr_is_column && rr_row_family)												\
			rr_htup = strom_locate_tuple(rr_kds, rr_format, rr_index);					\
		LIST(STROM_ROW_REF_##HOW##_)													\
	} while (0)

#define STROM_ROW_LOAD_ROW(KV, ERRCODE, kds_index)										\
	do {																				\
		STROM_ROW_LOAD(STROM_KVAR_LIST, NT, KV, ERRCODE, kds_index);					\
		if (rr_is_column)																\
			strom_kvars_from_column(KV, rr_kds, &(ERRCODE));							\
		STROM_KVARS_FINISH(KV);															\
	} while (0)

#endif	/* STROM_ROWREADER_DEVICE_H */
