/*
 * strom_textdict_table.h -- part of the C ABI of libstrom_hip.so (included by strom_hip.h, which
 * declares strom_textdict and strom_hashjoin_table): a DIMENSION's text column as a coded column.
 *
 * "SELECT dim.name, sum(..) FROM fact JOIN dim .. GROUP BY dim.name": the name is a property of the
 * few dimension rows, not of the fact rows.  The dictionary that encodes a chunk's text column
 * (strom_textdict_encode) also walks the rows of a hash table, once, at table time, and leaves an
 * int4 id per SLOT with the table.  Every fused fold -- strom_submit_gpupreagg_lookup,
 * _lookup_star, _lookup_typed, _lookup_snowflake -- then serves those ids like any int4 column of the
 * relation: a virtual column mapped with src_depth = d, src_colidx = the index returned here and
 * type_oids = int4; the aggregate program names it (var K int4) as a group key, in the qual or in an
 * aggregate's argument; the domain of a dense session is {0, num_keys-1}, as for an encoded chunk;
 * the caller replaces ids by key datums after the fetch (strom_textdict_fetch).  No text datum enters
 * a slot record or a fold kernel: a text VARIABLE mapped to a relation stays refused.
 */
#ifndef STROM_TEXTDICT_TABLE_H
#define STROM_TEXTDICT_TABLE_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * inner column colidx (0-based, attlen -1) of the table's one relation under dict: a coded column, int4
 * ids by slot, kept with the table.  Returns its column index (>= the relation's own ncols), negative:
 * -errcode.  Blocks like strom_textdict_encode and follows the same policy (probe, grow and rebuild on
 * NoSpace, settle, emit; the dictionary's counters move last): a call that ends in an error leaves the
 * dictionary as it was and attaches nothing.  Idempotent per (table, column, dictionary): a second
 * call returns the same index, launches nothing and adds no key.  strom_textdict_kernel_ns then holds this
 * call's kernels (the pass that turns slots into checked datum offsets is counted with the probe).
 *
 * One dictionary may encode several tables (supplier.nation and customer.nation as one domain) and
 * fact chunks as well; ids are stable once settled, so the dictionary may grow after the call and the
 * coded column stays valid.  An absent slot and a NULL datum both have id 0 and are NULL.
 *
 * -BadRequest before any launch: a NULL handle; a table that is not one relation with a DIRECT index
 * and unique keys, or lives on another device than the dictionary; a column index outside the
 * relation; the same (table, column) already coded under another living dictionary.  A column that is
 * not varlena is found by the kernel: -DataStoreCorruption.  A compressed or external datum in any
 * row: -CpuReCheck.
 *
 * THE DICTIONARY MUST OUTLIVE THE TABLE, unreset.  strom_textdict_reset and strom_textdict_release
 * end the dictionary's epoch: a fold that asks for a coded column made under an earlier epoch answers
 * BadRequest with nothing launched; the column may be encoded again (same index).
 */
int			strom_textdict_encode_table(strom_textdict *dict, strom_hashjoin_table *tbl, int colidx);

#ifdef __cplusplus
}
#endif

#endif	/* STROM_TEXTDICT_TABLE_H */
