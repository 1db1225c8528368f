"""
The model of the unmatched pass of a RIGHT / FULL join (include/strom_hip.h, "RIGHT and FULL joins"),
on top of the nested-loop model of tests/join_model.py, which is imported unchanged.

The tracked relation is the LAST one of the program.  An entry of it is matched when some record of
some chunk fed to the table holds it in that relation's slot; the unmatched pass returns every other
entry -- an entry with a NULL key among them, since it can never be in a record:

    unmatched row ids = all row ids of the relation - the row ids join_model(..) puts into its slot

A device record of the pass is (0, .., 0, entry offset): word 0 == 0 means "no outer row", every
relation but the last has "no entry".  Both sides are compared as sets of row ids.
"""
import numpy as np

import join_model as jm


def matched_rowids(feeds):
    """feeds: [(outer rows of one chunk, the model's Rels for that chunk)] -> the sorted row ids of the
    last relation that the records of those chunks hold"""
    seen = [np.zeros(0, dtype=np.int64)]
    for rows, rels in feeds:
        slot = jm.join_model(rows, rels)[:, -1]
        seen.append(slot[slot >= 0])
    return np.unique(np.concatenate(seen))


def unmatched_rowids(nrows, feeds):
    """the row ids of the tracked (last) relation, nrows entries, that the unmatched pass returns
    after the chunks `feeds` (see matched_rowids)"""
    return np.setdiff1d(np.arange(nrows, dtype=np.int64), matched_rowids(feeds))


def unmatched_from_records(recs):
    """the same from records the model made itself (join_model over every chunk), for callers that
    keep them"""
    slot = np.asarray(recs)[:, -1]
    return slot[slot >= 0]


def device_unmatched_rowids(device_kmhash, records):
    """records of the unmatched pass -> sorted row ids; every word but the last must be 0, and no
    entry comes twice"""
    records = np.asarray(records)
    if len(records) == 0:
        return np.zeros(0, dtype=np.int64)
    assert not records[:, :-1].any(), "an unmatched record names an outer row or another relation's entry"
    assert (records[:, -1] != 0).all(), "an unmatched record without an entry"
    ids = jm.records_to_rowids(device_kmhash, records)[:, -1]
    out = np.sort(ids)
    assert len(np.unique(out)) == len(out), "an entry was emitted twice"
    return out
