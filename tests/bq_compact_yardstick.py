"""The yardstick of BQ compaction in plain numpy: AbstractGraphIndexWriter.sequentialRenumbering
(B/graph/disk/AbstractGraphIndexWriter.java:146-159) — the nodes in the graph get 0, 1, 2 ... in their old relative order — and the
working rows carried across it (include/jvector_bq_compact.h, rules 5 and 6).  No device, no product code."""
import numpy as np


def renumbering(present):
    """(old_to_new int32 [n], -1 where present is False; new_to_old int32 [live])"""
    present = np.asarray(present, bool)
    old_to_new = np.where(present, np.cumsum(present) - 1, -1).astype(np.int32)
    new_to_old = np.flatnonzero(present).astype(np.int32)
    return old_to_new, new_to_old


def compact_lists(ids, sc, db, present, capacity):
    """the expected rows of the compacted builder: (ids [capacity, R], score BITS as int32 [capacity, R], diverseBefore [capacity]).
    New row r is old row new_to_old[r] with every id >= 0 sent through old_to_new; rows at and beyond live are blank.  `sc` may be
    float32 or its bits as int32."""
    old_to_new, new_to_old = renumbering(present)
    live, R = len(new_to_old), ids.shape[1]
    assert capacity >= live
    bits = np.ascontiguousarray(sc).view(np.int32)
    out_ids = np.full((capacity, R), -1, np.int32)
    out_sc = np.zeros((capacity, R), np.int32)
    out_db = np.zeros(capacity, np.int32)
    rows = ids[new_to_old]
    out_ids[:live] = np.where(rows >= 0, old_to_new[np.maximum(rows, 0)], rows)
    out_sc[:live] = bits[new_to_old]
    out_db[:live] = db[new_to_old]
    return out_ids, out_sc, out_db
