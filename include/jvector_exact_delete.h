/*
 * jvector_exact_delete.h — deleting nodes from a graph under construction over float rows: the deletion half of the jv_exact_builder
 * ABI.  Includes jvector_exact_builder.h.  Conventions are jvector_hip.h's.
 */
#ifndef JVECTOR_EXACT_DELETE_H
#define JVECTOR_EXACT_DELETE_H

#include "jvector_exact_builder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Deletions: GraphIndexBuilder.markNodeDeleted / removeDeletedNodes (B/graph/GraphIndexBuilder.java:678-799, FreshDiskANN's
 * consolidation) with Neighbors.replaceDeletedNeighbors (B/graph/ConcurrentNeighborMap.java:225-239), for the builder's one level.
 * The five entry points mirror jv_hip_bq_builder_mark_deleted / _deleted_count / _live_bits / _remove_deleted / _entry
 * (jvector_bq_delete.h) one to one with `bq` replaced by the builder's (vectors, vsf); every call means what its twin means:
 *   mark_deleted  : sets the marks of B nodes (host or device ids); marking twice is not an error.  A marked node stays an ordinary
 *                   node of the graph — inserts and improves see it, link to it and rewrite its row — until it is removed;
 *                   jv_hip_exact_graph_search hides it through live_bits.  JV_ERR_INVALID, the builder as it was: an id outside the
 *                   rows, an id never seeded or inserted, an id already removed.
 *   deleted_count : marked = nodes marked and not yet removed, removed = nodes removed so far (each nullable)
 *   live_bits     : ceil(n / 64) words, bit i of word i / 64 set = node i is in the graph and not marked: accept_bits of
 *                   jv_hip_exact_graph_search (accept_stride_words = 0)
 *   entry         : the node a search of the working graph starts from; -1: the graph is empty
 *   remove_deleted: removeDeletedNodes.  Rewrites the rows of the live nodes that have a marked neighbour, blanks the rows of the marked
 *                   nodes (ids -1, scores 0, diverseBefore 0), clears their marks and takes them out of the graph, lowers the node count
 *                   (counts5[2] of stats), moves the entry if it was removed.  counts4 (nullable) = {nodes removed, live rows rewritten,
 *                   candidates scored (distinct per node), rows that took the fallback}.  With nothing marked: JV_OK, nothing touched.
 *                   Its time is added to seconds3[2] of stats.  A removed id is never reused: seed / insert_batch / improve_batch /
 *                   mark_deleted of one is JV_ERR_INVALID.  Rows are not compacted, ids not renumbered.
 * Rules 1 - 9 of jvector_bq_delete.h hold word for word, with two substitutions:
 *   2. Candidate order: score compare(v[i], v[k]) under the builder's similarity, with the bits of
 *      jv_hip_exact_pair_scores(node1 = i, node2 = k); higher first, the smaller id on equal score.
 *   9. Refused, never truncated: if the longest merged list (rule 4, exact, computed for every affected node before any row, bit or
 *      counter changes) exceeds jv_hip_exact_retain_diverse_max_candidates at the builder's maxDegree, the call is JV_ERR_UNSUPPORTED,
 *      the message names the node and both numbers, and the builder is as it was: remove in smaller sets.
 * Rows are assumed to give non-NaN scores, as everywhere in the builder.  Two runs over equal graphs, marks and seed are
 * byte-identical: no atomic decides an order or a tie.  Not covered: compacting or renumbering an exact builder, deleting from a
 * finished jv_layered, id reuse, deletes concurrent with inserts. */
JV_API int jv_hip_exact_builder_mark_deleted(jv_ctx *ctx, jv_exact_builder *b, const int32_t *nodes, int B);
JV_API int jv_hip_exact_builder_deleted_count(const jv_exact_builder *b, int64_t *marked, int64_t *removed);
JV_API int jv_hip_exact_builder_live_bits(jv_ctx *ctx, jv_exact_builder *b, uint64_t *bits_out);
JV_API int jv_hip_exact_builder_remove_deleted(jv_ctx *ctx, jv_exact_builder *b, uint64_t seed, int64_t *counts4);
JV_API int32_t jv_hip_exact_builder_entry(const jv_exact_builder *b);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_EXACT_DELETE_H */
