/*
 * jvector_bq_delete.h — deleting nodes from a graph under construction over binary-quantized vectors: the deletion half of the
 * jv_bq_builder ABI.  jvector_bq_builder.h includes this file; either header gives the whole ABI.  Conventions are jvector_hip.h's.
 */
#ifndef JVECTOR_BQ_DELETE_H
#define JVECTOR_BQ_DELETE_H

#include "jvector_bq_builder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Deletions: GraphIndexBuilder.markNodeDeleted / removeDeletedNodes (B/graph/GraphIndexBuilder.java:678-799, FreshDiskANN's
 * consolidation) with Neighbors.replaceDeletedNeighbors (B/graph/ConcurrentNeighborMap.java:225-239), for the builder's one level.
 *   mark_deleted  : sets the marks of B nodes (host or device ids); marking twice is not an error.  A marked node stays an ordinary
 *                   node of the graph — inserts and improves see it, link to it and rewrite its row — until it is removed, as in the
 *                   reference (addGraphNode / improveConnections never look at the deleted set); jv_hip_bq_graph_search hides it
 *                   through live_bits.  JV_ERR_INVALID, the builder as it was: an id outside the rows, an id never seeded or inserted,
 *                   an id already removed.
 *   deleted_count : marked = nodes marked and not yet removed, removed = nodes removed so far (each nullable)
 *   live_bits     : ceil(n / 64) words, bit i of word i / 64 set = node i is in the graph and not marked: accept_bits of
 *                   jv_hip_bq_graph_search (accept_stride_words = 0)
 *   entry         : the node a search of the working graph starts from; -1: the graph is empty
 *   remove_deleted: removeDeletedNodes.  Rewrites the rows of the live nodes that have a marked neighbour, blanks the rows of the marked
 *                   nodes (ids -1, scores 0, diverseBefore 0), clears their marks and takes them out of the graph, lowers the node count
 *                   (counts5[2] of stats), moves the entry if it was removed.  counts4 (nullable) = {nodes removed, live rows rewritten,
 *                   candidates scored (distinct per node), rows that took the fallback}.  With nothing marked: JV_OK, nothing touched.
 *                   Its time is added to seconds3[2] of stats.  A removed id is never reused: seed / insert_batch / improve_batch /
 *                   mark_deleted of one is JV_ERR_INVALID.  Rows are not compacted, ids not renumbered.
 * The rules, where the reference leaves a choice open stated as one:
 *   1. Candidates of a live node i: the distinct live k != i in the rows of i's marked neighbours, rows as they are when the call starts.
 *   2. Candidate order: score 1 - (float) h / D of row i against row k, higher first, the smaller id on equal score (the reference
 *      inserts with insertSorted in the iteration order of a concurrent hash set; ascending id is this engine's order, and insertSorted
 *      puts an equal score behind the ones it finds).
 *   3. Survivors: i's unmarked entries, in stored order, under their stored scores.
 *   4. The list pruned is NodeArray.merge(survivors, candidates) (B/graph/NodeArray.java:63-143), its duplicate rule included: a node
 *      is added once per run of equal scores.
 *   5. Prune with diverseBefore = 0, the builder's alpha and maxDegree; the selection replaces the row, diverseBefore = its size.
 *   6. A live node without a marked neighbour is not touched: ids, score bits and mark stay as they are.
 *   7. Fallback, when rule 1 yields no candidate: 2 maxDegree draws r = splitmix64 % n from the state seed + id x 0x9E3779B97F4A7C15
 *      (jv_internal.h's splitmix64; the reference draws from ThreadLocalRandom); a marked r is drawn again, at most 64 times, and a draw
 *      still marked is skipped; a draw equal to i, drawn before, or not in the graph is skipped; maxDegree candidates end the loop.
 *      They go through rules 2 - 5.  The result is a function of (graph, marks, seed).
 *   8. New entry, only when the entry was removed: the smallest id in the graph and not marked; -1 if there is none (then seed again).
 *   9. Refused, never truncated: if the longest merged list (rule 4, exact, computed for every affected node before any row, bit or
 *      counter changes) exceeds jv_hip_bq_retain_diverse_max_candidates, the call is JV_ERR_UNSUPPORTED, the message names the node and
 *      both numbers, and the builder is as it was: remove in smaller sets.
 * Two runs over equal graphs, marks and seed are byte-identical: no atomic decides an order or a tie.  Not covered: deleting from a
 * finished jv_layered, id reuse, deletes concurrent with inserts. */
JV_API int jv_hip_bq_builder_mark_deleted(jv_ctx *ctx, jv_bq_builder *b, const int32_t *nodes, int B);
JV_API int jv_hip_bq_builder_deleted_count(const jv_bq_builder *b, int64_t *marked, int64_t *removed);
JV_API int jv_hip_bq_builder_live_bits(jv_ctx *ctx, jv_bq_builder *b, uint64_t *bits_out);
JV_API int jv_hip_bq_builder_remove_deleted(jv_ctx *ctx, jv_bq_builder *b, uint64_t seed, int64_t *counts4);
JV_API int32_t jv_hip_bq_builder_entry(const jv_bq_builder *b);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_BQ_DELETE_H */
