/*
 * jvector_bq_builder.h — graph construction from binary-quantized vectors alone, on the device: GraphIndexBuilder driven by
 * BuildScoreProvider.bqBuildScoreProvider(BQVectors).  No codebook, no training, no full-resolution vectors: a jv_bq_vectors is all a
 * build takes, and what comes out is searched by jv_hip_bq_graph_search.  Conventions are jvector_hip.h's.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/):
 *   B/graph/GraphIndexBuilder.java:605-659  addGraphNode; :510-560 improveConnections; :472-508 cleanup -> enforceDegree
 *   B/graph/ConcurrentNeighborMap.java:104-163,190-200,222-322  insertDiverse / backlink / Neighbors.insert / enforceDegree
 *   B/graph/similarity/BuildScoreProvider.java:214-258  bqBuildScoreProvider: one score, 1 - (float) hamming / D, for the search, the
 *     back link and the diversity test
 *
 * The entry points mirror jv_hip_builder_* (jvector_hip.h) one to one with (pq, codes, vectors, vsf) replaced by `bq`, and every call
 * means what it means there.  What differs is the list discipline: there is ONE, the reference's.  similarityBetween is symmetric, so the
 * score a search gives a neighbour is the score its back link is stored under and the score the prune tests against: every entry keeps
 * the score it was inserted under, lists stay in NodeArray order and keep ConcurrentNeighborMap's diverseBefore mark, and nothing is ever
 * re-scored or re-sorted (jv_hip_builder_*'s REFERENCE ORDER; the context options bl_ref_order / bl_sorted_lists are not read).
 *   create       : nodes = the rows of `bq`.  The working adjacency is count x R int32 with R = max(maxDegree, min(64, (int) (maxDegree x
 *                  neighborOverflow))), device memory owned by the builder.
 *   seed         : the first node
 *   insert_batch : B concurrent addGraphNode calls that do not see each other: jv_hip_bq_graph_search_nodes (topK = beamWidth) over the
 *                  graph so far, jv_hip_bq_retain_diverse over the result lists, insertDiverse on the new rows, back links in batch order
 *                  through Neighbors.insert; a list that outgrows (int) (neighborOverflow x maxDegree) goes back through
 *                  jv_hip_bq_retain_diverse with its stored scores and its diverseBefore mark.
 *   improve_batch: improveConnections for nodes IN the graph: the search with exclude_self, merged with the node's row, pruned, linked
 *                  back.  The three deviations of jv_hip_builder_improve_batch: ids de-duplicated, the node's own row as the query,
 *                  sorted candidates.
 *   finish       : enforceDegree on every row; neighbors_out (nullable; host or device) receives count x maxDegree int32, rows packed,
 *                  -1 padded.
 *   stats        : seconds3 / counts5 as jv_hip_builder_stats
 *   working_lists: ids_out [count x R] (-1 padded), scores_out [count x R], diverse_before_out [count]; each nullable, host or device
 *   neighbors_device : the working adjacency in place (row width in *row_width)
 * With ONE node per batch this is addGraphNode operation for operation: ids, order, score bits and marks equal the reference's
 * one-thread build, and so does the adjacency after finish (the limits of that claim are jv_hip_builder_working_lists's: no
 * re-inserts, maxDegree x overflow <= 64).  With larger batches the result depends on the insertion order and the batch boundaries
 * only: no atomic decides an edge.
 *
 * JV_ERR_INVALID: NULL arguments, maxDegree outside 2..64, beamWidth outside 1..4096, alpha outside [1, 64], neighborOverflow outside
 * [1, 8], more than 2^31 - 1 rows; a batch id outside the rows or listed twice; insert before seed.  JV_ERR_UNSUPPORTED: D > 16383;
 * beamWidth above jv_hip_bq_graph_max_rerank_k; max(beamWidth + R, 3 R) above jv_hip_bq_retain_diverse_max_candidates for these rows —
 * a list is never truncated to fit.  A refused call leaves the builder as it was.
 */
#ifndef JVECTOR_BQ_BUILDER_H
#define JVECTOR_BQ_BUILDER_H

#include "jvector_bq_build.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jv_bq_builder jv_bq_builder;
JV_API int jv_hip_bq_builder_create(jv_ctx *ctx, const jv_bq_vectors *bq, int max_degree, int beam_width, float alpha,
                                    float neighbor_overflow, jv_bq_builder **out);
JV_API int jv_hip_bq_builder_seed(jv_ctx *ctx, jv_bq_builder *b, int32_t node);
JV_API int jv_hip_bq_builder_insert_batch(jv_ctx *ctx, jv_bq_builder *b, const int32_t *nodes, int B);
JV_API int jv_hip_bq_builder_improve_batch(jv_ctx *ctx, jv_bq_builder *b, const int32_t *nodes, int B);
JV_API int jv_hip_bq_builder_finish(jv_ctx *ctx, jv_bq_builder *b, int32_t *neighbors_out);
JV_API int jv_hip_bq_builder_stats(const jv_bq_builder *b, double *seconds3, int64_t *counts5);
JV_API int jv_hip_bq_builder_working_lists(jv_ctx *ctx, const jv_bq_builder *b, int32_t *ids_out, float *scores_out,
                                           int32_t *diverse_before_out);
JV_API const int32_t *jv_hip_bq_builder_neighbors_device(const jv_bq_builder *b, int *row_width);
JV_API int jv_hip_bq_builder_destroy(jv_bq_builder *b);

/* The whole LAYERED build in one call, jv_hip_build_layered's contract: levels from the same splitmix64 draw seeded with `seed`, levels
 * with fewer than min_top nodes folded into the one below; every level a jv_bq_builder of its own — level 0 over `bq`, a level >= 1 over
 * a compacted copy of its members' rows, ids mapped back to global ones — with inserts in a seeded order in prefix-doubling batches of
 * at most max_batch, then improve_passes (0..8) passes of improve_batch over every node of the level, then enforceDegree.  Entry point:
 * the member of the top level at minimum Hamming distance to the top level's bitwise-majority row (bit b set iff strictly more than
 * half of the members have it set), ties to the smaller id; a graph of one level is entered where its construction started.
 * A function of (rows, parameters, seed) only.  The result is read and released through jv_hip_layered_info / _level / _stats /
 * _level0_device / _destroy (jvector_hip.h). */
JV_API int jv_hip_bq_build_layered(jv_ctx *ctx, const jv_bq_vectors *bq, int max_degree, int beam_width, float alpha,
                                   float neighbor_overflow, int max_batch, int improve_passes, uint64_t seed, int min_top,
                                   jv_layered **out);

#ifdef __cplusplus
}
#endif

#include "jvector_bq_delete.h" /* mark_deleted / remove_deleted and their companions: the deletion half of this ABI */

#endif /* JVECTOR_BQ_BUILDER_H */
