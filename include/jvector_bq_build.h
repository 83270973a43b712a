/*
 * jvector_bq_build.h — build-time scoring over binary-quantized vectors, on the device: the two places graph construction calls
 * BuildScoreProvider.bqBuildScoreProvider(BQVectors) once per inserted node, batched.  Conventions are jvector_hip.h's.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/):
 *   B/graph/similarity/BuildScoreProvider.java:214-258  bqBuildScoreProvider: searchProviderFor(node1) and
 *     diversityScoreFunctionFor(node1) both score BQVectors.similarityBetween(row(node1), row(n)) = 1 - (float) hamming / D; no rerank.
 *   B/graph/diversity/VamanaDiversityProvider.java:45-96  retainDiverse / isDiverse, the robust prune.
 * The pair scores themselves are jv_hip_bq_pair_scores (jvector_bq.h).  The builder that drives these calls is jvector_bq_builder.h.
 */
#ifndef JVECTOR_BQ_BUILD_H
#define JVECTOR_BQ_BUILD_H

#include "jvector_bq_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* retainDiverse for P nodes at once, scored row against row.  The argument and output contract is jv_hip_retain_diverse's
 * (jvector_hip.h) with the pair table and the codes replaced by `bq`:
 *   node p's NodeArray is cand_nodes / cand_scores[p * C .. p * C + cand_count[p]) (cand_count NULL: C entries each; a count is
 *   clamped to [0, C]); diverse_before (nullable, default 0): that many leading entries are taken as already diverse.
 *   selected_out: P x maxDegree candidate POSITIONS in ascending order, -1 padded.  n_selected_out: P.  short_edges_out (nullable):
 *   nSelected / (float) maxDegree after the alpha = 1 round, NaN if the loop never ran.
 * Exactly the reference's arithmetic: the first min(diverse_before, maxDegree) positions are set and nSelected starts at
 * diverse_before; currentAlpha is an f32 from 1.0f in steps of += 0.2f, the loop bound currentAlpha <= alpha + 1E-6 is evaluated
 * in double (an alpha below 1, or NaN, means no round at all; an alpha above 64, +INFINITY included, is refused as in
 * jv_hip_retain_diverse: the rounds are a loop on the device); a candidate is tested against the selected positions in ascending order
 * and the test ends at the first position holding the candidate's own id (diverse); it is not diverse when
 * 1 - (float) h / D > cand_scores[i] * currentAlpha, both sides f32, strictly.  A pair with an ordinal outside [0, count of bq)
 * has similarity -INFINITY, as in jv_hip_bq_pair_scores.  Scores need not be sorted or finite.
 * All buffers: host or device memory.
 * JV_ERR_INVALID: NULL handles or outputs, P < 0, C < 1, maxDegree < 1, alpha > 64; P == 0 returns JV_OK at once.  JV_ERR_UNSUPPORTED:
 * maxDegree > 64, D > 16383, C above jv_hip_bq_retain_diverse_max_candidates. */
JV_API int jv_hip_bq_retain_diverse(jv_ctx *ctx, const jv_bq_vectors *bq, int P, int C,
                                    const int32_t *cand_nodes, const float *cand_scores, const int32_t *cand_count,
                                    const int32_t *diverse_before, int maxDegree, float alpha,
                                    int32_t *selected_out, int32_t *n_selected_out, float *short_edges_out);
/* largest C jv_hip_bq_retain_diverse takes for these rows: one node's candidate rows and selected rows share the kernel's LDS
 * block (0: rows too wide for any list) */
JV_API int jv_hip_bq_retain_diverse_max_candidates(jv_ctx *ctx, const jv_bq_vectors *bq, int maxDegree, int *out);

/* GraphSearcher.search(bqBuildScoreProvider.searchProviderFor(nodes[q]), topK, topK, 0, 0, Bits.ALL) for Q nodes: the query words of
 * item q are row nodes[q] of `bq`, gathered on the device; the walk is jv_hip_bq_graph_search's, its second pass for queries that
 * outgrow the first attempt's structures, its counters and its options included.  out_ids / out_scores (Q x topK, host or device):
 * the approximate top topK with their BQ similarities in NodeQueue order, the tail (-1, -INFINITY).  stats (nullable, host): Q x 2 =
 * {visitedCount, expandedCount}.  `nodes` (host or device) may name an ordinal more than once.
 * exclude_self != 0: node nodes[q] is traversed but never returned to item q (it still counts as visited and expanded) — the
 * accept mask of item q with that one bit cleared; what an improve pass over a node already in the graph needs.
 * JV_ERR_INVALID: an ordinal outside [0, count of bq) in HOST `nodes`; in device memory the ordinals are not brought back to be
 * looked at: such an item's row comes back as (-1, -INFINITY) with zero counters.  It is blanked AFTER the walk: the item still
 * runs a search from zero query words, so it costs what any item costs and it is counted in the context's bq_gs_queries (and in
 * bq_gs_queries_retried if that walk needed the second pass).  Every other check is jv_hip_bq_graph_search's. */
JV_API int jv_hip_bq_graph_search_nodes(jv_ctx *ctx, const jv_graph *g, const jv_bq_vectors *bq, const int32_t *nodes, int Q,
                                        int topK, int exclude_self, int32_t *out_ids, float *out_scores, int64_t *stats);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_BQ_BUILD_H */
