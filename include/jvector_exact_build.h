/*
 * jvector_exact_build.h — build-time scoring over the float rows themselves, on the device: the two places graph construction calls
 * BuildScoreProvider.randomAccessScoreProvider once per inserted node, batched.  The exact twin of jvector_bq_build.h.  Conventions
 * are jvector_hip.h's.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/):
 *   B/graph/similarity/BuildScoreProvider.java:106-160  randomAccessScoreProvider: searchProviderFor(node1) and
 *     diversityScoreFunctionFor(node1) both score VectorSimilarityFunction.compare(vectors[node1], vectors[n]); no quantizer, no rerank.
 *   B/graph/diversity/VamanaDiversityProvider.java:45-96  retainDiverse / isDiverse, the robust prune.
 * The pair scores themselves are jv_hip_exact_pair_scores (jvector_hip.h); the plain walk is jv_hip_exact_graph_search
 * (jvector_exact_graph.h).
 */
#ifndef JVECTOR_EXACT_BUILD_H
#define JVECTOR_EXACT_BUILD_H

#include "jvector_exact_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* retainDiverse for P nodes at once, scored float row against float row under `vsf`.  The argument and output contract is
 * jv_hip_bq_retain_diverse's (jvector_bq_build.h) with `bq` replaced by (vectors, vsf):
 *   node p's NodeArray is cand_nodes / cand_scores[p * C .. p * C + cand_count[p]) (cand_count NULL: C entries each; a count is
 *   clamped to [0, C]); diverse_before (nullable, default 0): that many leading entries are taken as already diverse.
 *   selected_out: P x maxDegree candidate POSITIONS in ascending order, -1 padded.  n_selected_out: P.  short_edges_out (nullable):
 *   nSelected / (float) maxDegree after the alpha = 1 round, NaN if the loop never ran.
 * Exactly the reference's arithmetic: the first min(diverse_before, maxDegree) positions are set and nSelected starts at
 * diverse_before, even above maxDegree; currentAlpha is an f32 from 1.0f in steps of += 0.2f, the loop bound
 * currentAlpha <= alpha + 1E-6 is evaluated in double (an alpha below 1, or NaN, means no round at all; an alpha above 64, +INFINITY
 * included, is refused: the rounds are a loop on the device); a candidate is tested against the selected positions in ascending
 * order and the test ends at the first position holding the candidate's own id (diverse); it is not diverse when
 * pair(cand, other) > cand_scores[i] * currentAlpha, both sides f32, strictly.
 * pair(a, b) carries the bits of jv_hip_exact_pair_scores(node1 = a, node2 = b): the non-fused chains of DefaultVectorUtilSupport in
 * the reference's association order and VectorSimilarityFunction.compare's finish.  The kernel runs the chain with the operand
 * roles SWAPPED (the selected row is the wave-uniform operand, the candidate's row the lane's): every product a[i] * b[i] commutes,
 * L2's differences a[i] - b[i] and b[i] - a[i] are exact negations with one square, cosine's two norms meet in one commutative f32
 * product, and the order of the additions over i is the same — identical bits for the three similarities (csrc/xb_body.h).
 * An ordinal outside [0, count of vectors) on either side gives pair = -INFINITY.  Scores need not be sorted or finite.
 * All buffers: host or device memory.  Selections are a function of the arguments only: no atomic decides anything.
 * JV_ERR_INVALID: NULL handles or outputs, P < 0, C < 1, maxDegree < 1, alpha > 64; P == 0 returns JV_OK at once.  JV_ERR_UNSUPPORTED:
 * maxDegree > 64, a `vectors` made by jv_hip_vectors_from_nvq, C above jv_hip_exact_retain_diverse_max_candidates.  A refused call
 * leaves the outputs untouched.  Counters (jv_hip_ctx_get_stat): exact_retain_calls, exact_retain_nodes. */
JV_API int jv_hip_exact_retain_diverse(jv_ctx *ctx, const jv_vectors *vectors, jv_vsf vsf, int P, int C,
                                       const int32_t *cand_nodes, const float *cand_scores, const int32_t *cand_count,
                                       const int32_t *diverse_before, int maxDegree, float alpha,
                                       int32_t *selected_out, int32_t *n_selected_out, float *short_edges_out);
/* largest C jv_hip_exact_retain_diverse takes at this maxDegree: the pair-score matrix [min(maxDegree, C)][C rounded up to 64] shares
 * the kernel's LDS block with one 64 x 64 row tile and four words per candidate; the rows themselves stay in device memory, so D does
 * not lower it.  A multiple of 64, at most 2048; 0 for maxDegree > 64 or when not even 64 candidates fit. */
JV_API int jv_hip_exact_retain_diverse_max_candidates(jv_ctx *ctx, const jv_vectors *vectors, int maxDegree, int *out);

/* GraphSearcher.search(randomAccessScoreProvider.searchProviderFor(nodes[q]), topK, beamK, 0, 0, Bits.ALL) for Q nodes:
 * jv_hip_exact_graph_search with row nodes[q] of `vectors` as query q and no accept mask.  The rows are gathered on the device;
 * `nodes` in device memory never travels to the host.  `nodes` (host or device) may name an ordinal more than once.
 * exclude_self != 0: node nodes[q] is traversed, visited and expanded as ever but never returned to item q — what an improve pass
 * over a node already in the graph needs.  The kernel compares the popped node with one id per query; no mask is built.
 * JV_ERR_INVALID: an ordinal outside [0, count of vectors) in HOST `nodes`; in device memory the ordinals are not brought back to be
 * looked at: such an item's row comes back as (-1, -INFINITY) with zero counters.  It is blanked AFTER the walk: the item still
 * runs a search from a zero query, so it costs what any item costs and it is counted in exact_gs_queries.  Every other check, the
 * second pass for items that outgrow the first attempt's structures, the options and the counters are jv_hip_exact_graph_search's. */
JV_API int jv_hip_exact_graph_search_nodes(jv_ctx *ctx, const jv_graph *g, const jv_vectors *vectors, const int32_t *nodes, int Q,
                                           jv_vsf vsf, int topK, int beamK, int exclude_self,
                                           int32_t *out_ids, float *out_scores, int64_t *stats);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_EXACT_BUILD_H */
