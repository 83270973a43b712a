/*
 * jvector_nvq_graph.h — graph search scored on NVQ rows alone, on the device: one byte per dimension plus four floats per sub-vector,
 * no float rows, no other quantizer.  The search of an index that keeps NVQVectors as its CompressedVectors.  Conventions are
 * jvector_hip.h's.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/):
 *   GraphSearcher.search(DefaultSearchScoreProvider(NVQVectors.scoreFunctionFor(query, vsf)), topK, rerankK = beamK, 0, 0, acceptOrds)
 *   (B/graph/GraphSearcher.java:263-282, 334-369, 406-469; B/quantization/NVQVectors.java:100-109, NVQScorer.java:33-137): the entry
 *   node is scored; levels entry_level .. 1 run with a result list of 1 and Bits.ALL, each handing its result (and what it evicted) to
 *   the next as candidates; level 0 keeps beamK results under the accept filter (a rejected node is traversed, never returned); the stop
 *   rule is a strict <.  The score function is NVQScorer's similarityTo on the compressed row and there is no reranker, so the result is
 *   the first topK of the beamK kept, in NodeQueue order (higher score first, ties to the smaller id).  As in the reference at
 *   threshold 0, a node whose score is negative is traversed but not kept.
 */
#ifndef JVECTOR_NVQ_GRAPH_H
#define JVECTOR_NVQ_GRAPH_H

#include "jvector_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The graph `g` (built any way: jv_hip_graph_set_level / jv_hip_graph_set_level0_device / jv_hip_build_layered) searched with the NVQ
 * rows `nv` under `vsf`.  Scores carry the bits of jv_hip_nvq_scores; the walk is steered by them, so the visit order is the
 * reference's over the same rows.
 * beamK == 0 means beamK = topK.  A tail shorter than topK is (-1, -INFINITY).  stats (nullable, host memory): Q x 2 =
 * {visitedCount, expandedCount} as the reference counts them (the entry node is not a visit, every fresh neighbour is).
 * accept_bits (nullable, host or device): jv_hip_graph_search_filtered's layout — bit n of word n / 64 set = node n may be returned;
 * accept_stride_words = 0 one mask for the batch, else query q reads accept_bits + q * accept_stride_words (>= ceil(n_nodes / 64)).
 * queries (Q x D floats), out_ids / out_scores (Q x topK): host or device memory.
 * JV_ERR_INVALID: NULL handles or outputs, topK < 1, beamK < topK (beamK != 0), Q < 0, nv->count < n_nodes, no entry node set, a
 * stride smaller than one mask, an unknown vsf; Q == 0 returns JV_OK at once.  JV_ERR_UNSUPPORTED: a degree above 512, beamK above
 * jv_hip_nvq_graph_max_beam_k, a graph whose level 0 has neither host rows nor a device adjacency.  A refused call leaves the outputs
 * untouched.
 * Nothing is truncated silently: a query that outgrows the kernel's fixed-size visited table or candidate storage is run again, in a
 * following launch, with a visited bitmap of n_nodes bits and candidate storage for every node; the results are identical.
 * There is no node-seeded variant and no robust prune over these rows: the reference's NVQVectors.diversityFunctionFor throws.
 * Counters (jv_hip_ctx_get_stat): nvq_gs_calls, nvq_gs_queries, nvq_gs_queries_retried.  Options (jv_hip_ctx_set_option):
 * nvq_gs_vcap_log2 (log2 of the first attempt's visited table, 8..24), nvq_gs_cand_cap (keys of the candidates' LDS tier, >= 128). */
JV_API int jv_hip_nvq_graph_search(jv_ctx *ctx, const jv_graph *g, const jv_nvq_vectors *nv,
                                   const float *queries, int Q, jv_vsf vsf, int topK, int beamK,
                                   const uint64_t *accept_bits, int64_t accept_stride_words,
                                   int32_t *out_ids, float *out_scores, int64_t *stats);
/* largest beamK the device kernel takes for this graph (the result list's share of the kernel's LDS block — the exact-score walk's);
 * a larger one is JV_ERR_UNSUPPORTED */
JV_API int jv_hip_nvq_graph_max_beam_k(jv_ctx *ctx, const jv_graph *g, int *out);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_NVQ_GRAPH_H */
