/*
 * jvector_bq_graph.h — graph search over binary-quantized vectors, on the device: BQVectors as the approximate score of
 * GraphSearcher.search, the way every other CompressedVectors of the reference is used.  Conventions are jvector_hip.h's.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/):
 *   GraphSearcher.search(DefaultSearchScoreProvider(bqv.scoreFunctionFor(query, vsf), exact reranker), topK, rerankK, 0, 0, acceptOrds)
 *   (B/graph/GraphSearcher.java:263-282, 334-369, 406-469): the queries are encoded with BinaryQuantization.encode; the entry node is
 *   scored; levels entry_level .. 1 run with rerankK = 1 and Bits.ALL, each handing its result (and what it evicted) to the next as
 *   candidates; level 0 runs with rerankK and the accept filter (a rejected node is traversed, never returned); the stop rule is a strict <.
 *   The approximate score is BQVectors.similarityBetween = 1 - (float) hamming / D in f32; `vsf` matters to the rerank only.
 */
#ifndef JVECTOR_BQ_GRAPH_H
#define JVECTOR_BQ_GRAPH_H

#include "jvector_bq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The graph `g` (built any way: jv_hip_graph_set_level / jv_hip_graph_set_level0_device / jv_hip_build_layered) searched with the rows
 * of `bq` as approximate scores.
 *   vectors != NULL: the approximate results (at most rerankK) are reranked with exact scores under `vsf` (the launchers of
 *     jv_hip_graph_search and jv_hip_bq_search_flat: the same bits) and the top topK come back in NodeQueue order (higher score
 *     first, ties to the smaller id).
 *   vectors == NULL: the approximate top topK with their BQ similarities.
 * A tail shorter than topK is (-1, -INFINITY).  stats (nullable, host memory): Q x 2 = {visitedCount, expandedCount} as the
 * reference counts them (the entry node is not a visit, every fresh neighbour is).
 * accept_bits (nullable, host or device): jv_hip_graph_search_filtered's layout — bit n of word n / 64 set = node n may be returned;
 * accept_stride_words = 0 one mask for the batch, else query q reads accept_bits + q * accept_stride_words (>= ceil(n_nodes / 64)).
 * queries (Q x D floats), out_ids / out_scores (Q x topK): host or device memory.
 * JV_ERR_INVALID: NULL handles or outputs, topK < 1, rerankK < topK, Q < 0, bq->D != vectors->D, bq->count < n_nodes,
 * vectors->count < n_nodes, no entry node set; Q == 0 returns JV_OK at once.  JV_ERR_UNSUPPORTED: a degree above 512, D above 16383,
 * rerankK above jv_hip_bq_graph_max_rerank_k, or a graph whose level 0 has neither host rows nor a device adjacency.
 * Nothing is truncated silently: a query that outgrows the kernel's fixed-size visited table or candidate storage is run again, in a
 * following launch, with a visited bitmap of n_nodes bits and candidate storage for every node; the results are identical.
 * Counters (jv_hip_ctx_get_stat): bq_gs_calls, bq_gs_queries, bq_gs_queries_retried.  Options (jv_hip_ctx_set_option):
 * bq_gs_vcap_log2 (log2 of the first attempt's visited table, 8..24), bq_gs_cand_cap (keys of the candidates' LDS tier, >= 128). */
JV_API int jv_hip_bq_graph_search(jv_ctx *ctx, const jv_graph *g, const jv_bq_vectors *bq, const jv_vectors *vectors,
                                  const float *queries, int Q, jv_vsf vsf, int topK, int rerankK,
                                  const uint64_t *accept_bits, int64_t accept_stride_words,
                                  int32_t *out_ids, float *out_scores, int64_t *stats);
/* largest rerankK the device kernel takes for this graph (its queues' LDS share); a larger one is JV_ERR_UNSUPPORTED */
JV_API int jv_hip_bq_graph_max_rerank_k(jv_ctx *ctx, const jv_graph *g, int *out);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_BQ_GRAPH_H */
