/*
 * jvector_flat_filtered.h — the flat PQ search under an accept filter: jv_hip_search_flat over the rows a `Bits acceptOrds` admits.
 * The accept masks are compacted to ascending ordinal lists on the device and only the listed rows are scored, so a selective
 * predicate costs what its accepted rows cost.  Includes jvector_hip.h; conventions are that header's.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/): GraphSearcher.search(..., Bits acceptOrds)
 * (B/graph/GraphSearcher.java) visits rejected nodes without returning them, so under a selective predicate its visitedCount grows
 * roughly as 1 / selectivity; callers then score the accepted ordinals by brute force with the PQ score function and rerank exactly.
 * This is that brute force: PQDecoder scores (ADC) of the accepted rows -> top rerankK in NodeQueue order -> exact rerank -> topK.
 */
#ifndef JVECTOR_FLAT_FILTERED_H
#define JVECTOR_FLAT_FILTERED_H

#include "jvector_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* jv_hip_search_flat with the mask layout of jv_hip_graph_search_filtered / jv_hip_bq_search_flat (N = rows of `codes`):
 *   - bit n of word n / 64 set: row n may be returned.  accept_stride_words = 0: one mask for the batch; else query q reads
 *     accept_bits + q * accept_stride_words, with accept_stride_words >= ceil(N / 64).  accept_bits is host or device memory.
 *   - Bits at and beyond N are ignored: the tail of the last word and any slack words of a wider stride may hold anything.
 *   - Rejected rows are never returned and do not count toward rerankK: the approximate top rerankK (top topK when vectors is NULL
 *     or rerankK is 0) is taken among the accepted rows only, higher score first, ties to the smaller id; the survivors are reranked
 *     exactly as jv_hip_search_flat reranks (the same launchers, the same bits; NVQ-backed jv_vectors included); id_base is added
 *     to every valid id.
 *   - Fewer accepted rows than topK leave a tail of (-1, -INFINITY); id_base does not touch the -1.
 *   - accept_bits == NULL: the call is jv_hip_search_flat (accepted_out, if given, receives N for every query).
 *   - accepted_out (nullable, Q int64, host memory): the accepted rows of each query; the shared count repeated when the stride is 0.
 *   - JV_ERR_INVALID: a NULL handle or output, topK < 1, rerankK < 0, rerankK < topK with a rerank, a negative stride, a non-zero
 *     stride below ceil(N / 64), a dimension or count mismatch with `vectors`.  Q == 0 returns JV_OK at once.  A k above what the
 *     top-k takes gives the status jv_hip_search_flat gives.  A refused call leaves the outputs untouched.
 *   - Results are a function of the arguments only: no atomic decides a position, and the chunking of the query batch (context
 *     option flat_acc_score_bytes, default 1 GiB of scores per chunk, never less than four queries) does not change them.
 *   - Two routes lead to the same ids and the same score bits.  The list route (above) suits a selective predicate.  The dense route
 *     suits a mask that accepts a good part of the rows, shared or per query: the rejected rows are taken out of jv_hip_search_flat's
 *     strided sample, the k_s-th best of what is left is the query's threshold, and one scan over all N rows reads the accept bits
 *     itself (a 64-bit word per wavefront and 64 rows) and appends the accepted rows that reach the threshold to a short list; no
 *     Q x L scores are written.  It wants M % 16 == 0, 16-byte aligned codes, Q >= 2 and jv_hip_search_flat's sample parameters
 *     (k_s <= 4096, S >= k_s).  Every query must end with min(k1, accepted) <= list length <= capacity, else the whole call runs
 *     the list route: the result is exact either way.
 *   - Options (jv_hip_ctx_set_option): flat_acc_dense — unset or 0: the dense route is taken where N >= 2^18, 64 k1 <= N and the
 *     sparsest mask of the batch accepts at least flat_acc_dense_pct percent of the rows; 1: wherever its requirements hold; -1: never.
 *     flat_acc_dense_pct — that gate; default 50 for a shared mask and 25 for per-query masks, 75 and 50 when M > 32 (the measured
 *     crossovers).  flat_acc_dense_r — rows per lane of the scan, 4 or 8; 0: chosen from the grid.
 *   - Counters (jv_hip_ctx_get_stat): flat_acc_calls, flat_acc_queries, flat_acc_rows (sum of the accepted rows over the queries),
 *     flat_acc_chunks (one on the dense route), flat_acc_generic (calls under a shared mask whose shape the multi-query list kernel
 *     does not take: M % 16 != 0), flat_acc_dense_calls (calls answered by the dense route), flat_acc_dense_fallbacks (calls that
 *     tried it, failed the list-length check and were answered by the list route). */
JV_API int jv_hip_search_flat_filtered(jv_ctx *ctx, jv_luts *luts, const jv_codes *codes, const jv_vectors *vectors,
                                       const float *queries, int Q, jv_vsf vsf, int topK, int rerankK,
                                       const uint64_t *accept_bits, int64_t accept_stride_words, int32_t id_base,
                                       int32_t *out_ids, float *out_scores, int64_t *accepted_out /* nullable, Q, host */);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_FLAT_FILTERED_H */
