/*
 * jvector_nvq_flat.h — the NVQ flat search: the nearest neighbours of a query batch among the NVQ rows an accept filter admits, in
 * one call.  The brute-force search of a deployment that keeps only NVQ rows on the device (a FUSED_PQ + NVQ_VECTORS index): what it
 * falls back to for a small segment or a very selective predicate, and the ground truth of its own recall numbers.  Includes
 * jvector_hip.h; conventions are that header's.
 *
 * Before this call the recipe was jv_hip_nvq_scores over every ordinal into a Q x N score matrix plus a top-k, which de-quantises
 * every byte once per query.  Here a tile kernel de-quantises a chunk of 128 rows once and scores it against 128 queries through
 * MFMA.
 */
#ifndef JVECTOR_NVQ_FLAT_H
#define JVECTOR_NVQ_FLAT_H

#include "jvector_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N = rows of `nv`, D and S = dimension and sub-vectors of its NVQuantization.  The contract is jv_hip_search_exact's
 * (jvector_exact_flat.h) point for point, over NVQ rows:
 *   - Step 1 scores every accepted row against every query with the tile arithmetic below and takes, per query, the top candK in
 *     NodeQueue order: higher score first, ties to the smaller id.  candK == 0: the top topK of that order, with those scores, is the
 *     result and step 2 is skipped.
 *   - Step 2 (candK >= topK): the candK candidates are rescored by the kernel behind jv_hip_nvq_scores — the reference's NVQScorer,
 *     bit for bit — and the top topK by jv_hip_topk is returned: the launchers jv_hip_search_flat uses over a jv_vectors made by
 *     jv_hip_vectors_from_nvq, the same bits.
 *   - Tile arithmetic of step 1.  val[k] is the de-quantised value of byte k of the row: scaledLogitFunctionNQT with the reference's
 *     bits, from the derived numbers of the sub-vector k falls in (sub-vector s covers D / S dimensions, the first D % S one more).
 *     The query side is NVQScorer's: qaux[q] = VectorUtil.dotProduct(query, globalMean) for DOT_PRODUCT, (float)sqrt(dotProduct(query,
 *     query)) for COSINE; EUCLIDEAN scores qwork = query - globalMean.  dot is ONE k-ascending fmaf chain from +0 over the whole row,
 *     acc = fmaf(a[k], b[k], acc) — NVQScorer restarts its chain at every sub-vector and adds the parts; that is the only difference,
 *     it is of f32 round-off class, and step 2 removes it.
 *         DOT_PRODUCT  a = query, b = val            score = (1 + dot + qaux[q]) / 2
 *         EUCLIDEAN    a = qwork, b = val            d2 = fmaf(-2, dot, qn + vn) clamped at 0, score = 1 / (1 + d2); qn and vn are
 *                                                    the k-ascending fmaf chains of a[k]^2 and b[k]^2
 *         COSINE       a = query, b = val[k] + globalMean[k]
 *                                                    score = (1 + (dot / qaux[q]) / (float)sqrt((double)cosnorm[row])) / 2, cosnorm
 *                                                    the row's squared-normalisation sum as jv_hip_nvq_scores computes it
 *   - The mask is that of jv_hip_search_exact: bit n of word n / 64 set: row n may be returned.  accept_stride_words = 0: one mask for
 *     the batch; else query q reads accept_bits + q * accept_stride_words, with accept_stride_words >= ceil(N / 64).  accept_bits is
 *     host or device memory.  Bits at and beyond N are ignored: the tail of the last word and any slack words of a wider stride may
 *     hold anything.  accept_bits == NULL: no filter.  Rejected rows are never returned and do not count toward candK.  Fewer accepted
 *     rows than topK leave a tail of (-1, -INFINITY).  id_base is added to valid ids only.
 *   - JV_ERR_INVALID: a NULL handle or output, topK < 1, candK < 0, 0 < candK < topK, a negative stride, a non-zero stride below
 *     ceil(N / 64), Q < 0, an unknown similarity function, rows on another device than the context's.  Q == 0 returns JV_OK at once.
 *     A candK (or topK) above what the top-k takes gives that launcher's status.  A refused call leaves the outputs untouched.
 *   - Results are a function of the arguments only: an atomic decides a position in a candidate list, never a result, and neither
 *     the route nor the chunking of the queries changes an id or a score bit.
 *   - Two routes, as in jv_hip_search_exact.  The fused route: a sample pass scores every g-th tile of 128 rows into a Q x S matrix
 *     whose kc-th best per query (kc = candK ? candK : topK) is a threshold at least kc accepted rows reach; a select pass scores all
 *     rows and appends the accepted rows that reach the threshold to a list of `cap` entries per query; a device-side check of the
 *     list lengths; the top kc of the lists.  If a list overflowed, the whole call runs the chunked route: the same kernel storing
 *     every score of a chunk of rows, -1 ids for the rejected columns, a top-k per chunk and a merge.
 *   - Options (jv_hip_ctx_set_option), with the meanings and defaults of their exact_flat_* counterparts: nvq_flat_fused — unset or 0:
 *     the fused route where N >= 65536; 1: wherever N > 0; -1: never.  nvq_flat_sample_stride — g, in tiles of 128 rows; 0 (default):
 *     16, more where that keeps the sample at 2^18 rows.  nvq_flat_cap — list entries per query; 0 (default): 4 kc g rounded up to
 *     64.  nvq_flat_score_bytes — default 1 GiB: the queries run in chunks whose sample matrix and lists (fused route) or score and
 *     id matrix (chunked route) stay under it.
 *   - Counters (jv_hip_ctx_get_stat): nvq_flat_calls, nvq_flat_fused_calls (answered by the fused route), nvq_flat_fallbacks (tried
 *     it, failed the list-length check, answered by the chunked route), nvq_flat_listed (sum of the list lengths of the select
 *     passes). */
JV_API int jv_hip_nvq_search_flat(jv_ctx *ctx, const jv_nvq_vectors *nv, const float *queries, int Q, jv_vsf vsf, int topK, int candK,
                                  const uint64_t *accept_bits, int64_t accept_stride_words, int32_t id_base, int32_t *out_ids,
                                  float *out_scores);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_NVQ_FLAT_H */
