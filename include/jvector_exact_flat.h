/*
 * jvector_exact_flat.h — the exact flat search: the true nearest neighbours of a query batch among the float rows an accept filter
 * admits, in one call.  What a caller falls back to for a small segment or a very selective predicate, and the ground truth every
 * recall number is measured against.  Includes jvector_hip.h; conventions are that header's.
 *
 * Before this call the recipe was a host loop: jv_hip_exact_scan_dense into a Q x chunk score matrix, jv_hip_topk per chunk, a merge,
 * jv_hip_exact_scores over the candidates and a last jv_hip_topk.  The fused route computes the same result without the matrix: the
 * MFMA tile kernel of the dense scan with an epilogue that keeps only the scores that reach a per-query threshold (DESIGN.md
 * section 11).
 */
#ifndef JVECTOR_EXACT_FLAT_H
#define JVECTOR_EXACT_FLAT_H

#include "jvector_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N = rows of `vectors`.
 *   - Step 1 scores every accepted row against every query with the fused-chain arithmetic of jv_hip_exact_scan_dense (dot products
 *     and norms are k-ascending fmaf chains) and takes, per query, the top candK in NodeQueue order: higher score first, ties to the
 *     smaller id.  The ids and score bits are those of jv_hip_topk over a jv_hip_exact_scan_dense matrix with the rejected columns
 *     removed.  candK == 0: the top topK of that order, with those scores, is the result and step 2 is skipped.
 *   - Step 2 (candK >= topK): the candK candidates are rescored by the bit-exact scalar-order kernel behind jv_hip_exact_scores and
 *     the top topK by jv_hip_topk is returned: the same launchers, the same bits.
 *   - The mask is that of jv_hip_search_flat_filtered: bit n of word n / 64 set: row n may be returned.  accept_stride_words = 0: one
 *     mask for the batch; else query q reads accept_bits + q * accept_stride_words, with accept_stride_words >= ceil(N / 64).
 *     accept_bits is host or device memory.  Bits at and beyond N are ignored: the tail of the last word and any slack words of a
 *     wider stride may hold anything.  accept_bits == NULL: no filter.  Rejected rows are never returned and do not count toward
 *     candK.  Fewer accepted rows than topK leave a tail of (-1, -INFINITY).  id_base is added to valid ids only.
 *   - JV_ERR_INVALID: a NULL handle or output, topK < 1, candK < 0, 0 < candK < topK, a negative stride, a non-zero stride below
 *     ceil(N / 64), Q < 0.  Q == 0 returns JV_OK at once.  JV_ERR_UNSUPPORTED: a jv_vectors made by jv_hip_vectors_from_nvq (the
 *     float rows are needed).  A candK (or topK) above what the top-k takes gives that launcher's status.  A refused call leaves the
 *     outputs untouched.
 *   - Results are a function of the arguments only: an atomic decides a position in a candidate list, never a result, and neither
 *     the route nor the chunking of the queries changes an id or a score bit.
 *   - Two routes.  The fused route: a sample pass scores every g-th tile of 128 rows into a Q x S matrix whose kc-th best per query
 *     (kc = candK ? candK : topK) is a threshold at least kc accepted rows reach; a select pass scores all rows and appends the
 *     accepted rows that reach the threshold to a list of `cap` entries per query; a device-side check of the list lengths; the top
 *     kc of the lists.  If a list overflowed, the whole call runs the chunked route: the dense scan per chunk of rows, -1 ids for the
 *     rejected columns, a top-k per chunk and a merge.  Exactness depends on none of the options below.
 *   - Options (jv_hip_ctx_set_option): exact_flat_fused — unset or 0: the fused route is taken where N >= 65536 (below that the
 *     chunked route's one scan and one top-k are as fast and need no sample); 1: wherever N > 0; -1: never.
 *     exact_flat_sample_stride — g, in tiles of 128 rows; 0 (default): 16, more where that keeps the sample at 2^18 rows.
 *     exact_flat_cap — list entries per query; 0 (default): 4 kc g rounded up to 64.  exact_flat_score_bytes — default 1 GiB: the
 *     queries run in chunks whose sample matrix and lists (fused route) or score and id matrix (chunked route) stay under it.
 *   - Counters (jv_hip_ctx_get_stat): exact_flat_calls, exact_flat_fused_calls (answered by the fused route), exact_flat_fallbacks
 *     (tried it, failed the list-length check, answered by the chunked route), exact_flat_listed (sum of the list lengths of the
 *     select passes). */
JV_API int jv_hip_search_exact(jv_ctx *ctx, const jv_vectors *vectors, const float *queries, int Q, jv_vsf vsf, int topK, int candK,
                               const uint64_t *accept_bits, int64_t accept_stride_words, int32_t id_base, int32_t *out_ids,
                               float *out_scores);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_EXACT_FLAT_H */
