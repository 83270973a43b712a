/*
 * jvector_bq.h — binary quantization (BQ) entry points of libjvector_hip.so: the third of JVector's vector compressors, next to
 * ProductQuantization and NVQuantization (jvector_hip.h).  Conventions are jvector_hip.h's: every call returns a jv_status,
 * jv_hip_last_error() describes a failure, user buffers may be host or device memory, a jv_ctx belongs to one host thread.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/):
 *   encode      BinaryQuantization.encode / encodeTo (B/quantization/BinaryQuantization.java): a vector of dimension D becomes
 *               W = ceil(D / 64) 64-bit words; bit j of word i is set iff v[64 i + j] > 0 (NaN, -0.0, +0.0 give 0; +inf gives 1);
 *               bits at and beyond D are 0.
 *   similarity  BQVectors.similarityBetween: 1 - (float) hammingDistance(a, b) / D in f32 (IEEE division), hammingDistance =
 *               sum of Long.bitCount(a[i] ^ b[i]) (DefaultVectorUtilSupport.hammingDistance).  The similarity function is
 *               ignored: scoreFunctionFor (query encoded with bq.encode(q)) and diversityFunctionFor (node vs node) both
 *               return the Hamming similarity.
 *   bytes       BinaryQuantization.write / load + BQVectors.write / load, big-endian: int D, D floats (written as zeros,
 *               ignored on load), int count, then — only when count > 0 — int compressedLength and count x compressedLength
 *               longs.
 *
 * Device layout of a jv_bq_vectors: row-major, W little-endian uint64 words per row in the reference's bit order (word i of
 * the reference's long[] is word i here; bit j is 1 << j); padding bits are zero.
 */
#ifndef JVECTOR_BQ_H
#define JVECTOR_BQ_H

#include "jvector_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jv_bq_vectors jv_bq_vectors;

/* BQVectors on the device: `count` rows of ceil(D / 64) words, zero filled.  D >= 1. */
JV_API int jv_hip_bq_create(jv_ctx *ctx, int D, int64_t count, jv_bq_vectors **out);
/* rows [first, first + count): src / dst hold count x W uint64 words (host or device) */
JV_API int jv_hip_bq_upload(jv_ctx *ctx, jv_bq_vectors *bq, int64_t first, int64_t count, const uint64_t *src);
JV_API int jv_hip_bq_download(jv_ctx *ctx, const jv_bq_vectors *bq, int64_t first, int64_t count, uint64_t *dst);
JV_API int64_t jv_hip_bq_count(const jv_bq_vectors *bq);      /* -1 for NULL */
JV_API int jv_hip_bq_dimension(const jv_bq_vectors *bq);      /* -1 for NULL */
JV_API int jv_hip_bq_destroy(jv_bq_vectors *bq);

/* BinaryQuantization.encodeAll: rows [first, first + count) of `v` into rows [dst_first, ...) of `dst` (same D). */
JV_API int jv_hip_bq_encode_into(jv_ctx *ctx, const jv_vectors *v, int64_t first, int64_t count, jv_bq_vectors *dst,
                                 int64_t dst_first);
/* BinaryQuantization.encode of arbitrary rows: rows = count x D floats, words_out = count x ceil(D / 64) uint64 words;
 * either may be host or device memory. */
JV_API int jv_hip_bq_encode(jv_ctx *ctx, int D, const float *rows, int64_t count, uint64_t *words_out);

/* Parses a BinaryQuantization + BQVectors block (host memory only, no device): D, count, W (words per row, 0 when count == 0),
 * data_offset (byte offset of the first long) and block_len (bytes of the whole block).  Any output may be NULL.
 * JV_ERR_INVALID: buffer shorter than the block, D < 1, negative count or compressedLength.  JV_ERR_UNSUPPORTED: a
 * compressedLength other than ceil(D / 64) (the reference accepts it; the device layout cannot hold it). */
JV_API int jv_hip_bq_describe(const uint8_t *buf, size_t len, int *D, int64_t *count, int *words, size_t *data_offset,
                              size_t *block_len);
/* BQVectors.load: a new jv_bq_vectors from the block at buf (host memory); *consumed = block_len (nullable). */
JV_API int jv_hip_bq_load(jv_ctx *ctx, const uint8_t *buf, size_t len, size_t *consumed, jv_bq_vectors **out);
/* BQVectors.write: *len_out = bytes of the block; it is written only when buf != NULL and cap >= *len_out (host memory). */
JV_API int jv_hip_bq_write(jv_ctx *ctx, const jv_bq_vectors *bq, uint8_t *buf, size_t cap, size_t *len_out);

/* scores_out[q * B + b] = scoreFunctionFor(queries[q]).similarityTo(ordinals[q * B + b]); queries: Q x D floats.
 * An ordinal outside [0, count) gives -INFINITY. */
JV_API int jv_hip_bq_scores(jv_ctx *ctx, const jv_bq_vectors *bq, const float *queries, int Q, const int32_t *ordinals, int B,
                            float *scores_out);
/* scores_out[p * C + c] = diversityFunctionFor(node1[p]).similarityTo(node2[p * C + c]); an ordinal outside [0, count) on
 * either side gives -INFINITY. */
JV_API int jv_hip_bq_pair_scores(jv_ctx *ctx, const jv_bq_vectors *bq, const int32_t *node1, int P, const int32_t *node2, int C,
                                 float *scores_out);

/* Two-pass flat search over every row of `bq`, the BQ counterpart of jv_hip_search_flat:
 *   1. encode the queries (Q x D floats);
 *   2. take the top-rerankK ACCEPTED rows by BQ similarity in NodeQueue order (higher score first, ties to the smaller id) —
 *      exact however many rows share the threshold distance; the scan runs on integer Hamming distances and never holds a
 *      Q x N score matrix;
 *   3. rerank them with vectors' exact scores under `vsf` (the launchers of jv_hip_search_flat: the same bits);
 *   4. return the top-K in NodeQueue order, id_base added to every id.
 * vectors == NULL or rerankK == 0: the BQ top-K with BQ similarities.  Otherwise rerankK >= topK and vectors->D == D,
 * vectors->count >= count.  Fewer valid rows than K leave a tail of (-1, -INFINITY).
 * accept_bits (nullable): jv_hip_graph_search_filtered's layout — bit n of word n / 64 set = row n may be returned;
 * accept_stride_words = 0 one mask for the batch, else query q reads accept_bits + q * accept_stride_words
 * (>= ceil(count / 64)).  Rejected rows are never returned and do not count toward rerankK.
 * out_ids / out_scores: Q x topK, host or device.  JV_ERR_INVALID: NULL handles / outputs, topK < 1, Q < 0, a dimension
 * mismatch; Q == 0 returns JV_OK at once.  Dimensions above 16383 are JV_ERR_UNSUPPORTED. */
JV_API int jv_hip_bq_search_flat(jv_ctx *ctx, const jv_bq_vectors *bq, const jv_vectors *vectors, const float *queries, int Q,
                                 jv_vsf vsf, int topK, int rerankK, const uint64_t *accept_bits, int64_t accept_stride_words,
                                 int32_t id_base, int32_t *out_ids, float *out_scores);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_BQ_H */
