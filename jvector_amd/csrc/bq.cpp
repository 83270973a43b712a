// bq.cpp — host side of binary quantization (include/jvector_bq.h): the device row store, the reference's byte format, and the
// entry points over k_bq.hip.  The flat search reuses jv_hip_search_flat's launchers for the exact rerank and the final top-K
// (rerank_gather -> launch_exact_gather, launch_topk), so its reranked results carry the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"

namespace jv {

static int bq_words(int D) { return (D + 63) / 64; }

static uint32_t be_u32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }
static void put_be_u32(uint8_t *p, uint32_t v)
{
    for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (24 - 8 * i));
}

// the scan's query tile: the largest of {32, 16, 8} whose histogram (QT x (D + 1) counters) fits 64 KB, no wider than needed
static int bq_tile(int Q, int D)
{
    if (Q <= 1) return 1;
    int qt = 1;
    for (int c : {8, 16, 32})
        if ((size_t)c * (D + 1) * 4 <= 65536) qt = c;
    while (qt > 8 && qt / 2 >= Q) qt /= 2;
    return qt;
}

static int bq_check(const jv_ctx *ctx, const jv_bq_vectors *bq, const char *what)
{
    JV_REQUIRE(ctx && bq, "%s: NULL argument", what);
    JV_REQUIRE(bq->device == ctx->device, "%s: the BQ vectors live on device %d, the context on %d", what, bq->device, ctx->device);
    return JV_OK;
}

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_bq_create(jv_ctx *ctx, int D, int64_t count, jv_bq_vectors **out)
{
    clear_error();
    JV_REQUIRE(ctx && out, "bq_create: NULL argument");
    *out = nullptr;
    JV_REQUIRE(D >= 1, "bq_create: dimension %d < 1", D);
    JV_REQUIRE(count >= 0 && count <= INT32_MAX, "bq_create: count %lld out of range", (long long)count);
    JV_TRY(use_device(ctx->device));
    jv_bq_vectors *b = new jv_bq_vectors();
    b->device = ctx->device;
    b->D = D;
    b->W = bq_words(D);
    b->count = count;
    const size_t bytes = sizeof(uint64_t) * (size_t)count * b->W;
    if (bytes) {
        hipError_t e = hipMalloc(&b->d_rows, bytes);
        if (e == hipSuccess) e = hipMemsetAsync(b->d_rows, 0, bytes, ctx->stream);
        if (e != hipSuccess) {
            set_error("bq_create: %zu bytes: %s", bytes, hipGetErrorString(e));
            (void)hipGetLastError();
            jv_hip_bq_destroy(b);
            return e == hipErrorOutOfMemory ? JV_ERR_OOM : JV_ERR_HIP;
        }
    }
    *out = b;
    return JV_OK;
}

int jv_hip_bq_upload(jv_ctx *ctx, jv_bq_vectors *bq, int64_t first, int64_t count, const uint64_t *src)
{
    clear_error();
    JV_TRY(bq_check(ctx, bq, "bq_upload"));
    JV_REQUIRE(first >= 0 && count >= 0 && first + count <= bq->count, "bq_upload: rows out of range");
    if (count == 0) return JV_OK;
    JV_REQUIRE(src, "bq_upload: NULL buffer");
    JV_TRY(use_device(ctx->device));
    JV_HIP_CHECK(hipMemcpyAsync(bq->d_rows + first * bq->W, src, sizeof(uint64_t) * (size_t)count * bq->W, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // a pageable source must not outlive the call
    return JV_OK;
}

int jv_hip_bq_download(jv_ctx *ctx, const jv_bq_vectors *bq, int64_t first, int64_t count, uint64_t *dst)
{
    clear_error();
    JV_TRY(bq_check(ctx, bq, "bq_download"));
    JV_REQUIRE(first >= 0 && count >= 0 && first + count <= bq->count, "bq_download: rows out of range");
    if (count == 0) return JV_OK;
    JV_REQUIRE(dst, "bq_download: NULL buffer");
    JV_TRY(use_device(ctx->device));
    JV_HIP_CHECK(hipMemcpyAsync(dst, bq->d_rows + first * bq->W, sizeof(uint64_t) * (size_t)count * bq->W, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return JV_OK;
}

int64_t jv_hip_bq_count(const jv_bq_vectors *bq) { return bq ? bq->count : -1; }
int jv_hip_bq_dimension(const jv_bq_vectors *bq) { return bq ? bq->D : -1; }

int jv_hip_bq_destroy(jv_bq_vectors *bq)
{
    if (!bq) return JV_OK;
    if (bq->d_rows) {
        (void)hipSetDevice(bq->device);
        (void)hipFree(bq->d_rows);
    }
    delete bq;
    return JV_OK;
}

int jv_hip_bq_encode_into(jv_ctx *ctx, const jv_vectors *v, int64_t first, int64_t count, jv_bq_vectors *dst, int64_t dst_first)
{
    clear_error();
    JV_TRY(bq_check(ctx, dst, "bq_encode_into"));
    JV_REQUIRE(v, "bq_encode_into: NULL vectors");
    JV_FLOAT_ROWS(v, "bq_encode_into");
    JV_REQUIRE(v->D == dst->D, "bq_encode_into: vectors of dimension %d, BQ of dimension %d", v->D, dst->D);
    JV_REQUIRE(first >= 0 && count >= 0 && first + count <= v->count, "bq_encode_into: source rows out of range");
    JV_REQUIRE(dst_first >= 0 && dst_first + count <= dst->count, "bq_encode_into: destination rows out of range");
    if (count == 0) return JV_OK;
    JV_TRY(use_device(ctx->device));
    ProfScope ps(ctx, R_ENCODE);
    return launch_bq_encode(ctx->stream, v->d_vecs + first * (int64_t)v->D, count, v->D, dst->W, 0, dst->d_rows + dst_first * dst->W);
}

int jv_hip_bq_encode(jv_ctx *ctx, int D, const float *rows, int64_t count, uint64_t *words_out)
{
    clear_error();
    JV_REQUIRE(ctx, "bq_encode: ctx is NULL");
    JV_REQUIRE(D >= 1 && count >= 0, "bq_encode: bad sizes");
    if (count == 0) return JV_OK;
    JV_REQUIRE(rows && words_out, "bq_encode: NULL buffer");
    JV_TRY(use_device(ctx->device));
    const int W = bq_words(D);
    const void *d_src = nullptr;
    JV_TRY(stage_in(ctx, rows, sizeof(float) * (size_t)count * D, ctx->h_in, ctx->d_in, &d_src));
    OutStage os;
    JV_TRY(stage_out_begin(ctx, words_out, sizeof(uint64_t) * (size_t)count * W, ctx->d_out, &os));
    {
        ProfScope ps(ctx, R_ENCODE);
        JV_TRY(launch_bq_encode(ctx->stream, (const float *)d_src, count, D, W, 0, (uint64_t *)os.dev));
    }
    return stage_out_end(ctx, os);
}

int jv_hip_bq_describe(const uint8_t *buf, size_t len, int *D_out, int64_t *count_out, int *words_out, size_t *data_offset,
                       size_t *block_len)
{
    clear_error();
    JV_REQUIRE(buf || len == 0, "bq_describe: NULL buffer");
    JV_REQUIRE(len >= 4, "bq_describe: truncated (%zu bytes, no dimension)", len);
    const int32_t D = (int32_t)be_u32(buf);
    JV_REQUIRE(D >= 1, "bq_describe: dimension %d < 1", D);
    const size_t off_count = 4 + 4 * (size_t)D;
    JV_REQUIRE(len >= off_count + 4, "bq_describe: truncated (%zu bytes, the header needs %zu)", len, off_count + 4);
    const int32_t count = (int32_t)be_u32(buf + off_count);
    JV_REQUIRE(count >= 0, "bq_describe: invalid compressed vector count %d", count);
    int W = 0;
    size_t data = off_count + 4, total = data;
    if (count > 0) {
        JV_REQUIRE(len >= off_count + 8, "bq_describe: truncated (no compressed length)");
        const int32_t cl = (int32_t)be_u32(buf + off_count + 4);
        JV_REQUIRE(cl >= 0, "bq_describe: invalid compressed vector dimension %d", cl);
        if (cl != bq_words(D)) {
            set_error("bq_describe: compressed length %d, a dimension of %d needs %d words", cl, D, bq_words(D));
            return JV_ERR_UNSUPPORTED;
        }
        W = cl;
        data = off_count + 8;
        total = data + sizeof(uint64_t) * (size_t)count * W;
        JV_REQUIRE(len >= total, "bq_describe: truncated (%zu bytes, the block needs %zu)", len, total);
    }
    if (D_out) *D_out = D;
    if (count_out) *count_out = count;
    if (words_out) *words_out = W;
    if (data_offset) *data_offset = data;
    if (block_len) *block_len = total;
    return JV_OK;
}

int jv_hip_bq_load(jv_ctx *ctx, const uint8_t *buf, size_t len, size_t *consumed, jv_bq_vectors **out)
{
    clear_error();
    JV_REQUIRE(ctx && out, "bq_load: NULL argument");
    *out = nullptr;
    int D = 0, W = 0;
    int64_t count = 0;
    size_t data = 0, total = 0;
    JV_TRY(jv_hip_bq_describe(buf, len, &D, &count, &W, &data, &total));
    jv_bq_vectors *b = nullptr;
    JV_TRY(jv_hip_bq_create(ctx, D, count, &b));
    if (count > 0) {
        std::vector<uint64_t> host((size_t)count * W);
        const uint8_t *p = buf + data;
        for (size_t i = 0; i < host.size(); ++i, p += 8) host[i] = (uint64_t)be_u32(p) << 32 | be_u32(p + 4);
        int s = jv_hip_bq_upload(ctx, b, 0, count, host.data());
        if (s != JV_OK) {
            jv_hip_bq_destroy(b);
            return s;
        }
    }
    if (consumed) *consumed = total;
    *out = b;
    return JV_OK;
}

int jv_hip_bq_write(jv_ctx *ctx, const jv_bq_vectors *bq, uint8_t *buf, size_t cap, size_t *len_out)
{
    clear_error();
    JV_TRY(bq_check(ctx, bq, "bq_write"));
    JV_REQUIRE(len_out, "bq_write: len_out is NULL");
    const size_t off_count = 4 + 4 * (size_t)bq->D;
    const size_t total = off_count + 4 + (bq->count > 0 ? 4 + sizeof(uint64_t) * (size_t)bq->count * bq->W : 0);
    *len_out = total;
    if (!buf || cap < total) return JV_OK;
    memset(buf, 0, off_count);   // the dimension's zero floats (BinaryQuantization.write)
    put_be_u32(buf, (uint32_t)bq->D);
    put_be_u32(buf + off_count, (uint32_t)bq->count);
    if (bq->count > 0) {
        put_be_u32(buf + off_count + 4, (uint32_t)bq->W);
        std::vector<uint64_t> host((size_t)bq->count * bq->W);
        JV_TRY(jv_hip_bq_download(ctx, bq, 0, bq->count, host.data()));
        uint8_t *p = buf + off_count + 8;
        for (size_t i = 0; i < host.size(); ++i, p += 8) {
            put_be_u32(p, (uint32_t)(host[i] >> 32));
            put_be_u32(p + 4, (uint32_t)host[i]);
        }
    }
    return JV_OK;
}

int jv_hip_bq_scores(jv_ctx *ctx, const jv_bq_vectors *bq, const float *queries, int Q, const int32_t *ordinals, int B, float *scores_out)
{
    clear_error();
    JV_TRY(bq_check(ctx, bq, "bq_scores"));
    JV_REQUIRE(Q >= 0 && B >= 0, "bq_scores: negative sizes");
    if (Q == 0 || B == 0) return JV_OK;
    JV_REQUIRE(queries && ordinals && scores_out, "bq_scores: NULL buffer");
    JV_TRY(use_device(ctx->device));
    const void *d_q = nullptr, *d_ord = nullptr;
    JV_TRY(stage_in(ctx, queries, sizeof(float) * (size_t)Q * bq->D, ctx->h_in, ctx->d_in, &d_q));
    JV_TRY(stage_in(ctx, ordinals, sizeof(int32_t) * (size_t)Q * B, ctx->h_in, ctx->d_scratch2, &d_ord));
    JV_TRY(ctx->d_bin_work.reserve(sizeof(uint64_t) * (size_t)Q * bq->W));
    OutStage os;
    JV_TRY(stage_out_begin(ctx, scores_out, sizeof(float) * (size_t)Q * B, ctx->d_out, &os));
    JV_TRY(launch_bq_encode(ctx->stream, (const float *)d_q, Q, bq->D, bq->W, 0, (uint64_t *)ctx->d_bin_work.ptr));
    JV_TRY(launch_bq_gather(ctx->stream, bq->d_rows, bq->count, bq->W, bq->D, (const uint64_t *)ctx->d_bin_work.ptr, nullptr, Q,
                            (const int32_t *)d_ord, B, (float *)os.dev));
    return stage_out_end(ctx, os);
}

int jv_hip_bq_pair_scores(jv_ctx *ctx, const jv_bq_vectors *bq, const int32_t *node1, int P, const int32_t *node2, int C, float *scores_out)
{
    clear_error();
    JV_TRY(bq_check(ctx, bq, "bq_pair_scores"));
    JV_REQUIRE(P >= 0 && C >= 0, "bq_pair_scores: negative sizes");
    if (P == 0 || C == 0) return JV_OK;
    JV_REQUIRE(node1 && node2 && scores_out, "bq_pair_scores: NULL buffer");
    JV_TRY(use_device(ctx->device));
    const void *d_n1 = nullptr, *d_n2 = nullptr;
    JV_TRY(stage_in(ctx, node1, sizeof(int32_t) * (size_t)P, ctx->h_in, ctx->d_in, &d_n1));
    JV_TRY(stage_in(ctx, node2, sizeof(int32_t) * (size_t)P * C, ctx->h_in, ctx->d_scratch2, &d_n2));
    OutStage os;
    JV_TRY(stage_out_begin(ctx, scores_out, sizeof(float) * (size_t)P * C, ctx->d_out, &os));
    JV_TRY(launch_bq_gather(ctx->stream, bq->d_rows, bq->count, bq->W, bq->D, nullptr, (const int32_t *)d_n1, P, (const int32_t *)d_n2, C,
                            (float *)os.dev));
    return stage_out_end(ctx, os);
}

int jv_hip_bq_search_flat(jv_ctx *ctx, const jv_bq_vectors *bq, const jv_vectors *vectors, const float *queries, int Q, jv_vsf vsf,
                          int topK, int rerankK, const uint64_t *accept_bits, int64_t accept_stride_words, int32_t id_base,
                          int32_t *out_ids, float *out_scores)
{
    clear_error();
    JV_TRY(bq_check(ctx, bq, "bq_search_flat"));
    JV_REQUIRE(Q >= 0, "bq_search_flat: negative query count");
    JV_REQUIRE(topK > 0, "bq_search_flat: topK must be positive");
    JV_REQUIRE(rerankK >= 0, "bq_search_flat: negative rerankK");
    const bool rerank = vectors != nullptr && rerankK > 0;
    JV_REQUIRE(!rerank || rerankK >= topK, "rerankK %d must be >= topK %d", rerankK, topK);
    JV_REQUIRE(!rerank || vectors->D == bq->D, "bq_search_flat: vectors of dimension %d, BQ of dimension %d", rerank ? vectors->D : 0,
               bq->D);
    JV_REQUIRE(!rerank || vectors->count >= bq->count, "bq_search_flat: fewer vectors than BQ rows");
    const int64_t N = bq->count;
    const int64_t mask_words = (N + 63) / 64;
    JV_REQUIRE(accept_stride_words == 0 || accept_stride_words >= mask_words, "bq_search_flat: accept stride %lld < %lld words",
               (long long)accept_stride_words, (long long)mask_words);
    JV_REQUIRE(accept_stride_words >= 0, "bq_search_flat: negative accept stride");
    if (Q == 0) return JV_OK;
    JV_REQUIRE(queries && out_ids && out_scores, "bq_search_flat: NULL buffer");
    if (bq->D > kBqMaxDim) {
        set_error("bq_search_flat: dimension %d above %d", bq->D, kBqMaxDim);
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(use_device(ctx->device));
    const int D = bq->D, W = bq->W;
    const int k1 = rerank ? rerankK : topK;
    const int qt = bq_tile(Q, D);
    const int tiles = (Q + qt - 1) / qt;
    // rows per block: enough blocks for eight per CU over all tiles, whole waves of 256 rows
    int64_t X = std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, ((int64_t)8 * ctx->num_cus + tiles - 1) / tiles));
    int64_t R = ((N + X - 1) / X + 255) / 256 * 256;
    if (R == 0) R = 256;
    X = std::max<int64_t>(1, (N + R - 1) / R);
    // list capacity: every row below the threshold (< k1) plus the ties, up to k1 + max(k1, 4096) of them; more ties go in by rank
    const int cap = (int)std::max<int64_t>(1, std::min<int64_t>(N, (int64_t)k1 + std::max(k1, 4096)));

    const void *d_q = nullptr, *d_acc = nullptr;
    JV_TRY(stage_in(ctx, queries, sizeof(float) * (size_t)Q * D, ctx->h_in, ctx->d_in, &d_q));
    if (accept_bits)
        JV_TRY(stage_in(ctx, accept_bits, sizeof(uint64_t) * (size_t)(accept_stride_words * (Q - 1) + mask_words), ctx->h_in,
                        ctx->d_scratch2, &d_acc));

    // work: [query words tiles x W x qt][hist Q x (D + 1)][thr, need, all_ties, cand_cnt: Q each][tiec Q x X][tie_prefix Q x X]
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_qw = al(sizeof(uint64_t) * (size_t)tiles * W * qt), b_hist = al(sizeof(uint32_t) * (size_t)Q * (D + 1));
    const size_t b_q = al(sizeof(int32_t) * (size_t)Q), b_x = al(sizeof(uint32_t) * (size_t)Q * X);
    JV_TRY(ctx->d_bin_work.reserve(b_qw + b_hist + 4 * b_q + 2 * b_x));
    char *wb = (char *)ctx->d_bin_work.ptr;
    uint64_t *d_qw = (uint64_t *)wb;
    BqScanArgs a;
    a.N = N;
    a.D = D;
    a.W = W;
    a.Q = Q;
    a.tiles = tiles;
    a.X = X;
    a.R = R;
    a.accept = (const uint64_t *)d_acc;
    a.accept_stride = accept_stride_words;
    a.hist = (uint32_t *)(wb + b_qw);
    a.thr = (int32_t *)(wb + b_qw + b_hist);
    a.need = (int32_t *)(wb + b_qw + b_hist + b_q);
    a.all_ties = (int32_t *)(wb + b_qw + b_hist + 2 * b_q);
    a.cand_cnt = (unsigned int *)(wb + b_qw + b_hist + 3 * b_q);
    a.tiec = (uint32_t *)(wb + b_qw + b_hist + 4 * b_q);
    a.tie_prefix = (uint32_t *)(wb + b_qw + b_hist + 4 * b_q + b_x);
    a.cap = cap;
    // candidates: [ids Q x cap][scores Q x cap][top-k1 ids Q x k1][top-k1 scores Q x k1][exact Q x k1][qnorm Q]
    const size_t c1 = (size_t)Q * k1, cc = (size_t)Q * cap;
    JV_TRY(ctx->d_bin_cand.reserve(al(4 * cc) * 2 + al(4 * c1) * 3 + al(4 * (size_t)Q)));
    char *cb = (char *)ctx->d_bin_cand.ptr;
    a.cand_ids = (int32_t *)cb;
    a.cand_sc = (float *)(cb + al(4 * cc));
    int32_t *d_k1_ids = (int32_t *)(cb + 2 * al(4 * cc));
    float *d_k1_sc = (float *)(cb + 2 * al(4 * cc) + al(4 * c1));
    float *d_exact = (float *)(cb + 2 * al(4 * cc) + 2 * al(4 * c1));
    float *d_qnorm = (float *)(cb + 2 * al(4 * cc) + 3 * al(4 * c1));
    JV_TRY(ctx->d_scratch.reserve(topk_scratch_bytes(Q, std::max(k1, topK))));

    OutStage oi, osc;
    JV_TRY(stage_out_begin(ctx, out_ids, sizeof(int32_t) * (size_t)Q * topK, ctx->d_out, &oi));
    JV_TRY(stage_out_begin(ctx, out_scores, sizeof(float) * (size_t)Q * topK, ctx->d_scratch3, &osc));

    JV_HIP_CHECK(hipMemsetAsync(d_qw, 0, b_qw + b_hist, ctx->stream));   // padded queries of the last tile, the histogram
    {
        ProfScope ps(ctx, R_ENCODE);
        JV_TRY(launch_bq_encode(ctx->stream, (const float *)d_q, Q, D, W, qt, d_qw));
    }
    {
        ProfScope ps(ctx, R_ADC);
        JV_TRY(launch_bq_select(ctx->stream, bq->d_rows, d_qw, a, qt, k1));
    }
    if (rerank) {
        {
            ProfScope ps(ctx, R_TOPK);
            JV_TRY(launch_topk(ctx->stream, ctx, a.cand_sc, a.cand_ids, Q, cap, cap, 0, k1, d_k1_ids, d_k1_sc, ctx->d_scratch.ptr,
                               a.cand_cnt));
        }
        JV_TRY(rerank_gather(ctx, vectors, (const float *)d_q, Q, vsf, d_k1_ids, k1, d_exact, d_qnorm));
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_exact, d_k1_ids, Q, k1, k1, 0, topK, (int32_t *)oi.dev, (float *)osc.dev, ctx->d_scratch.ptr));
    } else {
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, a.cand_sc, a.cand_ids, Q, cap, cap, 0, topK, (int32_t *)oi.dev, (float *)osc.dev,
                           ctx->d_scratch.ptr, a.cand_cnt));
    }
    JV_TRY(launch_add_id_base(ctx->stream, (int32_t *)oi.dev, (int64_t)Q * topK, id_base));
    JV_TRY(stage_out_end(ctx, oi));
    return stage_out_end(ctx, osc);
}

}  // extern "C"
