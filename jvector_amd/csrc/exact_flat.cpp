// exact_flat.cpp — the exact flat search (include/jvector_exact_flat.h): the host driver over the kernels of k_exact_flat.hip
// (libjvector_hip_xf.so).  Two routes to the same top-kc of the fused-chain scores among the accepted rows:
//   * the fused route (fused_route below): exact_select_kernel's sample pass over every g-th row tile, the existing top-k on the
//     Q x S sample (tau[q] = its kc-th best; -INFINITY when fewer than kc accepted rows were sampled, and then every accepted row
//     passes), the select pass over all tiles into Q x cap lists, a device-side check of the list lengths read back as one flag,
//     launch_topk over the lists.  tau is the kc-th best of a SUBSET of the accepted rows, so at least kc accepted rows reach it
//     (all of them when there are fewer): only the upper bound needs the check.
//   * the chunked route (chunked_route): launch_exact_scan_dense per chunk of rows, -1 ids for the rejected columns, a top-k per
//     chunk and a merge — the recipe callers used to write by hand, bounded by exact_flat_score_bytes.  The route of small N, of
//     exact_flat_fused = -1, and of a call whose lists overflowed.
// The rescoring and the final top-k are jv_hip_exact_scores' and jv_hip_topk's own launchers on either route.
#include <vector>

#include "jv_internal.h"
#include "xf_params.h"
#include "../../include/jvector_exact_flat.h"

namespace jv {
// k_exact_flat.hip
int launch_exact_select(hipStream_t s, const XfParams &p, size_t p_bytes, int vsf, int select);
int launch_exact_flat_init(hipStream_t s, int32_t *ids, float *scores, int64_t cells, unsigned int *counts, int Q, XfCheck *chk);
int launch_exact_flat_check(hipStream_t s, const unsigned int *counts, int Q, int cap, XfCheck *chk);
int launch_exact_flat_ids(hipStream_t s, const XfIdsParams &p, size_t p_bytes);
}  // namespace jv

using namespace jv;

// exact_flat_fused's auto gate: rows from which the fused route is taken.  Below it one dense scan and one top-k over a matrix of a
// few megabytes is all the chunked route does, and a sample cannot pay for its extra launches.
constexpr int64_t kFusedMinRows = 65536;
constexpr int64_t kSampleRowsMax = 1 << 18;   // the auto stride keeps the sample at this many rows
constexpr int64_t kChunkRows = 1 << 20;       // rows per chunk of the chunked route

#define XF_TRY(expr, what)                                              \
    do {                                                                \
        int _s = (expr);                                                \
        if (_s != JV_OK) {                                              \
            set_error("search_exact: %s failed (status %d)", what, _s); \
            return _s;                                                  \
        }                                                               \
    } while (0)

namespace {

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct Call {
    jv_ctx *ctx;
    const jv_vectors *v;
    const float *d_q;
    const uint64_t *d_acc;   // nullptr: no filter
    int64_t stride_words;
    int Q, kvsf, kc;
    int32_t *d_k1_ids;       // [Q][kc]
    float *d_k1_sc;
    long long budget;
};

const uint64_t *mask_of(const Call &c, int64_t q_lo) { return c.d_acc ? c.d_acc + q_lo * c.stride_words : nullptr; }

// the top-kc of every query by the fused route; *done = false when some list overflowed (nothing the caller keeps was written)
int fused_route(const Call &c, int64_t g, int cap, bool *done, long long *listed)
{
    jv_ctx *ctx = c.ctx;
    const int64_t N = c.v->count, n_tiles = (N + XF_TILE - 1) / XF_TILE;
    const int64_t s_tiles = (n_tiles + g - 1) / g, S = s_tiles * XF_TILE;
    const int kc = c.kc;
    // queries per chunk: the sample matrix and the lists stay under the budget; whole query tiles where that leaves any
    const size_t per_q = sizeof(float) * (size_t)S + 8 * (size_t)kc + 8 * (size_t)cap + sizeof(unsigned int);
    int64_t qc = (int64_t)((size_t)c.budget / per_q);
    if (qc >= XF_TILE) qc = qc / XF_TILE * XF_TILE;
    qc = std::min<int64_t>(std::max<int64_t>(qc, 1), c.Q);

    const size_t b_samp = al(sizeof(float) * (size_t)qc * S), b_ks = al(sizeof(float) * (size_t)qc * kc);
    const size_t b_cap = al(sizeof(float) * (size_t)qc * cap), b_cnt = al(sizeof(unsigned int) * (size_t)qc);
    JV_TRY(ctx->d_scratch2.reserve(b_samp + 2 * b_ks + 2 * b_cap + b_cnt + al(sizeof(XfCheck))));
    char *base = (char *)ctx->d_scratch2.ptr;
    float *d_samp = (float *)base;
    int32_t *d_ks_ids = (int32_t *)(base + b_samp);
    float *d_ks_sc = (float *)(base + b_samp + b_ks);
    int32_t *d_f_ids = (int32_t *)(base + b_samp + 2 * b_ks);
    float *d_f_sc = (float *)(base + b_samp + 2 * b_ks + b_cap);
    unsigned int *d_cnt = (unsigned int *)(base + b_samp + 2 * b_ks + 2 * b_cap);
    XfCheck *d_chk = (XfCheck *)(base + b_samp + 2 * b_ks + 2 * b_cap + b_cnt);
    JV_TRY(ctx->h_out.reserve(sizeof(XfCheck)));

    *done = true;
    for (int64_t q_lo = 0; q_lo < c.Q; q_lo += qc) {
        const int nq = (int)std::min<int64_t>(qc, c.Q - q_lo);
        XfParams p{};
        p.vecs = c.v->d_vecs; p.queries = c.d_q + q_lo * c.v->D; p.bits = mask_of(c, q_lo); p.stride_words = c.stride_words;
        p.n = N; p.D = c.v->D; p.Q = nq;
        {
            ProfScope ps(ctx, R_SAMPLE);
            p.tiles = s_tiles; p.tile_stride = g; p.tile_offset = 0; p.samp = d_samp; p.S = S;
            XF_TRY(launch_exact_select(ctx->stream, p, sizeof(p), c.kvsf, 0), "the sample pass");
        }
        {
            ProfScope ps(ctx, R_TOPK);
            JV_TRY(launch_topk(ctx->stream, ctx, d_samp, nullptr, nq, S, S, 0, kc, d_ks_ids, d_ks_sc, ctx->d_scratch.ptr));
        }
        XF_TRY(launch_exact_flat_init(ctx->stream, d_f_ids, nullptr, (int64_t)nq * cap, d_cnt, nq, d_chk), "the list reset");
        {
            ProfScope ps(ctx, R_EXACT);
            p.tiles = n_tiles; p.tile_stride = 1; p.samp = nullptr; p.S = 0;
            p.tau = d_ks_sc + (kc - 1); p.tau_stride = kc; p.cand_ids = d_f_ids; p.cand_scores = d_f_sc; p.cand_count = d_cnt; p.cap = cap;
            XF_TRY(launch_exact_select(ctx->stream, p, sizeof(p), c.kvsf, 1), "the select pass");
        }
        XF_TRY(launch_exact_flat_check(ctx->stream, d_cnt, nq, cap, d_chk), "the list-length check");
        JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, d_chk, sizeof(XfCheck), hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const XfCheck chk = *(const XfCheck *)ctx->h_out.ptr;
        *listed += (long long)chk.listed;
        if (chk.over) {
            *done = false;
            return JV_OK;
        }
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_f_sc, d_f_ids, nq, cap, cap, 0, kc, c.d_k1_ids + q_lo * kc, c.d_k1_sc + q_lo * kc,
                           ctx->d_scratch.ptr, d_cnt));
    }
    return JV_OK;
}

// the same top-kc through score matrices of at most `budget` bytes: rows in chunks, queries in groups
int chunked_route(const Call &c)
{
    jv_ctx *ctx = c.ctx;
    const int64_t N = c.v->count;
    const int kc = c.kc;
    const size_t cell = c.d_acc ? 8 : 4;   // a score, and an id under a mask
    int64_t C = std::min<int64_t>(N, kChunkRows);
    int64_t qg = (int64_t)((size_t)c.budget / (cell * (size_t)C));
    if (qg < XF_TILE && c.Q > qg) {   // a small budget: keep a query tile and shorten the chunks instead
        qg = std::min<int64_t>(c.Q, XF_TILE);
        C = std::max<int64_t>(XF_TILE, (int64_t)((size_t)c.budget / (cell * (size_t)qg)) / XF_TILE * XF_TILE);
        C = std::min(C, N);
    }
    qg = std::min<int64_t>(std::max<int64_t>(qg, 1), std::min<int64_t>(c.Q, 32768));
    const int64_t n_chunks = (N + C - 1) / C;
    int64_t P = 0;   // columns of the merge: every chunk's min(kc, rows)
    for (int64_t s = 0; s < N; s += C) P += std::min<int64_t>(kc, std::min(C, N - s));

    const size_t b_sc = al(sizeof(float) * (size_t)qg * C), b_id = c.d_acc ? b_sc : 0;
    const size_t b_tmp = al(sizeof(float) * (size_t)qg * kc), b_part = al(sizeof(float) * (size_t)qg * P);
    JV_TRY(ctx->d_scratch2.reserve(b_sc + b_id + 2 * b_tmp + 2 * b_part));
    char *base = (char *)ctx->d_scratch2.ptr;
    float *d_sc = (float *)base;
    int32_t *d_id = c.d_acc ? (int32_t *)(base + b_sc) : nullptr;
    int32_t *d_tmp_ids = (int32_t *)(base + b_sc + b_id);
    float *d_tmp_sc = (float *)(base + b_sc + b_id + b_tmp);
    int32_t *d_part_ids = (int32_t *)(base + b_sc + b_id + 2 * b_tmp);
    float *d_part_sc = (float *)(base + b_sc + b_id + 2 * b_tmp + b_part);

    for (int64_t q_lo = 0; q_lo < c.Q; q_lo += qg) {
        const int nq = (int)std::min<int64_t>(qg, c.Q - q_lo);
        const float *d_q = c.d_q + q_lo * c.v->D;
        int32_t *k1_ids = c.d_k1_ids + q_lo * kc;
        float *k1_sc = c.d_k1_sc + q_lo * kc;
        int64_t col = 0;
        for (int64_t s = 0; s < N; s += C) {
            const int64_t rows = std::min(C, N - s);
            const int kk = (int)std::min<int64_t>(kc, rows);
            {
                ProfScope ps(ctx, R_EXACT);
                JV_TRY(launch_exact_scan_dense(ctx->stream, c.v->d_vecs, c.v->D, d_q, nq, c.kvsf, s, rows, d_sc));
            }
            if (c.d_acc) {
                XfIdsParams ip{};
                ip.bits = mask_of(c, q_lo); ip.stride_words = c.stride_words; ip.first = s; ip.count = rows; ip.ids = d_id; ip.Q = nq;
                XF_TRY(launch_exact_flat_ids(ctx->stream, ip, sizeof(ip)), "the chunk's ids");
            }
            const bool direct = n_chunks == 1 && kk == kc;   // one chunk: its top-k is the result
            ProfScope ps(ctx, R_TOPK);
            JV_TRY(launch_topk(ctx->stream, ctx, d_sc, d_id, nq, rows, rows, (int32_t)s, kk, direct ? k1_ids : d_tmp_ids,
                               direct ? k1_sc : d_tmp_sc, ctx->d_scratch.ptr));
            if (direct) break;
            JV_HIP_CHECK(hipMemcpy2DAsync(d_part_ids + col, sizeof(int32_t) * (size_t)P, d_tmp_ids, sizeof(int32_t) * (size_t)kk,
                                          sizeof(int32_t) * (size_t)kk, (size_t)nq, hipMemcpyDeviceToDevice, ctx->stream));
            JV_HIP_CHECK(hipMemcpy2DAsync(d_part_sc + col, sizeof(float) * (size_t)P, d_tmp_sc, sizeof(float) * (size_t)kk,
                                          sizeof(float) * (size_t)kk, (size_t)nq, hipMemcpyDeviceToDevice, ctx->stream));
            col += kk;
        }
        if (col > 0) {
            ProfScope ps(ctx, R_TOPK);
            JV_TRY(launch_topk(ctx->stream, ctx, d_part_sc, d_part_ids, nq, P, P, 0, kc, k1_ids, k1_sc, ctx->d_scratch.ptr));
        }
    }
    return JV_OK;
}

}  // namespace

extern "C" {

int jv_hip_search_exact(jv_ctx *ctx, const jv_vectors *vectors, const float *queries, int Q, jv_vsf vsf, int topK, int candK,
                        const uint64_t *accept_bits, int64_t accept_stride_words, int32_t id_base, int32_t *out_ids, float *out_scores)
{
    clear_error();
    JV_REQUIRE(ctx && vectors, "search_exact: NULL argument");
    JV_REQUIRE(Q >= 0, "search_exact: negative query count");
    JV_REQUIRE(topK > 0, "search_exact: topK must be positive");
    JV_REQUIRE(candK >= 0, "search_exact: negative candK");
    JV_REQUIRE(candK == 0 || candK >= topK, "search_exact: candK %d must be 0 or >= topK %d", candK, topK);
    const int64_t N = vectors->count;
    const int64_t mask_words = (N + 63) / 64;
    JV_REQUIRE(accept_stride_words >= 0, "search_exact: negative accept stride");
    JV_REQUIRE(accept_stride_words == 0 || accept_stride_words >= mask_words, "search_exact: accept stride %lld < %lld words",
               (long long)accept_stride_words, (long long)mask_words);
    JV_FLOAT_ROWS(vectors, "search_exact");
    if (Q == 0) return JV_OK;
    JV_REQUIRE(queries && out_ids && out_scores, "search_exact: NULL buffer");
    if (N > 0x7fffffffLL) {
        set_error("search_exact: %lld rows do not fit an ordinal", (long long)N);
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(use_device(ctx->device));
    const bool rescore = candK > 0;
    const int kc = rescore ? candK : topK;
    const int masks = accept_stride_words == 0 ? 1 : Q;

    const void *d_q = nullptr, *d_acc = nullptr;
    JV_TRY(stage_in(ctx, queries, sizeof(float) * (size_t)Q * vectors->D, ctx->h_in, ctx->d_in, &d_q));
    if (accept_bits && N > 0)
        JV_TRY(stage_in(ctx, accept_bits, sizeof(uint64_t) * (size_t)(accept_stride_words * (masks - 1) + mask_words), ctx->h_in, ctx->d_gs_mask,
                        &d_acc));
    OutStage oi, osc;
    JV_TRY(stage_out_begin(ctx, out_ids, sizeof(int32_t) * (size_t)Q * topK, ctx->d_out, &oi));
    JV_TRY(stage_out_begin(ctx, out_scores, sizeof(float) * (size_t)Q * topK, ctx->d_bq_work, &osc));

    // scratch3: [cand ids Q*kc][cand fused-chain scores Q*kc][exact scores Q*kc][qnorm Q]
    const size_t c1 = (size_t)Q * kc;
    JV_TRY(ctx->d_scratch3.reserve(sizeof(int32_t) * c1 + sizeof(float) * c1 * 2 + sizeof(float) * (size_t)Q + 1024));
    int32_t *d_cand = (int32_t *)ctx->d_scratch3.ptr;
    float *d_cand_sc = (float *)(d_cand + c1);
    float *d_exact = d_cand_sc + c1;
    float *d_qnorm = d_exact + c1;
    JV_TRY(ctx->d_scratch.reserve(topk_scratch_bytes(Q, std::max(kc, topK))));

    Call c{};
    c.ctx = ctx; c.v = vectors; c.d_q = (const float *)d_q; c.d_acc = (const uint64_t *)d_acc; c.stride_words = accept_stride_words;
    c.Q = Q; c.kvsf = to_kernel_vsf(vsf); c.kc = kc;
    c.d_k1_ids = rescore ? d_cand : (int32_t *)oi.dev;
    c.d_k1_sc = rescore ? d_cand_sc : (float *)osc.dev;
    c.budget = std::max<long long>(1, ctx_opt(ctx, "exact_flat_score_bytes", 1ll << 30));

    // ---------------- step 1: the top-kc of the fused-chain scores among the accepted rows ----------------
    ctx_stat_add(ctx, "exact_flat_calls", 1);
    if (N == 0) {
        XF_TRY(launch_exact_flat_init(ctx->stream, c.d_k1_ids, c.d_k1_sc, (int64_t)c1, nullptr, 0, nullptr), "the empty result");
    } else {
        const long long fused_opt = ctx_opt(ctx, "exact_flat_fused", 0);
        bool done = false;
        if (fused_opt > 0 || (fused_opt == 0 && N >= kFusedMinRows)) {
            const int64_t n_tiles = (N + XF_TILE - 1) / XF_TILE;
            int64_t g = ctx_opt(ctx, "exact_flat_sample_stride", 0);
            if (g <= 0) g = std::max<int64_t>(16, (N + kSampleRowsMax - 1) / kSampleRowsMax);
            g = std::min(g, n_tiles);
            long long cap = ctx_opt(ctx, "exact_flat_cap", 0);
            if (cap <= 0) cap = (4ll * kc * g + 63) / 64 * 64;
            cap = std::min<long long>(cap, std::max<int64_t>(N, 64));
            long long listed = 0;
            JV_TRY(fused_route(c, g, (int)cap, &done, &listed));
            ctx_stat_add(ctx, "exact_flat_listed", listed);
            ctx_stat_add(ctx, done ? "exact_flat_fused_calls" : "exact_flat_fallbacks", 1);
        }
        if (!done) JV_TRY(chunked_route(c));
    }

    // ---------------- step 2: jv_hip_exact_scores' kernel over the candidates, jv_hip_topk ----------------
    if (rescore) {
        JV_TRY(rerank_gather(ctx, vectors, (const float *)d_q, Q, vsf, d_cand, kc, d_exact, d_qnorm));
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_exact, d_cand, Q, kc, kc, 0, topK, (int32_t *)oi.dev, (float *)osc.dev, ctx->d_scratch.ptr));
    }
    JV_TRY(launch_add_id_base(ctx->stream, (int32_t *)oi.dev, (int64_t)Q * topK, id_base));
    JV_TRY(stage_out_end(ctx, oi));
    return stage_out_end(ctx, osc);
}

}  // extern "C"
