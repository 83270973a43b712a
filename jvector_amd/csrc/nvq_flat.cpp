// nvq_flat.cpp — the NVQ flat search (include/jvector_nvq_flat.h): the host driver over nvq_select_kernel (k_nvq_flat.hip,
// libjvector_hip_nf.so).  The structure is exact_flat.cpp's.  Two routes to the same top-kc of the tile scores among the accepted rows:
//   * the fused route (fused_route below): the kernel's sample pass over every g-th row tile, the existing top-k on the Q x S sample
//     (tau[q] = its kc-th best; -INFINITY when fewer than kc accepted rows were sampled, and then every accepted row passes), the
//     select pass over all tiles into Q x cap lists, a device-side check of the list lengths read back as one flag, launch_topk over
//     the lists.  tau is the kc-th best of a SUBSET of the accepted rows, so at least kc accepted rows reach it: only the upper
//     bound needs the check.
//   * the chunked route (chunked_route): the same kernel with the sample epilogue at stride 1 over chunks of rows — the dense NVQ
//     scan — then -1 ids for the rejected columns, a top-k per chunk and a merge, bounded by nvq_flat_score_bytes.  The route of
//     small N, of nvq_flat_fused = -1, and of a call whose lists overflowed.
// The query side (nvq_query_prep_kernel), the rescoring (launch_nvq_gather through rerank_gather) and the final top-k are the
// launchers jv_hip_nvq_scores and jv_hip_search_flat use.  The list reset, the list-length check and the chunk ids are the exact
// flat search's kernels (k_exact_flat.hip).
#include <vector>

#include "jv_internal.h"
#include "nf_params.h"
#include "xf_params.h"
#include "../../include/jvector_nvq_flat.h"

namespace jv {
// k_nvq_flat.hip
int launch_nvq_select(hipStream_t s, const NfParams &p, size_t p_bytes, int vsf, int select);
// k_exact_flat.hip
int launch_exact_flat_init(hipStream_t s, int32_t *ids, float *scores, int64_t cells, unsigned int *counts, int Q, XfCheck *chk);
int launch_exact_flat_check(hipStream_t s, const unsigned int *counts, int Q, int cap, XfCheck *chk);
int launch_exact_flat_ids(hipStream_t s, const XfIdsParams &p, size_t p_bytes);
}  // namespace jv

using namespace jv;

// nvq_flat_fused's auto gate: rows from which the fused route is taken.  The value is the exact flat search's,
// carried over unmeasured (section 12).
constexpr int64_t kFusedMinRows = 65536;
constexpr int64_t kSampleRowsMax = 1 << 18;   // the auto stride keeps the sample at this many rows
constexpr int64_t kChunkRows = 1 << 20;       // rows per chunk of the chunked route: a multiple of the tile

#define NF_TRY(expr, what)                                                 \
    do {                                                                   \
        int _s = (expr);                                                   \
        if (_s != JV_OK) {                                                 \
            set_error("nvq_search_flat: %s failed (status %d)", what, _s); \
            return _s;                                                     \
        }                                                                  \
    } while (0)

namespace {

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct Call {
    jv_ctx *ctx;
    const jv_nvq_vectors *nv;
    const float *d_a;        // the A operand: the queries; EUCLIDEAN: query - globalMean
    const float *d_qaux;     // [Q]
    const uint64_t *d_acc;   // nullptr: no filter
    int64_t stride_words;
    int Q, kvsf, kc;
    int32_t *d_k1_ids;       // [Q][kc]
    float *d_k1_sc;
    long long budget;
};

// the kernel's parameters for queries q_lo .. q_lo + nq; the caller sets the tiles and the epilogue
NfParams params_of(const Call &c, int64_t q_lo, int nq)
{
    const jv_nvq_vectors *nv = c.nv;
    NfParams p{};
    p.bytes = nv->d_bytes; p.derived = nv->d_derived; p.cosnorm = nv->d_cosnorm; p.mean = nv->nvq->d_mean;
    p.queries = c.d_a + q_lo * nv->nvq->D; p.qaux = c.d_qaux + q_lo;
    p.bits = c.d_acc ? c.d_acc + q_lo * c.stride_words : nullptr; p.stride_words = c.stride_words;
    p.n = nv->count; p.ld = nv->ld; p.D = nv->nvq->D; p.subs = nv->nvq->S; p.Q = nq;
    p.tile_stride = 1;
    return p;
}

// the top-kc of every query by the fused route; *done = false when some list overflowed (nothing the caller keeps was written)
int fused_route(const Call &c, int64_t g, int cap, bool *done, long long *listed)
{
    jv_ctx *ctx = c.ctx;
    const int64_t N = c.nv->count, n_tiles = (N + NF_TILE - 1) / NF_TILE;
    const int64_t s_tiles = (n_tiles + g - 1) / g, S = s_tiles * NF_TILE;
    const int kc = c.kc;
    // queries per chunk: the sample matrix and the lists stay under the budget; whole query tiles where that leaves any
    const size_t per_q = sizeof(float) * (size_t)S + 8 * (size_t)kc + 8 * (size_t)cap + sizeof(unsigned int);
    int64_t qc = (int64_t)((size_t)c.budget / per_q);
    if (qc >= NF_TILE) qc = qc / NF_TILE * NF_TILE;
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
        NfParams p = params_of(c, q_lo, nq);
        {
            ProfScope ps(ctx, R_SAMPLE);
            p.tiles = s_tiles; p.tile_stride = g; p.tile_offset = 0; p.samp = d_samp; p.S = S;
            NF_TRY(launch_nvq_select(ctx->stream, p, sizeof(p), c.kvsf, 0), "the sample pass");
        }
        {
            ProfScope ps(ctx, R_TOPK);
            JV_TRY(launch_topk(ctx->stream, ctx, d_samp, nullptr, nq, S, S, 0, kc, d_ks_ids, d_ks_sc, ctx->d_scratch.ptr));
        }
        NF_TRY(launch_exact_flat_init(ctx->stream, d_f_ids, nullptr, (int64_t)nq * cap, d_cnt, nq, d_chk), "the list reset");
        {
            ProfScope ps(ctx, R_EXACT);
            p.tiles = n_tiles; p.tile_stride = 1; p.samp = nullptr; p.S = 0;
            p.tau = d_ks_sc + (kc - 1); p.tau_stride = kc; p.cand_ids = d_f_ids; p.cand_scores = d_f_sc; p.cand_count = d_cnt; p.cap = cap;
            NF_TRY(launch_nvq_select(ctx->stream, p, sizeof(p), c.kvsf, 1), "the select pass");
        }
        NF_TRY(launch_exact_flat_check(ctx->stream, d_cnt, nq, cap, d_chk), "the list-length check");
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

// the same top-kc through score matrices of at most `budget` bytes: rows in chunks (whole tiles), queries in groups
int chunked_route(const Call &c)
{
    jv_ctx *ctx = c.ctx;
    const int64_t N = c.nv->count;
    const int kc = c.kc;
    const size_t cell = c.d_acc ? 8 : 4;   // a score, and an id under a mask
    int64_t C = std::min<int64_t>(N, kChunkRows);
    int64_t qg = (int64_t)((size_t)c.budget / (cell * (size_t)C));
    if (qg < NF_TILE && c.Q > qg) {   // a small budget: keep a query tile and shorten the chunks instead
        qg = std::min<int64_t>(c.Q, NF_TILE);
        C = std::max<int64_t>(NF_TILE, (int64_t)((size_t)c.budget / (cell * (size_t)qg)) / NF_TILE * NF_TILE);
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
        int32_t *k1_ids = c.d_k1_ids + q_lo * kc;
        float *k1_sc = c.d_k1_sc + q_lo * kc;
        int64_t col = 0;
        for (int64_t s = 0; s < N; s += C) {   // s is a multiple of the tile: C is one wherever there is a second chunk
            const int64_t rows = std::min(C, N - s);
            const int kk = (int)std::min<int64_t>(kc, rows);
            {
                ProfScope ps(ctx, R_EXACT);
                NfParams p = params_of(c, q_lo, nq);
                p.tiles = (rows + NF_TILE - 1) / NF_TILE; p.tile_offset = s / NF_TILE; p.samp = d_sc; p.S = rows;
                NF_TRY(launch_nvq_select(ctx->stream, p, sizeof(p), c.kvsf, 0), "the dense scan");
            }
            if (c.d_acc) {
                XfIdsParams ip{};
                ip.bits = c.d_acc + q_lo * c.stride_words; ip.stride_words = c.stride_words; ip.first = s; ip.count = rows; ip.ids = d_id; ip.Q = nq;
                NF_TRY(launch_exact_flat_ids(ctx->stream, ip, sizeof(ip)), "the chunk's ids");
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

int jv_hip_nvq_search_flat(jv_ctx *ctx, const jv_nvq_vectors *nv, const float *queries, int Q, jv_vsf vsf, int topK, int candK,
                           const uint64_t *accept_bits, int64_t accept_stride_words, int32_t id_base, int32_t *out_ids, float *out_scores)
{
    clear_error();
    JV_REQUIRE(ctx && nv, "nvq_search_flat: NULL argument");
    JV_REQUIRE(Q >= 0, "nvq_search_flat: negative query count");
    JV_REQUIRE(topK > 0, "nvq_search_flat: topK must be positive");
    JV_REQUIRE(candK >= 0, "nvq_search_flat: negative candK");
    JV_REQUIRE(candK == 0 || candK >= topK, "nvq_search_flat: candK %d must be 0 or >= topK %d", candK, topK);
    JV_REQUIRE(vsf == JV_EUCLIDEAN || vsf == JV_DOT_PRODUCT || vsf == JV_COSINE, "nvq_search_flat: unsupported similarity function %d", (int)vsf);
    const int64_t N = nv->count;
    const int64_t mask_words = (N + 63) / 64;
    JV_REQUIRE(accept_stride_words >= 0, "nvq_search_flat: negative accept stride");
    JV_REQUIRE(accept_stride_words == 0 || accept_stride_words >= mask_words, "nvq_search_flat: accept stride %lld < %lld words",
               (long long)accept_stride_words, (long long)mask_words);
    JV_REQUIRE(ctx->device == nv->device, "nvq_search_flat: the NVQ rows live on device %d, the context on %d", nv->device, ctx->device);
    if (Q == 0) return JV_OK;
    JV_REQUIRE(queries && out_ids && out_scores, "nvq_search_flat: NULL buffer");
    if (N > 0x7fffffffLL) {
        set_error("nvq_search_flat: %lld rows do not fit an ordinal", (long long)N);
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(use_device(ctx->device));
    const int D = nv->nvq->D;
    const bool rescore = candK > 0;
    const int kc = rescore ? candK : topK;
    const int masks = accept_stride_words == 0 ? 1 : Q;

    const void *d_q = nullptr, *d_acc = nullptr;
    JV_TRY(stage_in(ctx, queries, sizeof(float) * (size_t)Q * D, ctx->h_in, ctx->d_in, &d_q));
    if (accept_bits && N > 0)
        JV_TRY(stage_in(ctx, accept_bits, sizeof(uint64_t) * (size_t)(accept_stride_words * (masks - 1) + mask_words), ctx->h_in, ctx->d_gs_mask,
                        &d_acc));
    OutStage oi, osc;
    JV_TRY(stage_out_begin(ctx, out_ids, sizeof(int32_t) * (size_t)Q * topK, ctx->d_out, &oi));
    JV_TRY(stage_out_begin(ctx, out_scores, sizeof(float) * (size_t)Q * topK, ctx->d_bq_work, &osc));

    // scratch3: [qwork Q*D, EUCLIDEAN only: 16-byte aligned rows][cand ids Q*kc][cand tile scores Q*kc][NVQScorer scores Q*kc][qnorm Q][qaux Q]
    const size_t c1 = (size_t)Q * kc, b_work = vsf == JV_EUCLIDEAN ? al(sizeof(float) * (size_t)Q * D) : 0;
    JV_TRY(ctx->d_scratch3.reserve(b_work + sizeof(int32_t) * c1 + sizeof(float) * (c1 * 2 + 2 * (size_t)Q) + 1024));
    float *d_qwork = (float *)ctx->d_scratch3.ptr;
    int32_t *d_cand = (int32_t *)((char *)ctx->d_scratch3.ptr + b_work);
    float *d_cand_sc = (float *)(d_cand + c1);
    float *d_exact = d_cand_sc + c1;
    float *d_qnorm = d_exact + c1;
    float *d_qaux = d_qnorm + Q;
    JV_TRY(ctx->d_scratch.reserve(topk_scratch_bytes(Q, std::max(kc, topK))));

    Call c{};
    c.ctx = ctx; c.nv = nv; c.d_a = vsf == JV_EUCLIDEAN ? d_qwork : (const float *)d_q; c.d_qaux = d_qaux;
    c.d_acc = (const uint64_t *)d_acc; c.stride_words = accept_stride_words;
    c.Q = Q; c.kvsf = to_kernel_vsf(vsf); c.kc = kc;
    c.d_k1_ids = rescore ? d_cand : (int32_t *)oi.dev;
    c.d_k1_sc = rescore ? d_cand_sc : (float *)osc.dev;
    c.budget = std::max<long long>(1, ctx_opt(ctx, "nvq_flat_score_bytes", 1ll << 30));

    // ---------------- step 1: the top-kc of the tile scores among the accepted rows ----------------
    ctx_stat_add(ctx, "nvq_flat_calls", 1);
    if (N == 0) {
        NF_TRY(launch_exact_flat_init(ctx->stream, c.d_k1_ids, c.d_k1_sc, (int64_t)c1, nullptr, 0, nullptr), "the empty result");
    } else {
        JV_TRY(ensure_nvq_tables(ctx, const_cast<jv_nvq_vectors *>(nv), vsf == JV_COSINE));
        JV_TRY(launch_nvq_query_prep(ctx->stream, (const float *)d_q, Q, D, c.kvsf, nv->nvq->d_mean, d_qwork, d_qaux));
        const long long fused_opt = ctx_opt(ctx, "nvq_flat_fused", 0);
        bool done = false;
        if (fused_opt > 0 || (fused_opt == 0 && N >= kFusedMinRows)) {
            const int64_t n_tiles = (N + NF_TILE - 1) / NF_TILE;
            int64_t g = ctx_opt(ctx, "nvq_flat_sample_stride", 0);
            if (g <= 0) g = std::max<int64_t>(16, (N + kSampleRowsMax - 1) / kSampleRowsMax);
            g = std::min(g, n_tiles);
            long long cap = ctx_opt(ctx, "nvq_flat_cap", 0);
            if (cap <= 0) cap = (4ll * kc * g + 63) / 64 * 64;
            cap = std::min<long long>(cap, std::max<int64_t>(N, 64));
            long long listed = 0;
            JV_TRY(fused_route(c, g, (int)cap, &done, &listed));
            ctx_stat_add(ctx, "nvq_flat_listed", listed);
            ctx_stat_add(ctx, done ? "nvq_flat_fused_calls" : "nvq_flat_fallbacks", 1);
        }
        if (!done) JV_TRY(chunked_route(c));
    }

    // ---------------- step 2: NVQScorer's bits for the candidates (launch_nvq_gather), jv_hip_topk ----------------
    if (rescore) {
        jv_vectors view;   // what jv_hip_vectors_from_nvq makes: the reranker of jv_hip_search_flat over these rows
        view.device = nv->device; view.count = N; view.D = D; view.nvq = const_cast<jv_nvq_vectors *>(nv);
        JV_TRY(rerank_gather(ctx, &view, (const float *)d_q, Q, vsf, d_cand, kc, d_exact, d_qnorm));
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_exact, d_cand, Q, kc, kc, 0, topK, (int32_t *)oi.dev, (float *)osc.dev, ctx->d_scratch.ptr));
    }
    JV_TRY(launch_add_id_base(ctx->stream, (int32_t *)oi.dev, (int64_t)Q * topK, id_base));
    JV_TRY(stage_out_end(ctx, oi));
    return stage_out_end(ctx, osc);
}

}  // extern "C"
