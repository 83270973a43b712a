// flat_accept.cpp — the flat PQ search under an accept filter (include/jvector_flat_filtered.h): the host driver over the kernels of
// k_flat_accept.hip (libjvector_hip_fa.so).  The accept masks become ascending ordinal lists on the device; a shared mask on a shape
// the multi-query kernel takes is scored by adc_mq_list_kernel (a code row is fetched once for four queries), per-query masks and the
// other shapes go through launch_adc_pitched; the top-k, the exact rerank and the finish are jv_hip_search_flat's own launchers.
#include "fa_params.h"
#include "jv_internal.h"
#include "../../include/jvector_flat_filtered.h"

namespace jv {
// k_flat_accept.hip
int launch_flat_accept_count(hipStream_t s, const FaScanParams &p, size_t p_bytes, int masks);
int launch_flat_accept_write(hipStream_t s, const FaScanParams &p, size_t p_bytes, int rows);
int launch_flat_accept_adc_list(hipStream_t s, const FaAdcParams &p, size_t p_bytes, int vsf, int num_cus);
int launch_flat_accept_map(hipStream_t s, const FaMapParams &p, size_t p_bytes);
}  // namespace jv

using namespace jv;

#define FA_TRY(expr, what)                                                      \
    do {                                                                        \
        int _s = (expr);                                                        \
        if (_s != JV_OK) {                                                      \
            set_error("search_flat_filtered: %s failed (status %d)", what, _s);  \
            return _s;                                                          \
        }                                                                       \
    } while (0)

extern "C" {

int jv_hip_search_flat_filtered(jv_ctx *ctx, jv_luts *l, const jv_codes *codes, const jv_vectors *vectors, const float *queries, int Q,
                                jv_vsf vsf, int topK, int rerankK, const uint64_t *accept_bits, int64_t accept_stride_words,
                                int32_t id_base, int32_t *out_ids, float *out_scores, int64_t *accepted_out)
{
    clear_error();
    JV_REQUIRE(ctx && l && codes, "search_flat_filtered: NULL argument");
    JV_REQUIRE(Q >= 0, "search_flat_filtered: negative query count");
    JV_REQUIRE(topK > 0, "search_flat_filtered: topK must be positive");
    JV_REQUIRE(rerankK >= 0, "search_flat_filtered: negative rerankK");
    const bool rerank = vectors != nullptr && rerankK > 0;
    JV_REQUIRE(!rerank || rerankK >= topK, "rerankK %d must be >= topK %d", rerankK, topK);
    JV_REQUIRE(!rerank || vectors->D == l->pq->D, "search_flat_filtered: vector dimension mismatch");
    JV_REQUIRE(!rerank || vectors->count >= codes->count, "search_flat_filtered: fewer vectors than codes");
    const int64_t N = codes->count;
    const int64_t mask_words = (N + 63) / 64;
    JV_REQUIRE(accept_stride_words >= 0, "search_flat_filtered: negative accept stride");
    JV_REQUIRE(accept_stride_words == 0 || accept_stride_words >= mask_words, "search_flat_filtered: accept stride %lld < %lld words",
               (long long)accept_stride_words, (long long)mask_words);
    if (Q == 0) return JV_OK;
    JV_REQUIRE(queries && out_ids && out_scores, "search_flat_filtered: NULL buffer");
    if (!accept_bits || N == 0) {   // no filter (or nothing to filter): the unfiltered search itself
        JV_TRY(jv_hip_search_flat(ctx, l, codes, vectors, queries, Q, vsf, topK, rerankK, id_base, out_ids, out_scores));
        if (accepted_out)
            for (int q = 0; q < Q; ++q) accepted_out[q] = N;
        return JV_OK;
    }
    if (N > 0x7fffffffLL) {
        set_error("search_flat_filtered: %lld rows do not fit an ordinal", (long long)N);
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(use_device(ctx->device));
    JV_TRY(jv_hip_luts_build(ctx, l, queries, Q, vsf, JV_DECODER_PQ));
    if (vsf == JV_COSINE) JV_TRY(ensure_code_norms(ctx, const_cast<jv_codes *>(codes)));
    const int M = codes->M;
    const int kvsf = to_kernel_vsf(vsf);
    const int k1 = rerank ? rerankK : topK;
    const bool shared = accept_stride_words == 0;
    const int masks = shared ? 1 : Q;
    const bool mq = shared && adc_mq_supported(M, codes->d_codes);

    const void *d_acc = nullptr;
    JV_TRY(stage_in(ctx, accept_bits, sizeof(uint64_t) * (size_t)(accept_stride_words * (masks - 1) + mask_words), ctx->h_in, ctx->d_gs_mask,
                    &d_acc));

    // ---------------- masks -> counts ----------------
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    FaScanParams sp{};
    sp.bits = (const uint64_t *)d_acc;
    sp.stride_words = accept_stride_words;
    sp.n = N;
    sp.blocks = fa_scan_blocks(N);
    JV_TRY(ctx->d_bin_work.reserve(al(sizeof(uint32_t) * (size_t)masks) + al(sizeof(uint32_t) * (size_t)masks * sp.blocks)));
    sp.totals = (uint32_t *)ctx->d_bin_work.ptr;
    sp.block_base = (uint32_t *)((char *)ctx->d_bin_work.ptr + al(sizeof(uint32_t) * (size_t)masks));
    FA_TRY(launch_flat_accept_count(ctx->stream, sp, sizeof(sp), masks), "the mask scan");
    // one small D2H + sync: the longest list sizes the lists and the score matrix
    JV_TRY(ctx->h_out.reserve(sizeof(uint32_t) * (size_t)masks));
    JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, sp.totals, sizeof(uint32_t) * (size_t)masks, hipMemcpyDeviceToHost, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    int64_t longest = 0, rows_sum = 0;
    for (int m = 0; m < masks; ++m) {
        const int64_t c = ((const uint32_t *)ctx->h_out.ptr)[m];
        longest = std::max(longest, c);
        rows_sum += c;
    }
    if (shared) rows_sum *= Q;
    if (accepted_out)
        for (int q = 0; q < Q; ++q) accepted_out[q] = ((const uint32_t *)ctx->h_out.ptr)[shared ? 0 : q];
    const int64_t L = std::max<int64_t>(64, (longest + 63) & ~(int64_t)63);
    sp.L = L;

    // queries per chunk: the chunk's Q x L score matrix stays under flat_acc_score_bytes, whole groups of four, at least one
    const long long budget = std::max<long long>(0, ctx_opt(ctx, "flat_acc_score_bytes", 1ll << 30));
    int64_t qc = budget / (int64_t)(sizeof(float) * L) / FA_P * FA_P;
    qc = std::min<int64_t>(std::max<int64_t>(qc, FA_P), Q);

    OutStage oi, osc;
    JV_TRY(stage_out_begin(ctx, out_ids, sizeof(int32_t) * (size_t)Q * topK, ctx->d_out, &oi));
    JV_TRY(stage_out_begin(ctx, out_scores, sizeof(float) * (size_t)Q * topK, ctx->d_in, &osc));

    // scratch3: [cand ids Q*k1][cand approx scores Q*k1][exact scores Q*k1][qnorm Q]  (jv_hip_search_flat's layout)
    const size_t c1 = (size_t)Q * k1;
    JV_TRY(ctx->d_scratch3.reserve(sizeof(int32_t) * c1 + sizeof(float) * c1 * 2 + sizeof(float) * (size_t)Q + 1024));
    int32_t *d_cand = (int32_t *)ctx->d_scratch3.ptr;
    float *d_cand_sc = (float *)(d_cand + c1);
    float *d_exact = d_cand_sc + c1;
    float *d_qnorm = d_exact + c1;
    int32_t *d_k1_ids = rerank ? d_cand : (int32_t *)oi.dev;
    float *d_k1_sc = rerank ? d_cand_sc : (float *)osc.dev;
    JV_TRY(ctx->d_scratch.reserve(topk_scratch_bytes(Q, std::max(k1, topK))));
    JV_TRY(ctx->d_scratch2.reserve(sizeof(float) * (size_t)qc * L));
    float *d_scores = (float *)ctx->d_scratch2.ptr;
    const int list_rows = mq ? 1 : (int)qc;
    JV_TRY(ctx->d_bin_cand.reserve(sizeof(int32_t) * (size_t)list_rows * L));
    sp.lists = (int32_t *)ctx->d_bin_cand.ptr;

    // ---------------- pass 1: the approximate top-k1 among the accepted rows ----------------
    if (mq) FA_TRY(launch_flat_accept_write(ctx->stream, sp, sizeof(sp), 1), "the list write-out");
    int chunks = 0;
    for (int64_t q_lo = 0; q_lo < Q; q_lo += qc, ++chunks) {
        const int nq = (int)std::min<int64_t>(qc, Q - q_lo);
        const float *luts_c = l->d_luts + (size_t)q_lo * M * kClusters;
        const float *bmag_c = l->d_bmag ? l->d_bmag + q_lo : nullptr;
        int32_t *ids_c = d_k1_ids + (size_t)q_lo * k1;
        float *sc_c = d_k1_sc + (size_t)q_lo * k1;
        if (mq) {
            {
                ProfScope ps(ctx, R_ADC);
                FaAdcParams ap{};
                ap.luts = luts_c; ap.bmag = bmag_c; ap.codes = codes->d_codes; ap.norms = codes->d_norms; ap.list = sp.lists; ap.out = d_scores;
                ap.n = N; ap.count = longest; ap.L = L; ap.Q = nq; ap.M = M;
                FA_TRY(launch_flat_accept_adc_list(ctx->stream, ap, sizeof(ap), kvsf, ctx->num_cus), "the list ADC scan");
            }
            // columns are list positions, ascending ordinals: the tie rule (smaller id first) survives the detour
            ProfScope ps(ctx, R_TOPK);
            JV_TRY(launch_topk(ctx->stream, ctx, d_scores, nullptr, nq, longest, L, 0, k1, ids_c, sc_c, ctx->d_scratch.ptr));
        } else {
            sp.first_mask = (int)q_lo;
            FA_TRY(launch_flat_accept_write(ctx->stream, sp, sizeof(sp), nq), "the list write-out");
            {
                ProfScope ps(ctx, R_ADC);
                JV_TRY(launch_adc_pitched(ctx->stream, ctx, luts_c, bmag_c, nq, M, kvsf, codes->d_codes, codes->d_norms, N, longest, L, sp.lists,
                                          d_scores));
            }
            ProfScope ps(ctx, R_TOPK);
            JV_TRY(launch_topk(ctx->stream, ctx, d_scores, sp.lists, nq, longest, L, 0, k1, ids_c, sc_c, ctx->d_scratch.ptr,
                               shared ? nullptr : sp.totals + q_lo));
        }
    }
    if (mq) {
        FaMapParams mp{};
        mp.list = sp.lists; mp.ids = d_k1_ids; mp.cells = (int64_t)c1; mp.count = longest;
        FA_TRY(launch_flat_accept_map(ctx->stream, mp, sizeof(mp)), "the position map");
    }
    ctx_stat_add(ctx, "flat_acc_calls", 1);
    ctx_stat_add(ctx, "flat_acc_queries", Q);
    ctx_stat_add(ctx, "flat_acc_rows", rows_sum);
    ctx_stat_add(ctx, "flat_acc_chunks", chunks);
    if (shared && !mq) ctx_stat_add(ctx, "flat_acc_generic", 1);

    // ---------------- pass 2: jv_hip_search_flat's ----------------
    if (rerank) {
        JV_TRY(rerank_gather(ctx, vectors, l->d_raw_queries, Q, vsf, d_cand, k1, d_exact, d_qnorm));
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_exact, d_cand, Q, k1, k1, 0, topK, (int32_t *)oi.dev, (float *)osc.dev, ctx->d_scratch.ptr));
    }
    JV_TRY(launch_add_id_base(ctx->stream, (int32_t *)oi.dev, (int64_t)Q * topK, id_base));
    JV_TRY(stage_out_end(ctx, oi));
    return stage_out_end(ctx, osc);
}

}  // extern "C"
