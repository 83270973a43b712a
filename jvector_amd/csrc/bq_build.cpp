// bq_build.cpp — host side of the build-time scoring over binary-quantized vectors (include/jvector_bq_build.h): argument checks,
// staging, the LDS limit and the launch of the batched robust prune (k_bq_retain.hip), and the construction-time search from stored
// rows — a gather of rows[nodes[q]] into the query words, then jv_hip_bq_graph_search's own second half (bq_graph.cpp bq_graph_finish).
#include <algorithm>

#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"
#include "../../include/jvector_bq_build.h"

namespace jv {

// query words of item q = row nodes[q]; an ordinal outside the rows gives zero words (the item is blanked afterwards)
__global__ __launch_bounds__(256) void bq_gather_rows_kernel(const uint64_t *rows, int64_t n_rows, int W, const int32_t *nodes, int64_t total, uint64_t *qwords)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t q = t / W;
    const int w = (int)(t - q * W);
    const int32_t nd = nodes[q];
    uint64_t v = 0;
    if (nd >= 0 && nd < n_rows) v = rows[(int64_t)nd * W + w];
    qwords[t] = v;
}

int launch_bq_gather_rows(hipStream_t s, const uint64_t *d_rows, int64_t n_rows, int W, const int32_t *d_nodes, int64_t Q, uint64_t *d_out)
{
    const int64_t total = Q * W;
    if (total == 0) return JV_OK;
    hipLaunchKernelGGL(bq_gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_rows, n_rows, W, d_nodes, total, d_out);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

__global__ __launch_bounds__(256) void bq_blank_rows_kernel(const int32_t *nodes, int64_t n_rows, int Q, int K, int32_t *ids, float *scores, long long *stats)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)Q * K) return;
    const int64_t q = t / K;
    const int32_t nd = nodes[q];
    if (nd >= 0 && nd < n_rows) return;
    ids[t] = -1;
    scores[t] = -__builtin_inff();
    if (t == q * K) stats[2 * q] = stats[2 * q + 1] = 0;
}

int launch_bq_blank_rows(hipStream_t s, const int32_t *d_nodes, int64_t n_rows, int Q, int K, int32_t *d_ids, float *d_scores, long long *d_stats)
{
    const int64_t total = (int64_t)Q * K;
    if (total == 0) return JV_OK;
    hipLaunchKernelGGL(bq_blank_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_nodes, n_rows, Q, K, d_ids, d_scores, d_stats);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

static size_t bd_lds_limit(const jv_ctx *ctx) { return std::min<size_t>(65536, ctx->lds_per_block); }

// largest C whose rows fit the prune kernel's LDS block beside the 64 selected rows (bd_lds_bytes)
static int bd_max_candidates(const jv_ctx *ctx, int W)
{
    const size_t limit = bd_lds_limit(ctx), fixed = sizeof(uint64_t) * 64 * (size_t)W;
    if (fixed >= limit) return 0;
    return (int)std::min<size_t>(BD_MAX_CANDIDATES, (limit - fixed) / (sizeof(uint64_t) * (size_t)W + 8));
}

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_bq_retain_diverse_max_candidates(jv_ctx *ctx, const jv_bq_vectors *bq, int maxDegree, int *out)
{
    clear_error();
    JV_REQUIRE(ctx && bq && out, "bq_retain_diverse_max_candidates: NULL argument");
    JV_REQUIRE(maxDegree >= 1, "bq_retain_diverse_max_candidates: maxDegree must be positive");
    *out = (maxDegree > 64 || bq->D > kBqMaxDim) ? 0 : bd_max_candidates(ctx, bq->W);
    return JV_OK;
}

int jv_hip_bq_retain_diverse(jv_ctx *ctx, const jv_bq_vectors *bq, int P, int C, const int32_t *cand_nodes, const float *cand_scores,
                             const int32_t *cand_count, const int32_t *diverse_before, int maxDegree, float alpha, int32_t *selected_out,
                             int32_t *n_selected_out, float *short_edges_out)
{
    clear_error();
    JV_REQUIRE(ctx && bq, "bq_retain_diverse: NULL argument");
    JV_REQUIRE(bq->device == ctx->device, "bq_retain_diverse: the BQ vectors live on device %d, the context on %d", bq->device, ctx->device);
    JV_REQUIRE(P >= 0, "bq_retain_diverse: negative node count");
    JV_REQUIRE(C >= 1, "bq_retain_diverse: C must be positive");
    JV_REQUIRE(maxDegree >= 1, "bq_retain_diverse: maxDegree must be positive");
    // an alpha below 1, or NaN, means no round; above 64 (infinity included) the kernel's loop over the alpha steps has no useful end:
    // past 2^22 the f32 step of 0.2 no longer moves currentAlpha at all.  jv_hip_retain_diverse's upper bound.
    JV_REQUIRE(!(alpha > BD_MAX_ALPHA), "bq_retain_diverse: alpha %g above %g", (double)alpha, (double)BD_MAX_ALPHA);
    if (P == 0) return JV_OK;
    JV_REQUIRE(cand_nodes && cand_scores && selected_out && n_selected_out, "bq_retain_diverse: NULL buffer");
    if (maxDegree > 64) {
        set_error("bq_retain_diverse: maxDegree %d above 64", maxDegree);
        return JV_ERR_UNSUPPORTED;
    }
    if (bq->D > kBqMaxDim) {
        set_error("bq_retain_diverse: dimension %d above %d", bq->D, kBqMaxDim);
        return JV_ERR_UNSUPPORTED;
    }
    if (C > bd_max_candidates(ctx, bq->W)) {
        set_error("bq_retain_diverse: %d candidates of %d words above the %d the prune kernel's LDS block holds; prune in smaller candidate lists", C,
                  bq->W, bd_max_candidates(ctx, bq->W));
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(use_device(ctx->device));
    CtxBusy busy(ctx);
    JV_REQUIRE(busy.ok, "bq_retain_diverse: the context is in use by another thread");
    const size_t cells = (size_t)P * C;
    const void *d_nodes = nullptr, *d_scores = nullptr, *d_count = nullptr, *d_before = nullptr;
    // four inputs, one pinned staging buffer: staged one after another into distinct device buffers
    JV_TRY(stage_in(ctx, cand_nodes, sizeof(int32_t) * cells, ctx->h_in, ctx->d_in, &d_nodes));
    JV_TRY(stage_in(ctx, cand_scores, sizeof(float) * cells, ctx->h_in, ctx->d_scratch2, &d_scores));
    if (cand_count) JV_TRY(stage_in(ctx, cand_count, sizeof(int32_t) * (size_t)P, ctx->h_in, ctx->d_scratch3, &d_count));
    if (diverse_before) JV_TRY(stage_in(ctx, diverse_before, sizeof(int32_t) * (size_t)P, ctx->h_in, ctx->d_gs_mask, &d_before));
    // outputs: selected [P][maxDegree] + n_selected [P] + short_edges [P] in one device block
    const size_t sel_bytes = sizeof(int32_t) * (size_t)P * maxDegree, cnt_bytes = sizeof(int32_t) * (size_t)P;
    const size_t o_cnt = (sel_bytes + 255) & ~(size_t)255, o_se = (o_cnt + cnt_bytes + 255) & ~(size_t)255;
    JV_TRY(ctx->d_out.reserve(o_se + sizeof(float) * (size_t)P));
    char *base = (char *)ctx->d_out.ptr;
    BdParams p{};
    p.rows = bq->d_rows;
    p.n = bq->count;
    p.D = bq->D;
    p.W = bq->W;
    p.cand_nodes = (const int32_t *)d_nodes;
    p.cand_scores = (const float *)d_scores;
    p.cand_count = (const int32_t *)d_count;
    p.diverse_before = (const int32_t *)d_before;
    p.P = P;
    p.C = C;
    p.maxDegree = maxDegree;
    p.alpha = alpha;
    p.selected_out = (int32_t *)base;
    p.n_selected_out = (int32_t *)(base + o_cnt);
    p.short_edges_out = (float *)(base + o_se);
    {
        ProfScope ps(ctx, R_PRUNE);
        JV_TRY(launch_bq_retain(ctx->stream, ctx, p));
    }
    JV_HIP_CHECK(hipMemcpyAsync(selected_out, p.selected_out, sel_bytes, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipMemcpyAsync(n_selected_out, p.n_selected_out, cnt_bytes, hipMemcpyDefault, ctx->stream));
    if (short_edges_out) JV_HIP_CHECK(hipMemcpyAsync(short_edges_out, p.short_edges_out, sizeof(float) * (size_t)P, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return JV_OK;
}

int jv_hip_bq_graph_search_nodes(jv_ctx *ctx, const jv_graph *g, const jv_bq_vectors *bq, const int32_t *nodes, int Q, int topK,
                                 int exclude_self, int32_t *out_ids, float *out_scores, int64_t *stats)
{
    clear_error();
    BqGraphCall c{};
    c.who = "bq_graph_search_nodes";
    c.g = g;
    c.bq = bq;
    c.Q = Q;
    c.vsf = JV_DOT_PRODUCT;   // (read by a rerank only: there is none)
    c.topK = c.rerankK = topK;
    c.out_ids = out_ids;
    c.out_scores = out_scores;
    c.stats = stats;
    JV_TRY(bq_graph_begin(ctx, c, nodes));
    if (c.empty) return JV_OK;
    const bool on_device = is_device_ptr(nodes);
    if (!on_device)
        for (int q = 0; q < Q; ++q)
            JV_REQUIRE(nodes[q] >= 0 && nodes[q] < bq->count, "bq_graph_search_nodes: ordinal %d of item %d outside the %lld BQ rows", nodes[q], q,
                       (long long)bq->count);
    CtxBusy busy(ctx);
    JV_REQUIRE(busy.ok, "bq_graph_search_nodes: the context is in use by another thread");
    const void *d_nodes = nullptr;
    JV_TRY(stage_in(ctx, nodes, sizeof(int32_t) * (size_t)Q, ctx->h_in, ctx->d_in, &d_nodes));
    const int64_t total = (int64_t)Q * bq->W;
    JV_TRY(ctx->d_bin_work.reserve(sizeof(uint64_t) * (size_t)total));
    uint64_t *d_qw = (uint64_t *)ctx->d_bin_work.ptr;
    {
        ProfScope ps(ctx, R_ENCODE);
        JV_TRY(launch_bq_gather_rows(ctx->stream, bq->d_rows, bq->count, bq->W, (const int32_t *)d_nodes, Q, d_qw));
    }
    return bq_graph_finish(ctx, c, nullptr, d_qw, exclude_self ? (const int32_t *)d_nodes : nullptr, on_device ? (const int32_t *)d_nodes : nullptr);
}

}  // extern "C"
