// bq_graph.cpp — host side of the graph search over binary-quantized vectors (include/jvector_bq_graph.h): argument checks, the
// workspace, the launch of k_bq_gsearch.hip, the pass that runs again the queries that outgrew the first attempt's fixed-size
// structures, and the exact rerank + top-K through the launchers of jv_hip_graph_search / jv_hip_bq_search_flat (rerank_gather ->
// launch_exact_gather, launch_topk): reranked results carry the same bits.
#include <algorithm>
#include <vector>

#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"
#include "bg_params.h"
#include "../../include/jvector_bq_graph.h"

namespace jv {

constexpr int kBgMaxCandCap = 4096;
constexpr size_t kBgLdsLimit = 65536;
constexpr size_t kBgScratchBudget = (size_t)1 << 30;   // per-worker visited tables / bitmaps + spill slices of one launch

struct BgPlan {
    int vcap_log2 = 0, cand_cap = 0, spill_cap = 0;
};

static int ceil_log2(long long v)
{
    int b = 0;
    while ((1ll << b) < v) ++b;
    return b;
}

// candidates' LDS tier: bq_gs_cand_cap, else twice rerankK rounded up to a power of two within [512, 2048]
static int bg_cand_cap(const jv_ctx *ctx, int rerankK)
{
    long long c = ctx_opt(ctx, "bq_gs_cand_cap", 0);
    if (c <= 0) c = std::min(2048ll, std::max(512ll, 1ll << ceil_log2(2ll * rerankK)));
    return (int)std::min<long long>(kBgMaxCandCap, std::max<long long>(BG_MIN_CAND_CAP, c));
}

static size_t bg_lds_limit(const jv_ctx *ctx) { return std::min(kBgLdsLimit, ctx->lds_per_block); }

// largest rerankK whose result list fits next to the candidate tier, the samples and the widest query (generic form) — the visited table
// moves to global memory when LDS has no room for it, so it takes no share here
static int bg_max_rerank_k(const jv_ctx *ctx, int cand_cap)
{
    const size_t fixed = sizeof(long long) * ((size_t)cand_cap + 64 + (size_t)(kBqMaxDim + 63) / 64);
    return (int)((bg_lds_limit(ctx) - fixed) / sizeof(long long));
}

// the first attempt: a table for 48 visited nodes per kept result + 2048 at half load (bq_gs_vcap_log2 overrides), never more than the
// graph can fill; in LDS when it is small and fits beside the queues, else in global memory
static BgPlan bg_plan(const jv_ctx *ctx, int rerankK, int W, long long n_nodes)
{
    BgPlan pl;
    pl.cand_cap = bg_cand_cap(ctx, rerankK);
    long long v = ctx_opt(ctx, "bq_gs_vcap_log2", 0);
    if (v <= 0) v = std::min(ceil_log2(2 * (48ll * rerankK + 2048)), ceil_log2(2 * (n_nodes + 64)));
    pl.vcap_log2 = (int)std::min<long long>(BG_MAX_VCAP_LOG2, std::max<long long>(BG_MIN_VCAP_LOG2, v));
    if (pl.vcap_log2 <= BG_VIS_LDS_MAX_LOG2 && bq_graph_lds_bytes(rerankK, pl.cand_cap, W, pl.vcap_log2) > bg_lds_limit(ctx))
        pl.vcap_log2 = BG_VIS_LDS_MAX_LOG2 + 1;
    // live candidates + evicted results never exceed the visited nodes: a slice the table cannot outgrow, capped at 16 LDS tiers
    pl.spill_cap = (int)std::min<long long>((1ll << pl.vcap_log2) / 2 + 64, 16ll * pl.cand_cap);
    return pl;
}

// Everything jv_hip_bq_graph_search checks before it touches the stream, and the graph's device view (c.p.lv, entry, n_nodes).
// `input` is the caller's query buffer (floats or ordinals): only its presence is looked at.
int bq_graph_begin(jv_ctx *ctx, BqGraphCall &c, const void *input)
{
    c.empty = false;
    const jv_graph *g = c.g;
    const jv_bq_vectors *bq = c.bq;
    const jv_vectors *vectors = c.vectors;
    const int Q = c.Q, topK = c.topK, rerankK = c.rerankK;
    const uint64_t *accept_bits = c.accept_bits;
    const int64_t accept_stride_words = c.accept_stride_words;
    JV_REQUIRE(ctx && g && bq, "%s: NULL argument", c.who);
    JV_REQUIRE(bq->device == ctx->device, "%s: the BQ vectors live on device %d, the context on %d", c.who, bq->device, ctx->device);
    JV_REQUIRE(Q >= 0, "%s: negative query count", c.who);
    JV_REQUIRE(topK >= 1, "%s: topK must be positive", c.who);
    JV_REQUIRE(rerankK >= topK, "rerankK %d must be >= topK %d", rerankK, topK);
    if (vectors) {
        JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", c.who, vectors->device, ctx->device);
        JV_REQUIRE(vectors->D == bq->D, "%s: vectors of dimension %d, BQ of dimension %d", c.who, vectors->D, bq->D);
    }
    JV_TRY(use_device(ctx->device));
    BgParams &p = c.p;
    p = BgParams{};
    GraphDeviceView gv;
    {
        const int rc = graph_device_view(ctx, g, p.lv, &gv);
        if (rc != JV_OK) return rc;
    }
    const int64_t N = gv.n_nodes;
    JV_REQUIRE(bq->count >= N, "%s: %lld BQ rows for a graph of %lld nodes", c.who, (long long)bq->count, (long long)N);
    JV_REQUIRE(!vectors || vectors->count >= N, "%s: %lld vectors for a graph of %lld nodes", c.who, vectors ? (long long)vectors->count : 0ll,
               (long long)N);
    const int64_t mask_words = (N + 63) / 64;
    JV_REQUIRE(accept_stride_words >= 0 && (!accept_bits || accept_stride_words == 0 || accept_stride_words >= mask_words),
               "%s: accept_stride_words %lld is smaller than the %lld words one mask needs", c.who, (long long)accept_stride_words,
               (long long)mask_words);
    if (Q == 0) {
        c.empty = true;
        return JV_OK;
    }
    JV_REQUIRE(input && c.out_ids && c.out_scores, "%s: NULL buffer", c.who);
    const int D = bq->D, W = bq->W;
    if (gv.max_degree > kMaxGraphDegree) {
        set_error("%s: degree %d above %d", c.who, gv.max_degree, kMaxGraphDegree);
        return JV_ERR_UNSUPPORTED;
    }
    if (D > kBqMaxDim) {
        set_error("%s: dimension %d above %d", c.who, D, kBqMaxDim);
        return JV_ERR_UNSUPPORTED;
    }
    const BgPlan pl = bg_plan(ctx, rerankK, W, N);
    if (rerankK > bg_max_rerank_k(ctx, bg_cand_cap(ctx, 1 << 20)) || bq_graph_lds_bytes(rerankK, pl.cand_cap, W, pl.vcap_log2) > bg_lds_limit(ctx)) {
        set_error("%s: rerankK %d above the %d the traversal kernel's LDS block holds", c.who, rerankK, bg_max_rerank_k(ctx, bg_cand_cap(ctx, 1 << 20)));
        return JV_ERR_UNSUPPORTED;
    }
    p.entry_node = gv.entry_node;
    p.entry_level = gv.entry_level;
    p.n_nodes = (int32_t)N;
    return JV_OK;
}

// The search from the encoded queries on: d_qw holds Q x W query words, written by work already queued on the context's stream
// (the caller holds the context).  d_q: the float queries on the device, read by the rerank only (c.vectors != NULL).  d_exclude:
// BgParams::exclude.  d_blank_nodes (nullable): Q ordinals; an item whose ordinal lies outside the BQ rows gets a (-1, -INFINITY) row and
// zero counters (launch_bq_blank_rows).
int bq_graph_finish(jv_ctx *ctx, const BqGraphCall &c, const float *d_q, const uint64_t *d_qw, const int32_t *d_exclude,
                    const int32_t *d_blank_nodes)
{
    const jv_bq_vectors *bq = c.bq;
    const jv_vectors *vectors = c.vectors;
    const int Q = c.Q, topK = c.topK, rerankK = c.rerankK;
    const jv_vsf vsf = c.vsf;
    const int64_t accept_stride_words = c.accept_stride_words;
    int64_t *stats = c.stats;
    BgParams p = c.p;
    const int64_t N = p.n_nodes;
    const int64_t mask_words = (N + 63) / 64;
    const int D = bq->D, W = bq->W;
    const BgPlan pl = bg_plan(ctx, rerankK, W, N);

    // ---- inputs ----
    const void *d_acc = nullptr;
    if (c.accept_bits)
        JV_TRY(stage_in(ctx, c.accept_bits, sizeof(uint64_t) * (size_t)(accept_stride_words * (Q - 1) + mask_words), ctx->h_in, ctx->d_scratch2,
                        &d_acc));

    // ---- the first attempt's workers and their scratch ----
    const size_t lds = bq_graph_lds_bytes(rerankK, pl.cand_cap, W, pl.vcap_log2);
    const bool vis_global = pl.vcap_log2 > BG_VIS_LDS_MAX_LOG2;
    const size_t per_worker = sizeof(long long) * (size_t)pl.spill_cap + (vis_global ? ((size_t)4 << pl.vcap_log2) : 0);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / std::max<size_t>(lds, 1)));
    const int workers = (int)std::max<long long>(1, std::min<long long>({(long long)Q, (long long)ctx->num_cus * per_cu,
                                                                        (long long)(kBgScratchBudget / per_worker)}));
    JV_TRY(ctx->d_gs_spill.reserve(sizeof(long long) * (size_t)pl.spill_cap * (size_t)workers));
    if (vis_global) JV_TRY(ctx->d_gs_visited.reserve(((size_t)4 << pl.vcap_log2) * (size_t)workers));

    // ---- per-query staging: [ids Q x rerankK][scores Q x rerankK][stats Q x 2][status Q][qmap Q][qnorm Q][counter] ----
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_ids = carve(sizeof(int32_t) * (size_t)Q * rerankK), o_sc = carve(sizeof(float) * (size_t)Q * rerankK);
    const size_t o_stats = carve(sizeof(long long) * 2 * (size_t)Q), o_status = carve(sizeof(int32_t) * (size_t)Q);
    const size_t o_qmap = carve(sizeof(int32_t) * (size_t)Q), o_qn = carve(sizeof(float) * (size_t)Q), o_counter = carve(sizeof(uint32_t));
    JV_TRY(ctx->d_gs_out.reserve(off));
    char *base = (char *)ctx->d_gs_out.ptr;
    int32_t *d_cand = (int32_t *)(base + o_ids);
    float *d_cand_sc = (float *)(base + o_sc);
    long long *d_stats = (long long *)(base + o_stats);
    int32_t *d_status = (int32_t *)(base + o_status);
    int32_t *d_qmap = (int32_t *)(base + o_qmap);
    float *d_qnorm = (float *)(base + o_qn);
    uint32_t *d_counter = (uint32_t *)(base + o_counter);

    p.rows = bq->d_rows;
    p.qwords = d_qw;
    p.D = D;
    p.W = W;
    p.Q = Q;
    p.rerankK = rerankK;
    p.accept = (const unsigned long long *)d_acc;
    p.accept_stride = accept_stride_words;
    p.exclude = d_exclude;
    p.vcap_log2 = pl.vcap_log2;
    p.visited = vis_global ? (int32_t *)ctx->d_gs_visited.ptr : nullptr;
    p.cand_cap = pl.cand_cap;
    p.spill = (long long *)ctx->d_gs_spill.ptr;
    p.spill_cap = pl.spill_cap;
    p.out_ids = d_cand;
    p.out_scores = d_cand_sc;
    p.out_stats = d_stats;
    p.out_status = d_status;
    p.next_query = d_counter;

    JV_HIP_CHECK(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), ctx->stream));
    {
        ProfScope ps(ctx, R_GSEARCH);
        JV_TRY(launch_bq_graph_search(ctx->stream, p, workers, false));
    }

    // ---- queries that outgrew the table or the spill slice: once more with structures that hold every node ----
    std::vector<int32_t> redo;
    {
        JV_TRY(ctx->h_out.reserve(sizeof(int32_t) * (size_t)Q));
        JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, d_status, sizeof(int32_t) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const int32_t *hs = (const int32_t *)ctx->h_out.ptr;
        for (int q = 0; q < Q; ++q)
            if (hs[q] != GS_OK) redo.push_back(q);
    }
    if (!redo.empty()) {
        const int R = (int)redo.size();
        const long long bitmap_words = ((N + 31) / 32 + 3) / 4 * 4;
        const int spill2 = (int)std::min<long long>(N + 64, 0x7fffffff);
        const size_t per2 = sizeof(uint32_t) * (size_t)bitmap_words + sizeof(long long) * (size_t)spill2;
        const size_t lds2 = bq_graph_lds_bytes(rerankK, pl.cand_cap, W, 0);
        const int per_cu2 = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / std::max<size_t>(lds2, 1)));
        const int workers2 = (int)std::max<long long>(1, std::min<long long>({(long long)R, (long long)ctx->num_cus * per_cu2,
                                                                             (long long)(kBgScratchBudget / per2)}));
        JV_TRY(ctx->d_gs_visited.reserve(sizeof(uint32_t) * (size_t)bitmap_words * (size_t)workers2));
        JV_TRY(ctx->d_gs_spill.reserve(sizeof(long long) * (size_t)spill2 * (size_t)workers2));
        memcpy(ctx->h_out.ptr, redo.data(), sizeof(int32_t) * (size_t)R);
        JV_HIP_CHECK(hipMemcpyAsync(d_qmap, ctx->h_out.ptr, sizeof(int32_t) * (size_t)R, hipMemcpyHostToDevice, ctx->stream));
        JV_HIP_CHECK(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), ctx->stream));
        BgParams p2 = p;
        p2.qmap = d_qmap;
        p2.Q = R;
        p2.vcap_log2 = 0;
        p2.visited = nullptr;
        p2.bitmap = (uint32_t *)ctx->d_gs_visited.ptr;
        p2.bitmap_words = bitmap_words;
        p2.spill = (long long *)ctx->d_gs_spill.ptr;
        p2.spill_cap = spill2;
        {
            ProfScope ps(ctx, R_GSEARCH);
            JV_TRY(launch_bq_graph_search(ctx->stream, p2, workers2, true));
        }
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // h_out is reused below
        JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, d_status, sizeof(int32_t) * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const int32_t *hs = (const int32_t *)ctx->h_out.ptr;
        for (int q : redo)
            if (hs[q] != GS_OK) {   // cannot happen: the structures hold every node; never hand back a truncated answer
                set_error("%s: query %d did not finish in the roomy form (status %d)", c.who, q, hs[q]);
                return JV_ERR_HIP;
            }
    }

    // ---- reranking :471-507 on the device-resident candidates ----
    OutStage oi, osc;
    JV_TRY(stage_out_begin(ctx, c.out_ids, sizeof(int32_t) * (size_t)Q * topK, ctx->d_out, &oi));
    JV_TRY(stage_out_begin(ctx, c.out_scores, sizeof(float) * (size_t)Q * topK, ctx->d_scratch3, &osc));
    JV_TRY(ctx->d_scratch.reserve(topk_scratch_bytes(Q, std::max(rerankK, topK))));
    if (vectors) JV_TRY(rerank_gather(ctx, vectors, d_q, Q, vsf, d_cand, rerankK, d_cand_sc, d_qnorm));
    {
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_cand_sc, d_cand, Q, rerankK, rerankK, 0, topK, (int32_t *)oi.dev, (float *)osc.dev,
                           ctx->d_scratch.ptr));
    }
    if (d_blank_nodes)
        JV_TRY(launch_bq_blank_rows(ctx->stream, d_blank_nodes, bq->count, Q, topK, (int32_t *)oi.dev, (float *)osc.dev, d_stats));
    JV_TRY(stage_out_end(ctx, oi));
    JV_TRY(stage_out_end(ctx, osc));
    if (stats) {   // (after stage_out_end: it stages through h_out too)
        JV_TRY(ctx->h_out.reserve(sizeof(long long) * 2 * (size_t)Q));
        JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, d_stats, sizeof(long long) * 2 * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const long long *h = (const long long *)ctx->h_out.ptr;
        for (int64_t i = 0; i < 2 * (int64_t)Q; ++i) stats[i] = h[i];
    } else {
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    ctx_stat_add(ctx, "bq_gs_calls", 1);
    ctx_stat_add(ctx, "bq_gs_queries", Q);
    ctx_stat_add(ctx, "bq_gs_queries_retried", (long long)redo.size());
    ctx_stat_set(ctx, "bq_gs_last_vcap_log2", pl.vcap_log2);
    ctx_stat_set(ctx, "bq_gs_last_workers", workers);
    return JV_OK;
}

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_bq_graph_max_rerank_k(jv_ctx *ctx, const jv_graph *g, int *out)
{
    clear_error();
    JV_REQUIRE(ctx && g && out, "bq_graph_max_rerank_k: NULL argument");
    *out = bg_max_rerank_k(ctx, bg_cand_cap(ctx, 1 << 20));
    return JV_OK;
}

int jv_hip_bq_graph_search(jv_ctx *ctx, const jv_graph *g, const jv_bq_vectors *bq, const jv_vectors *vectors, const float *queries, int Q,
                           jv_vsf vsf, int topK, int rerankK, const uint64_t *accept_bits, int64_t accept_stride_words, int32_t *out_ids,
                           float *out_scores, int64_t *stats)
{
    clear_error();
    BqGraphCall c{};
    c.who = "bq_graph_search";
    c.g = g;
    c.bq = bq;
    c.vectors = vectors;
    c.Q = Q;
    c.vsf = vsf;
    c.topK = topK;
    c.rerankK = rerankK;
    c.accept_bits = accept_bits;
    c.accept_stride_words = accept_stride_words;
    c.out_ids = out_ids;
    c.out_scores = out_scores;
    c.stats = stats;
    JV_TRY(bq_graph_begin(ctx, c, queries));
    if (c.empty) return JV_OK;
    CtxBusy busy(ctx);
    JV_REQUIRE(busy.ok, "bq_graph_search: the context is in use by another thread");
    const void *d_q = nullptr;
    JV_TRY(stage_in(ctx, queries, sizeof(float) * (size_t)Q * bq->D, ctx->h_in, ctx->d_in, &d_q));
    JV_TRY(ctx->d_bin_work.reserve(sizeof(uint64_t) * (size_t)Q * bq->W));
    uint64_t *d_qw = (uint64_t *)ctx->d_bin_work.ptr;
    {
        ProfScope ps(ctx, R_ENCODE);
        JV_TRY(launch_bq_encode(ctx->stream, (const float *)d_q, Q, bq->D, bq->W, 0, d_qw));
    }
    return bq_graph_finish(ctx, c, (const float *)d_q, d_qw, nullptr, nullptr);
}

}  // extern "C"
