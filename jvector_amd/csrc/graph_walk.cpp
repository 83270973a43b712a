// graph_walk.cpp — the host side the one-wave graph walks share (gw_body.h; front ends: bq_graph.cpp over BQ rows, exact_graph.cpp
// over float rows): the checks both make, the plan of the first attempt, the workspace, the launch, the pass that runs again the
// queries that outgrew the first attempt's fixed-size structures, the top-K through launch_topk, the outputs and the counters.
#include <algorithm>
#include <string>
#include <vector>

#include "jv_device.h"
#include "jv_internal.h"
#include "gw_params.h"

namespace jv {

constexpr int kGwMaxCandCap = 4096;
constexpr size_t kGwLdsLimit = 65536;
constexpr size_t kGwScratchBudget = (size_t)1 << 30;   // per-worker visited tables / bitmaps + spill slices of one launch

struct GwPlan {
    int vcap_log2 = 0, cand_cap = 0, spill_cap = 0;
};

static int ceil_log2(long long v)
{
    int b = 0;
    while ((1ll << b) < v) ++b;
    return b;
}

static long long gw_opt(const jv_ctx *ctx, const GwFront &f, const char *name) { return ctx_opt(ctx, (std::string(f.prefix) + name).c_str(), 0); }

// candidates' LDS tier: <prefix>_cand_cap, else twice K rounded up to a power of two within [512, 2048]
static int gw_cand_cap(const jv_ctx *ctx, const GwFront &f, int K)
{
    long long c = gw_opt(ctx, f, "_cand_cap");
    if (c <= 0) c = std::min(2048ll, std::max(512ll, 1ll << ceil_log2(2ll * K)));
    return (int)std::min<long long>(kGwMaxCandCap, std::max<long long>(BG_MIN_CAND_CAP, c));
}

static size_t gw_lds_limit(const jv_ctx *ctx) { return std::min(kGwLdsLimit, ctx->lds_per_block); }

// next to the widest candidate tier and the front end's fixed share — the visited table moves to global memory when LDS has no room
// for it, so it takes no share here
int gw_max_k(const jv_ctx *ctx, const GwFront &f) { return (int)((gw_lds_limit(ctx) - f.fixed_lds(gw_cand_cap(ctx, f, 1 << 20))) / sizeof(long long)); }

// the first attempt: a table for 48 visited nodes per kept result + 2048 at half load (<prefix>_vcap_log2 overrides), never more than the
// graph can fill; in LDS when it is small and fits beside the rest of the block, else in global memory
static GwPlan gw_plan(const jv_ctx *ctx, const GwFront &f, int K, long long n_nodes)
{
    GwPlan pl;
    pl.cand_cap = gw_cand_cap(ctx, f, K);
    long long v = gw_opt(ctx, f, "_vcap_log2");
    if (v <= 0) v = std::min(ceil_log2(2 * (48ll * K + 2048)), ceil_log2(2 * (n_nodes + 64)));
    pl.vcap_log2 = (int)std::min<long long>(BG_MAX_VCAP_LOG2, std::max<long long>(BG_MIN_VCAP_LOG2, v));
    if (pl.vcap_log2 <= BG_VIS_LDS_MAX_LOG2 && f.lds_bytes(K, pl.cand_cap, pl.vcap_log2) > gw_lds_limit(ctx)) pl.vcap_log2 = BG_VIS_LDS_MAX_LOG2 + 1;
    // live candidates + evicted results never exceed the visited nodes: a slice the table cannot outgrow, capped at 16 LDS tiers
    pl.spill_cap = (int)std::min<long long>((1ll << pl.vcap_log2) / 2 + 64, 16ll * pl.cand_cap);
    return pl;
}

static int gw_workers(const jv_ctx *ctx, size_t lds, long long items, size_t per_worker)
{
    // LDS sets the waves of a CU (160 KB on gfx950), at most 16 workgroups; every worker owns a scratch slice
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / std::max<size_t>(lds, 1)));
    return (int)std::max<long long>(1, std::min<long long>({items, (long long)ctx->num_cus * per_cu, (long long)(kGwScratchBudget / per_worker)}));
}

int gw_check_counts(const GwCall &c, const GwFront &f)
{
    JV_REQUIRE(c.Q >= 0, "%s: negative query count", c.who);
    JV_REQUIRE(c.topK >= 1, "%s: topK must be positive", c.who);
    JV_REQUIRE(c.K >= c.topK, "%s %d must be >= topK %d", f.k_name, c.K, c.topK);
    return JV_OK;
}

int gw_begin(jv_ctx *ctx, const GwCall &c, const jv_graph *g, GwParams &p, GraphDeviceView *gv)
{
    JV_TRY(use_device(ctx->device));
    JV_TRY(graph_device_view(ctx, g, p.lv, gv));
    p.entry_node = gv->entry_node;
    p.entry_level = gv->entry_level;
    p.n_nodes = (int32_t)gv->n_nodes;
    const int64_t mask_words = (gv->n_nodes + 63) / 64;
    JV_REQUIRE(c.accept_stride_words >= 0 && (!c.accept_bits || c.accept_stride_words == 0 || c.accept_stride_words >= mask_words),
               "%s: accept_stride_words %lld is smaller than the %lld words one mask needs", c.who, (long long)c.accept_stride_words,
               (long long)mask_words);
    return JV_OK;
}

int gw_admit(const jv_ctx *ctx, const GwCall &c, const GwFront &f, int max_degree, int64_t n_nodes)
{
    if (max_degree > kMaxGraphDegree) {
        set_error("%s: degree %d above %d", c.who, max_degree, kMaxGraphDegree);
        return JV_ERR_UNSUPPORTED;
    }
    const GwPlan pl = gw_plan(ctx, f, c.K, n_nodes);
    const int max_k = gw_max_k(ctx, f);
    if (c.K > max_k || f.lds_bytes(c.K, pl.cand_cap, pl.vcap_log2) > gw_lds_limit(ctx)) {
        set_error("%s: %s %d above the %d the traversal kernel's LDS block holds", c.who, f.k_name, c.K, max_k);
        return JV_ERR_UNSUPPORTED;
    }
    return JV_OK;
}

int gw_run(jv_ctx *ctx, const GwCall &c, const GwFront &f, GwParams p)
{
    const int Q = c.Q, topK = c.topK, K = c.K;
    const int64_t N = p.n_nodes;
    const int64_t mask_words = (N + 63) / 64;
    const GwPlan pl = gw_plan(ctx, f, K, N);

    const void *d_acc = nullptr;
    if (c.accept_bits)
        JV_TRY(stage_in(ctx, c.accept_bits, sizeof(uint64_t) * (size_t)(c.accept_stride_words * (Q - 1) + mask_words), ctx->h_in, ctx->d_scratch2,
                        &d_acc));

    // ---- the first attempt's workers and their scratch ----
    const bool vis_global = pl.vcap_log2 > BG_VIS_LDS_MAX_LOG2;
    const size_t per_worker = sizeof(long long) * (size_t)pl.spill_cap + (vis_global ? ((size_t)4 << pl.vcap_log2) : 0);
    const int workers = gw_workers(ctx, f.lds_bytes(K, pl.cand_cap, pl.vcap_log2), Q, per_worker);
    JV_TRY(ctx->d_gs_spill.reserve(sizeof(long long) * (size_t)pl.spill_cap * (size_t)workers));
    if (vis_global) JV_TRY(ctx->d_gs_visited.reserve(((size_t)4 << pl.vcap_log2) * (size_t)workers));

    // ---- per-query staging: [ids Q x K][scores Q x K][stats Q x 2][status Q][qmap Q][qnorm Q][counter] ----
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_ids = carve(sizeof(int32_t) * (size_t)Q * K), o_sc = carve(sizeof(float) * (size_t)Q * K);
    const size_t o_stats = carve(sizeof(long long) * 2 * (size_t)Q), o_status = carve(sizeof(int32_t) * (size_t)Q);
    const size_t o_qmap = carve(sizeof(int32_t) * (size_t)Q), o_qn = carve(sizeof(float) * (size_t)Q), o_counter = carve(sizeof(uint32_t));
    JV_TRY(ctx->d_gs_out.reserve(off));
    char *base = (char *)ctx->d_gs_out.ptr;
    int32_t *d_kept = (int32_t *)(base + o_ids);
    float *d_kept_sc = (float *)(base + o_sc);
    long long *d_stats = (long long *)(base + o_stats);
    int32_t *d_status = (int32_t *)(base + o_status);
    int32_t *d_qmap = (int32_t *)(base + o_qmap);
    float *d_qnorm = (float *)(base + o_qn);
    uint32_t *d_counter = (uint32_t *)(base + o_counter);
    if (f.before_walk) JV_TRY(f.before_walk(d_qnorm));

    p.Q = Q;
    p.rerankK = K;
    p.accept = (const unsigned long long *)d_acc;
    p.accept_stride = c.accept_stride_words;
    p.exclude = c.d_exclude;
    p.vcap_log2 = pl.vcap_log2;
    p.visited = vis_global ? (int32_t *)ctx->d_gs_visited.ptr : nullptr;
    p.cand_cap = pl.cand_cap;
    p.spill = (long long *)ctx->d_gs_spill.ptr;
    p.spill_cap = pl.spill_cap;
    p.out_ids = d_kept;
    p.out_scores = d_kept_sc;
    p.out_stats = d_stats;
    p.out_status = d_status;
    p.next_query = d_counter;

    auto launch = [&](const GwParams &pp, int w, bool safe) -> int {
        ProfScope ps(ctx, R_GSEARCH);
        return f.launch(pp, w, safe);
    };
    JV_HIP_CHECK(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), ctx->stream));
    JV_TRY(launch(p, workers, false));

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
        const int workers2 = gw_workers(ctx, f.lds_bytes(K, pl.cand_cap, 0), R, per2);
        JV_TRY(ctx->d_gs_visited.reserve(sizeof(uint32_t) * (size_t)bitmap_words * (size_t)workers2));
        JV_TRY(ctx->d_gs_spill.reserve(sizeof(long long) * (size_t)spill2 * (size_t)workers2));
        memcpy(ctx->h_out.ptr, redo.data(), sizeof(int32_t) * (size_t)R);
        JV_HIP_CHECK(hipMemcpyAsync(d_qmap, ctx->h_out.ptr, sizeof(int32_t) * (size_t)R, hipMemcpyHostToDevice, ctx->stream));
        JV_HIP_CHECK(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), ctx->stream));
        GwParams p2 = p;
        p2.qmap = d_qmap;
        p2.Q = R;
        p2.vcap_log2 = 0;
        p2.visited = nullptr;
        p2.bitmap = (uint32_t *)ctx->d_gs_visited.ptr;
        p2.bitmap_words = bitmap_words;
        p2.spill = (long long *)ctx->d_gs_spill.ptr;
        p2.spill_cap = spill2;
        JV_TRY(launch(p2, workers2, true));
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

    // ---- the first topK of the kept results (reranked by after_walk, if the front end has one) in NodeQueue order ----
    OutStage oi, osc;
    JV_TRY(stage_out_begin(ctx, c.out_ids, sizeof(int32_t) * (size_t)Q * topK, ctx->d_out, &oi));
    JV_TRY(stage_out_begin(ctx, c.out_scores, sizeof(float) * (size_t)Q * topK, ctx->d_scratch3, &osc));
    JV_TRY(ctx->d_scratch.reserve(topk_scratch_bytes(Q, std::max(K, topK))));
    if (f.after_walk) JV_TRY(f.after_walk(d_kept, d_kept_sc, d_qnorm));
    {
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_kept_sc, d_kept, Q, K, K, 0, topK, (int32_t *)oi.dev, (float *)osc.dev, ctx->d_scratch.ptr));
    }
    if (c.d_blank) JV_TRY(launch_bq_blank_rows(ctx->stream, c.d_blank, c.blank_rows, Q, topK, (int32_t *)oi.dev, (float *)osc.dev, d_stats));
    JV_TRY(stage_out_end(ctx, oi));
    JV_TRY(stage_out_end(ctx, osc));
    if (c.stats) {   // (after stage_out_end: it stages through h_out too)
        JV_TRY(ctx->h_out.reserve(sizeof(long long) * 2 * (size_t)Q));
        JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, d_stats, sizeof(long long) * 2 * (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const long long *h = (const long long *)ctx->h_out.ptr;
        for (int64_t i = 0; i < 2 * (int64_t)Q; ++i) c.stats[i] = h[i];
    } else {
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    const std::string pre(f.prefix);
    ctx_stat_add(ctx, (pre + "_calls").c_str(), 1);
    ctx_stat_add(ctx, (pre + "_queries").c_str(), Q);
    ctx_stat_add(ctx, (pre + "_queries_retried").c_str(), (long long)redo.size());
    ctx_stat_set(ctx, (pre + "_last_vcap_log2").c_str(), pl.vcap_log2);
    ctx_stat_set(ctx, (pre + "_last_workers").c_str(), workers);
    return JV_OK;
}

}  // namespace jv
