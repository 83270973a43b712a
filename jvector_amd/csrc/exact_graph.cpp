// exact_graph.cpp — host side of the exact-score graph search (include/jvector_exact_graph.h): argument checks, the workspace, the
// launch of k_exact_gsearch.hip, the pass that runs again the queries that outgrew the first attempt's fixed-size structures, and the
// final ordering through launch_topk.  The walk itself, scores included, is the kernel's; bq_graph.cpp is the template.
#include <algorithm>
#include <vector>

#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"   // launch_bq_blank_rows: nothing in it looks at a BQ row
#include "xg_params.h"
#include "../../include/jvector_exact_graph.h"

namespace jv {

constexpr int kXgMaxCandCap = 4096;
constexpr size_t kXgLdsLimit = 65536;
constexpr size_t kXgScratchBudget = (size_t)1 << 30;   // per-worker visited tables / bitmaps + spill slices of one launch

struct XgPlan {
    int vcap_log2 = 0, cand_cap = 0, spill_cap = 0;
};

static int xg_ceil_log2(long long v)
{
    int b = 0;
    while ((1ll << b) < v) ++b;
    return b;
}

// candidates' LDS tier: exact_gs_cand_cap, else twice beamK rounded up to a power of two within [512, 2048]
static int xg_cand_cap(const jv_ctx *ctx, int beamK)
{
    long long c = ctx_opt(ctx, "exact_gs_cand_cap", 0);
    if (c <= 0) c = std::min(2048ll, std::max(512ll, 1ll << xg_ceil_log2(2ll * beamK)));
    return (int)std::min<long long>(kXgMaxCandCap, std::max<long long>(BG_MIN_CAND_CAP, c));
}

static size_t xg_lds_limit(const jv_ctx *ctx) { return std::min(kXgLdsLimit, ctx->lds_per_block); }

// largest beamK whose result list fits next to the score tile, the widest candidate tier and the samples — the visited table moves to
// global memory when LDS has no room for it, and the query is read through scalar loads: neither takes a share, whatever D is
static int xg_max_beam_k(const jv_ctx *ctx, int cand_cap)
{
    const size_t fixed = xg_lds_bytes(0, cand_cap, 0);
    return (int)((xg_lds_limit(ctx) - fixed) / sizeof(long long));
}

// the first attempt: a table for 48 visited nodes per kept result + 2048 at half load (exact_gs_vcap_log2 overrides), never more than the
// graph can fill; in LDS when it is small and fits beside the tile and the queues, else in global memory
static XgPlan xg_plan(const jv_ctx *ctx, int beamK, long long n_nodes)
{
    XgPlan pl;
    pl.cand_cap = xg_cand_cap(ctx, beamK);
    long long v = ctx_opt(ctx, "exact_gs_vcap_log2", 0);
    if (v <= 0) v = std::min(xg_ceil_log2(2 * (48ll * beamK + 2048)), xg_ceil_log2(2 * (n_nodes + 64)));
    pl.vcap_log2 = (int)std::min<long long>(BG_MAX_VCAP_LOG2, std::max<long long>(BG_MIN_VCAP_LOG2, v));
    if (pl.vcap_log2 <= BG_VIS_LDS_MAX_LOG2 && xg_lds_bytes(beamK, pl.cand_cap, pl.vcap_log2) > xg_lds_limit(ctx))
        pl.vcap_log2 = BG_VIS_LDS_MAX_LOG2 + 1;
    // live candidates + evicted results never exceed the visited nodes: a slice the table cannot outgrow, capped at 16 LDS tiers
    pl.spill_cap = (int)std::min<long long>((1ll << pl.vcap_log2) / 2 + 64, 16ll * pl.cand_cap);
    return pl;
}

static int xg_workers(const jv_ctx *ctx, size_t lds, long long items, size_t per_worker)
{
    // LDS sets the waves of a CU (160 KB on gfx950), at most 16 workgroups; every worker owns a scratch slice
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / std::max<size_t>(lds, 1)));
    return (int)std::max<long long>(1, std::min<long long>({items, (long long)ctx->num_cus * per_cu, (long long)(kXgScratchBudget / per_worker)}));
}

// jv_hip_exact_graph_search (queries) and jv_hip_exact_graph_search_nodes (seed_nodes: query q is row seed_nodes[q] of `vectors`,
// gathered on the device; exclude_self: item q never keeps node seed_nodes[q]) — one body, declared in jv_internal.h
int exact_graph_search_run(jv_ctx *ctx, const char *who, const jv_graph *g, const jv_vectors *vectors, const float *queries,
                           const int32_t *seed_nodes, int exclude_self, int Q, jv_vsf vsf, int topK, int beamK, const uint64_t *accept_bits,
                           int64_t accept_stride_words, int32_t *out_ids, float *out_scores, int64_t *stats)
{
    JV_REQUIRE(ctx && g && vectors, "%s: NULL argument", who);
    JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", who, vectors->device, ctx->device);
    JV_REQUIRE(Q >= 0, "%s: negative query count", who);
    JV_REQUIRE(topK >= 1, "%s: topK must be positive", who);
    if (beamK == 0) beamK = topK;
    JV_REQUIRE(beamK >= topK, "beamK %d must be >= topK %d", beamK, topK);
    JV_FLOAT_ROWS(vectors, who);
    JV_TRY(use_device(ctx->device));
    XgParams p{};
    GraphDeviceView gv;
    {
        const int rc = graph_device_view(ctx, g, p.lv, &gv);
        if (rc != JV_OK) return rc;
    }
    const int64_t N = gv.n_nodes;
    JV_REQUIRE(vectors->count >= N, "%s: %lld vectors for a graph of %lld nodes", who, (long long)vectors->count, (long long)N);
    JV_REQUIRE(gv.entry_node >= 0 && gv.entry_node < N, "%s: entry node %d outside the graph's %lld nodes", who, gv.entry_node, (long long)N);
    const int64_t mask_words = (N + 63) / 64;
    JV_REQUIRE(accept_stride_words >= 0 && (!accept_bits || accept_stride_words == 0 || accept_stride_words >= mask_words),
               "%s: accept_stride_words %lld is smaller than the %lld words one mask needs", who, (long long)accept_stride_words,
               (long long)mask_words);
    if (Q == 0) return JV_OK;
    JV_REQUIRE((queries || seed_nodes) && out_ids && out_scores, "%s: NULL buffer", who);
    const bool seeds_on_device = seed_nodes && is_device_ptr(seed_nodes);
    if (seed_nodes && !seeds_on_device)
        for (int q = 0; q < Q; ++q)
            JV_REQUIRE(seed_nodes[q] >= 0 && seed_nodes[q] < vectors->count, "%s: ordinal %d of item %d outside the %lld rows", who, seed_nodes[q], q,
                       (long long)vectors->count);
    const int D = vectors->D;
    if (gv.max_degree > kMaxGraphDegree) {
        set_error("%s: degree %d above %d", who, gv.max_degree, kMaxGraphDegree);
        return JV_ERR_UNSUPPORTED;
    }
    const XgPlan pl = xg_plan(ctx, beamK, N);
    const int max_beam = xg_max_beam_k(ctx, xg_cand_cap(ctx, 1 << 20));
    if (beamK > max_beam || xg_lds_bytes(beamK, pl.cand_cap, pl.vcap_log2) > xg_lds_limit(ctx)) {
        set_error("%s: beamK %d above the %d the traversal kernel's LDS block holds", who, beamK, max_beam);
        return JV_ERR_UNSUPPORTED;
    }
    CtxBusy busy(ctx);
    JV_REQUIRE(busy.ok, "%s: the context is in use by another thread", who);

    // ---- inputs: the queries (given, or gathered from the rows), the cosine norms of both sides, the masks ----
    const int kvsf = to_kernel_vsf(vsf);
    const bool tr = exact_tr_supported(vectors->d_vecs, D);
    const void *d_q = nullptr, *d_seeds = nullptr;
    if (seed_nodes) {
        JV_TRY(stage_in(ctx, seed_nodes, sizeof(int32_t) * (size_t)Q, ctx->h_in, ctx->d_gs_mask, &d_seeds));
        JV_TRY(ctx->d_in.reserve(sizeof(float) * (size_t)Q * D));
        ProfScope ps(ctx, R_EXACT);
        JV_TRY(launch_gather_rows(ctx->stream, vectors->d_vecs, vectors->count, D, (const int32_t *)d_seeds, Q, (float *)ctx->d_in.ptr, nullptr, 0));
        d_q = ctx->d_in.ptr;
    } else {
        JV_TRY(stage_in(ctx, queries, sizeof(float) * (size_t)Q * D, ctx->h_in, ctx->d_in, &d_q));
    }
    const void *d_acc = nullptr;
    if (accept_bits)
        JV_TRY(stage_in(ctx, accept_bits, sizeof(uint64_t) * (size_t)(accept_stride_words * (Q - 1) + mask_words), ctx->h_in, ctx->d_scratch2,
                        &d_acc));
    if (kvsf == VSF_COS && tr) JV_TRY(ensure_vector_norms(ctx, const_cast<jv_vectors *>(vectors)));

    // ---- the first attempt's workers and their scratch ----
    const size_t lds = xg_lds_bytes(beamK, pl.cand_cap, pl.vcap_log2);
    const bool vis_global = pl.vcap_log2 > BG_VIS_LDS_MAX_LOG2;
    const size_t per_worker = sizeof(long long) * (size_t)pl.spill_cap + (vis_global ? ((size_t)4 << pl.vcap_log2) : 0);
    const int workers = xg_workers(ctx, lds, Q, per_worker);
    JV_TRY(ctx->d_gs_spill.reserve(sizeof(long long) * (size_t)pl.spill_cap * (size_t)workers));
    if (vis_global) JV_TRY(ctx->d_gs_visited.reserve(((size_t)4 << pl.vcap_log2) * (size_t)workers));

    // ---- per-query staging: [ids Q x beamK][scores Q x beamK][stats Q x 2][status Q][qmap Q][qnorm Q][counter] ----
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_ids = carve(sizeof(int32_t) * (size_t)Q * beamK), o_sc = carve(sizeof(float) * (size_t)Q * beamK);
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
    if (kvsf == VSF_COS) {
        ProfScope ps(ctx, R_NORMS);
        JV_TRY(launch_query_sqnorms(ctx->stream, (const float *)d_q, D, Q, d_qnorm));
    }

    p.entry_node = gv.entry_node;
    p.entry_level = gv.entry_level;
    p.n_nodes = (int32_t)N;
    p.rows = vectors->d_vecs;
    p.vnorm = (kvsf == VSF_COS && tr) ? vectors->d_sqnorm : nullptr;
    p.queries = (const float *)d_q;
    p.qnorm = kvsf == VSF_COS ? d_qnorm : nullptr;
    p.D = D;
    p.Q = Q;
    p.beamK = beamK;
    p.accept = (const unsigned long long *)d_acc;
    p.accept_stride = accept_stride_words;
    p.exclude = exclude_self ? (const int32_t *)d_seeds : nullptr;
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

    auto launch = [&](const XgParams &pp, int w, bool safe) -> int {
        ProfScope ps(ctx, R_GSEARCH);
        const int rc = launch_exact_graph_search(ctx->stream, pp, sizeof(XgParams), kvsf, tr, w, safe);
        if (rc != JV_OK) set_error("%s: the traversal kernel refused its launch parameters (%d)", who, rc);
        return rc;
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
        const int workers2 = xg_workers(ctx, xg_lds_bytes(beamK, pl.cand_cap, 0), R, per2);
        JV_TRY(ctx->d_gs_visited.reserve(sizeof(uint32_t) * (size_t)bitmap_words * (size_t)workers2));
        JV_TRY(ctx->d_gs_spill.reserve(sizeof(long long) * (size_t)spill2 * (size_t)workers2));
        memcpy(ctx->h_out.ptr, redo.data(), sizeof(int32_t) * (size_t)R);
        JV_HIP_CHECK(hipMemcpyAsync(d_qmap, ctx->h_out.ptr, sizeof(int32_t) * (size_t)R, hipMemcpyHostToDevice, ctx->stream));
        JV_HIP_CHECK(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), ctx->stream));
        XgParams p2 = p;
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
                set_error("%s: query %d did not finish in the roomy form (status %d)", who, q, hs[q]);
                return JV_ERR_HIP;
            }
    }

    // ---- the first topK of the kept results in NodeQueue order ----
    OutStage oi, osc;
    JV_TRY(stage_out_begin(ctx, out_ids, sizeof(int32_t) * (size_t)Q * topK, ctx->d_out, &oi));
    JV_TRY(stage_out_begin(ctx, out_scores, sizeof(float) * (size_t)Q * topK, ctx->d_scratch3, &osc));
    JV_TRY(ctx->d_scratch.reserve(topk_scratch_bytes(Q, std::max(beamK, topK))));
    {
        ProfScope ps(ctx, R_TOPK);
        JV_TRY(launch_topk(ctx->stream, ctx, d_kept_sc, d_kept, Q, beamK, beamK, 0, topK, (int32_t *)oi.dev, (float *)osc.dev, ctx->d_scratch.ptr));
    }
    if (seeds_on_device)   // ordinals nobody looked at: an item whose ordinal names no row comes back empty, with zero counters
        JV_TRY(launch_bq_blank_rows(ctx->stream, (const int32_t *)d_seeds, vectors->count, Q, topK, (int32_t *)oi.dev, (float *)osc.dev, d_stats));
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
    ctx_stat_add(ctx, "exact_gs_calls", 1);
    ctx_stat_add(ctx, "exact_gs_queries", Q);
    ctx_stat_add(ctx, "exact_gs_queries_retried", (long long)redo.size());
    ctx_stat_set(ctx, "exact_gs_last_vcap_log2", pl.vcap_log2);
    ctx_stat_set(ctx, "exact_gs_last_workers", workers);
    return JV_OK;
}

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_exact_graph_max_beam_k(jv_ctx *ctx, const jv_graph *g, int D, int *out)
{
    clear_error();
    JV_REQUIRE(ctx && g && out, "exact_graph_max_beam_k: NULL argument");
    JV_REQUIRE(D >= 1, "exact_graph_max_beam_k: dimension %d", D);
    *out = xg_max_beam_k(ctx, xg_cand_cap(ctx, 1 << 20));
    return JV_OK;
}

int jv_hip_exact_graph_search(jv_ctx *ctx, const jv_graph *g, const jv_vectors *vectors, const float *queries, int Q, jv_vsf vsf, int topK,
                              int beamK, const uint64_t *accept_bits, int64_t accept_stride_words, int32_t *out_ids, float *out_scores,
                              int64_t *stats)
{
    clear_error();
    return exact_graph_search_run(ctx, "exact_graph_search", g, vectors, queries, nullptr, 0, Q, vsf, topK, beamK, accept_bits, accept_stride_words,
                                  out_ids, out_scores, stats);
}

}  // extern "C"
