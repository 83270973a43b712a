// exact_graph.cpp — the exact-score front end of the one-wave graph walk's host side (graph_walk.cpp) behind
// include/jvector_exact_graph.h: the checks of the float rows, the queries (given, or gathered from the rows), the cosine norms of both
// sides and the launch of k_exact_gsearch.hip.  The walk itself, scores included, is the kernel's.
#include "jv_device.h"
#include "jv_internal.h"
#include "xg_params.h"
#include "../../include/jvector_exact_graph.h"

namespace jv {

// the result list's share of the block is what remains beside the score tile, the candidate tier and the samples — the query is read
// through scalar loads and takes none, whatever D is
static GwFront xg_front()
{
    GwFront f;
    f.prefix = "exact_gs";
    f.k_name = "beamK";
    f.lds_bytes = [](int K, int cand_cap, int vcap_log2) { return xg_lds_bytes(K, cand_cap, vcap_log2); };
    f.fixed_lds = [](int cand_cap) { return xg_lds_bytes(0, cand_cap, 0); };
    return f;
}

// jv_hip_exact_graph_search (queries) and jv_hip_exact_graph_search_nodes (seed_nodes: query q is row seed_nodes[q] of `vectors`,
// gathered on the device; exclude_self: item q never keeps node seed_nodes[q]) — one body, declared in jv_internal.h
int exact_graph_search_run(jv_ctx *ctx, const char *who, const jv_graph *g, const jv_vectors *vectors, const float *queries,
                           const int32_t *seed_nodes, int exclude_self, int Q, jv_vsf vsf, int topK, int beamK, const uint64_t *accept_bits,
                           int64_t accept_stride_words, int32_t *out_ids, float *out_scores, int64_t *stats)
{
    JV_REQUIRE(ctx && g && vectors, "%s: NULL argument", who);
    JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", who, vectors->device, ctx->device);
    if (beamK == 0) beamK = topK;
    GwCall c{who, Q, topK, beamK, accept_bits, accept_stride_words, out_ids, out_scores, stats, nullptr, nullptr, vectors->count};
    GwFront f = xg_front();
    JV_TRY(gw_check_counts(c, f));
    JV_FLOAT_ROWS(vectors, who);
    XgParams p{};
    GraphDeviceView gv;
    JV_TRY(gw_begin(ctx, c, g, p, &gv));
    const int64_t N = gv.n_nodes;
    JV_REQUIRE(vectors->count >= N, "%s: %lld vectors for a graph of %lld nodes", who, (long long)vectors->count, (long long)N);
    JV_REQUIRE(gv.entry_node >= 0 && gv.entry_node < N, "%s: entry node %d outside the graph's %lld nodes", who, gv.entry_node, (long long)N);
    if (Q == 0) return JV_OK;
    JV_REQUIRE((queries || seed_nodes) && out_ids && out_scores, "%s: NULL buffer", who);
    const bool seeds_on_device = seed_nodes && is_device_ptr(seed_nodes);
    if (seed_nodes && !seeds_on_device)
        for (int q = 0; q < Q; ++q)
            JV_REQUIRE(seed_nodes[q] >= 0 && seed_nodes[q] < vectors->count, "%s: ordinal %d of item %d outside the %lld rows", who, seed_nodes[q], q,
                       (long long)vectors->count);
    JV_TRY(gw_admit(ctx, c, f, gv.max_degree, N));
    CtxBusy busy(ctx);
    JV_REQUIRE(busy.ok, "%s: the context is in use by another thread", who);

    // ---- inputs: the queries (given, or gathered from the rows); the cosine norms of both sides follow the masks (before_walk) ----
    const int D = vectors->D;
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
    c.d_exclude = exclude_self ? (const int32_t *)d_seeds : nullptr;
    c.d_blank = seeds_on_device ? (const int32_t *)d_seeds : nullptr;   // ordinals nobody looked at: one that names no row comes back empty
    p.rows = vectors->d_vecs;
    p.queries = (const float *)d_q;
    p.D = D;
    // (before_walk fills p.vnorm / p.qnorm after gw_run took its copy of the shared part; the launch below reads p only then)
    f.before_walk = [&](float *d_qnorm) -> int {
        if (kvsf != VSF_COS) return JV_OK;
        if (tr) JV_TRY(ensure_vector_norms(ctx, const_cast<jv_vectors *>(vectors)));
        ProfScope ps(ctx, R_NORMS);
        JV_TRY(launch_query_sqnorms(ctx->stream, (const float *)d_q, D, Q, d_qnorm));
        p.vnorm = tr ? vectors->d_sqnorm : nullptr;
        p.qnorm = d_qnorm;
        return JV_OK;
    };
    f.launch = [&](const GwParams &gp, int workers, bool safe) {
        XgParams pp = p;
        static_cast<GwParams &>(pp) = gp;
        const int rc = launch_exact_graph_search(ctx->stream, pp, sizeof(XgParams), kvsf, tr, workers, safe);
        if (rc != JV_OK) set_error("%s: the traversal kernel refused its launch parameters (%d)", who, rc);
        return rc;
    };
    return gw_run(ctx, c, f, p);
}

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_exact_graph_max_beam_k(jv_ctx *ctx, const jv_graph *g, int D, int *out)
{
    clear_error();
    JV_REQUIRE(ctx && g && out, "exact_graph_max_beam_k: NULL argument");
    JV_REQUIRE(D >= 1, "exact_graph_max_beam_k: dimension %d", D);
    *out = gw_max_k(ctx, xg_front());
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
