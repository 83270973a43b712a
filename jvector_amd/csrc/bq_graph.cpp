// bq_graph.cpp — the BQ front end of the one-wave graph walk's host side (graph_walk.cpp) behind include/jvector_bq_graph.h: the
// checks of the BQ rows, the encode of the queries, the launch of k_bq_gsearch.hip and the exact rerank through the launchers of
// jv_hip_graph_search / jv_hip_bq_search_flat (rerank_gather -> launch_exact_gather): reranked results carry the same bits.
#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"
#include "../../include/jvector_bq_graph.h"

namespace jv {

// W: words of a row (the generic kernel keeps the query's words in LDS); the result list's share of the block is what remains beside
// the candidate tier, the samples and the widest query
static GwFront bg_front(int W)
{
    GwFront f;
    f.prefix = "bq_gs";
    f.k_name = "rerankK";
    f.lds_bytes = [W](int K, int cand_cap, int vcap_log2) { return bq_graph_lds_bytes(K, cand_cap, W, vcap_log2); };
    f.fixed_lds = [](int cand_cap) { return bg_lds_bytes(0, cand_cap, (kBqMaxDim + 63) / 64, 0); };
    return f;
}

// Everything jv_hip_bq_graph_search checks before it touches the stream, and the graph's device view (c.p.lv, entry, n_nodes).
// `input` is the caller's query buffer (floats or ordinals): only its presence is looked at.
int bq_graph_begin(jv_ctx *ctx, BqGraphCall &c, const void *input)
{
    c.empty = false;
    const jv_bq_vectors *bq = c.bq;
    const jv_vectors *vectors = c.vectors;
    JV_REQUIRE(ctx && c.g && bq, "%s: NULL argument", c.who);
    JV_REQUIRE(bq->device == ctx->device, "%s: the BQ vectors live on device %d, the context on %d", c.who, bq->device, ctx->device);
    const GwCall w{c.who, c.Q, c.topK, c.rerankK, c.accept_bits, c.accept_stride_words, c.out_ids, c.out_scores, c.stats, nullptr, nullptr, 0};
    const GwFront f = bg_front(bq->W);
    JV_TRY(gw_check_counts(w, f));
    if (vectors) {
        JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", c.who, vectors->device, ctx->device);
        JV_REQUIRE(vectors->D == bq->D, "%s: vectors of dimension %d, BQ of dimension %d", c.who, vectors->D, bq->D);
    }
    c.p = BgParams{};
    GraphDeviceView gv;
    JV_TRY(gw_begin(ctx, w, c.g, c.p, &gv));
    const int64_t N = gv.n_nodes;
    JV_REQUIRE(bq->count >= N, "%s: %lld BQ rows for a graph of %lld nodes", c.who, (long long)bq->count, (long long)N);
    JV_REQUIRE(!vectors || vectors->count >= N, "%s: %lld vectors for a graph of %lld nodes", c.who, vectors ? (long long)vectors->count : 0ll,
               (long long)N);
    if (c.Q == 0) {
        c.empty = true;
        return JV_OK;
    }
    JV_REQUIRE(input && c.out_ids && c.out_scores, "%s: NULL buffer", c.who);
    if (bq->D > kBqMaxDim) {
        set_error("%s: dimension %d above %d", c.who, bq->D, kBqMaxDim);
        return JV_ERR_UNSUPPORTED;
    }
    return gw_admit(ctx, w, f, gv.max_degree, N);
}

// The search from the encoded queries on: d_qw holds Q x W query words, written by work already queued on the context's stream
// (the caller holds the context).  d_q: the float queries on the device, read by the rerank only (c.vectors != NULL).  d_exclude,
// d_blank_nodes (nullable): GwCall's d_exclude and d_blank over the BQ rows.
int bq_graph_finish(jv_ctx *ctx, const BqGraphCall &c, const float *d_q, const uint64_t *d_qw, const int32_t *d_exclude,
                    const int32_t *d_blank_nodes)
{
    const jv_bq_vectors *bq = c.bq;
    const GwCall w{c.who, c.Q, c.topK, c.rerankK, c.accept_bits, c.accept_stride_words, c.out_ids, c.out_scores, c.stats, d_exclude, d_blank_nodes, bq->count};
    BgParams p = c.p;
    p.rows = bq->d_rows;
    p.qwords = d_qw;
    p.D = bq->D;
    p.W = bq->W;
    GwFront f = bg_front(bq->W);
    f.launch = [&](const GwParams &gp, int workers, bool safe) {   // (the launcher sets the error text of a refused launch itself)
        BgParams pp = p;
        static_cast<GwParams &>(pp) = gp;
        return launch_bq_graph_search(ctx->stream, pp, workers, safe);
    };
    // reranking :471-507 on the device-resident candidates
    if (c.vectors)
        f.after_walk = [&](const int32_t *d_cand, float *d_cand_sc, float *d_qnorm) {
            return rerank_gather(ctx, c.vectors, d_q, c.Q, c.vsf, d_cand, c.rerankK, d_cand_sc, d_qnorm);
        };
    return gw_run(ctx, w, f, p);
}

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_bq_graph_max_rerank_k(jv_ctx *ctx, const jv_graph *g, int *out)
{
    clear_error();
    JV_REQUIRE(ctx && g && out, "bq_graph_max_rerank_k: NULL argument");
    *out = gw_max_k(ctx, bg_front(0));
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
