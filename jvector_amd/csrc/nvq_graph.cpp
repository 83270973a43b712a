// nvq_graph.cpp — the NVQ front end of the one-wave graph walk's host side (graph_walk.cpp) behind include/jvector_nvq_graph.h: the
// checks of the NVQ rows, their derived tables, the query side of NVQScorer (nvq_query_prep_kernel) and the launch of
// k_nvq_gsearch.hip.  The walk itself, scores included, is the kernel's.
#include "jv_device.h"
#include "jv_internal.h"
#include "ng_params.h"
#include "../../include/jvector_nvq_graph.h"

namespace jv {

// the block is the exact walk's: the result list's share is what remains beside the float tile, the candidate tier and the samples
static GwFront ng_front()
{
    GwFront f;
    f.prefix = "nvq_gs";
    f.k_name = "beamK";
    f.lds_bytes = [](int K, int cand_cap, int vcap_log2) { return ng_lds_bytes(K, cand_cap, vcap_log2); };
    f.fixed_lds = [](int cand_cap) { return ng_lds_bytes(0, cand_cap, 0); };
    return f;
}

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_nvq_graph_max_beam_k(jv_ctx *ctx, const jv_graph *g, int *out)
{
    clear_error();
    JV_REQUIRE(ctx && g && out, "nvq_graph_max_beam_k: NULL argument");
    *out = gw_max_k(ctx, ng_front());
    return JV_OK;
}

int jv_hip_nvq_graph_search(jv_ctx *ctx, const jv_graph *g, const jv_nvq_vectors *nv, const float *queries, int Q, jv_vsf vsf, int topK, int beamK,
                            const uint64_t *accept_bits, int64_t accept_stride_words, int32_t *out_ids, float *out_scores, int64_t *stats)
{
    clear_error();
    const char *who = "nvq_graph_search";
    JV_REQUIRE(ctx && g && nv, "%s: NULL argument", who);
    JV_REQUIRE(nv->device == ctx->device, "%s: the NVQ rows live on device %d, the context on %d", who, nv->device, ctx->device);
    JV_REQUIRE(vsf == JV_EUCLIDEAN || vsf == JV_DOT_PRODUCT || vsf == JV_COSINE, "%s: unsupported similarity function %d", who, (int)vsf);
    if (beamK == 0) beamK = topK;
    GwCall c{who, Q, topK, beamK, accept_bits, accept_stride_words, out_ids, out_scores, stats, nullptr, nullptr, nv->count};
    GwFront f = ng_front();
    JV_TRY(gw_check_counts(c, f));
    NgParams p{};
    GraphDeviceView gv;
    JV_TRY(gw_begin(ctx, c, g, p, &gv));
    const int64_t N = gv.n_nodes;
    JV_REQUIRE(nv->count >= N, "%s: %lld NVQ rows for a graph of %lld nodes", who, (long long)nv->count, (long long)N);
    JV_REQUIRE(gv.entry_node >= 0 && gv.entry_node < N, "%s: entry node %d outside the graph's %lld nodes", who, gv.entry_node, (long long)N);
    if (Q == 0) return JV_OK;
    JV_REQUIRE(queries && out_ids && out_scores, "%s: NULL buffer", who);
    JV_TRY(gw_admit(ctx, c, f, gv.max_degree, N));
    CtxBusy busy(ctx);
    JV_REQUIRE(busy.ok, "%s: the context is in use by another thread", who);

    // ---- inputs: the queries; NVQScorer's query side (per-query scalars, EUCLIDEAN: the shifted queries) follows the masks (before_walk) ----
    const jv_nvq *nq = nv->nvq;
    const int D = nq->D;
    const int kvsf = to_kernel_vsf(vsf);
    const void *d_q = nullptr;
    JV_TRY(stage_in(ctx, queries, sizeof(float) * (size_t)Q * D, ctx->h_in, ctx->d_in, &d_q));
    const size_t work = kvsf == VSF_L2 ? (size_t)Q * D : 0;
    JV_TRY(ctx->d_nvq_q.reserve(sizeof(float) * (work + (size_t)Q)));
    float *d_qwork = (float *)ctx->d_nvq_q.ptr, *d_qaux = d_qwork + work;
    p.bytes = nv->d_bytes;
    p.derived = nv->d_derived;
    p.mean = nq->d_mean;
    p.queries = kvsf == VSF_L2 ? d_qwork : (const float *)d_q;
    p.qaux = d_qaux;
    p.ld = nv->ld;
    p.D = D;
    p.S = nq->S;
    // (before_walk fills p.cosnorm — the table is made on first use — after gw_run took its copy of the shared part; the launch below
    // reads p only then)
    f.before_walk = [&](float *) -> int {
        JV_TRY(ensure_nvq_tables(ctx, const_cast<jv_nvq_vectors *>(nv), kvsf == VSF_COS));
        p.cosnorm = nv->d_cosnorm;
        ProfScope ps(ctx, R_NORMS);
        return launch_nvq_query_prep(ctx->stream, (const float *)d_q, Q, D, kvsf, nq->d_mean, d_qwork, d_qaux);
    };
    f.launch = [&](const GwParams &gp, int workers, bool safe) {
        NgParams pp = p;
        static_cast<GwParams &>(pp) = gp;
        const int rc = launch_nvq_graph_search(ctx->stream, pp, sizeof(NgParams), kvsf, workers, safe);
        if (rc != JV_OK) set_error("%s: the traversal kernel refused its launch parameters (%d)", who, rc);
        return rc;
    };
    return gw_run(ctx, c, f, p);
}

}  // extern "C"
