// exact_build.cpp — host side of the build-time scoring over float rows (include/jvector_exact_build.h): argument checks, staging,
// the LDS limit and the launch of the batched robust prune (k_exact_retain.hip), and the construction-time search from stored rows,
// which is jv_hip_exact_graph_search's own body with the rows gathered on the device (exact_graph.cpp).  bq_build.cpp is the template.
#include <algorithm>

#include "jv_device.h"
#include "jv_internal.h"
#include "xb_params.h"
#include "../../include/jvector_exact_build.h"

namespace jv {

// gfx950 lets one workgroup take the CU's whole 160 KB; the kernel opts in above 48 KB
static size_t xb_lds_limit(const jv_ctx *ctx) { return std::min<size_t>((size_t)160 << 10, ctx->lds_per_block); }

}  // namespace jv

using namespace jv;

extern "C" {

int jv_hip_exact_retain_diverse_max_candidates(jv_ctx *ctx, const jv_vectors *vectors, int maxDegree, int *out)
{
    clear_error();
    JV_REQUIRE(ctx && vectors && out, "exact_retain_diverse_max_candidates: NULL argument");
    JV_REQUIRE(maxDegree >= 1, "exact_retain_diverse_max_candidates: maxDegree must be positive");
    *out = (maxDegree > 64 || vectors->nvq) ? 0 : xb_max_candidates(xb_lds_limit(ctx), maxDegree);
    return JV_OK;
}

int jv_hip_exact_retain_diverse(jv_ctx *ctx, const jv_vectors *vectors, jv_vsf vsf, int P, int C, const int32_t *cand_nodes,
                                const float *cand_scores, const int32_t *cand_count, const int32_t *diverse_before, int maxDegree, float alpha,
                                int32_t *selected_out, int32_t *n_selected_out, float *short_edges_out)
{
    clear_error();
    const char *who = "exact_retain_diverse";
    JV_REQUIRE(ctx && vectors, "%s: NULL argument", who);
    JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", who, vectors->device, ctx->device);
    JV_REQUIRE(vsf == JV_EUCLIDEAN || vsf == JV_DOT_PRODUCT || vsf == JV_COSINE, "%s: unknown similarity %d", who, (int)vsf);
    JV_REQUIRE(P >= 0, "%s: negative node count", who);
    JV_REQUIRE(C >= 1, "%s: C must be positive", who);
    JV_REQUIRE(maxDegree >= 1, "%s: maxDegree must be positive", who);
    // an alpha below 1, or NaN, means no round; above 64 (infinity included) the kernel's loop over the alpha steps has no useful end
    JV_REQUIRE(!(alpha > XB_MAX_ALPHA), "%s: alpha %g above %g", who, (double)alpha, (double)XB_MAX_ALPHA);
    if (P == 0) return JV_OK;
    JV_REQUIRE(cand_nodes && cand_scores && selected_out && n_selected_out, "%s: NULL buffer", who);
    if (maxDegree > 64) {
        set_error("%s: maxDegree %d above 64", who, maxDegree);
        return JV_ERR_UNSUPPORTED;
    }
    JV_FLOAT_ROWS(vectors, who);
    const int max_c = xb_max_candidates(xb_lds_limit(ctx), maxDegree);
    if (C > max_c) {
        set_error("%s: %d candidates at maxDegree %d above the %d the prune kernel's LDS block holds; prune in smaller candidate lists", who, C,
                  maxDegree, max_c);
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(use_device(ctx->device));
    CtxBusy busy(ctx);
    JV_REQUIRE(busy.ok, "%s: the context is in use by another thread", who);
    const int kvsf = to_kernel_vsf(vsf);
    if (kvsf == VSF_COS) JV_TRY(ensure_vector_norms(ctx, const_cast<jv_vectors *>(vectors)));
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
    XbParams p{};
    p.rows = vectors->d_vecs;
    p.vnorm = kvsf == VSF_COS ? vectors->d_sqnorm : nullptr;
    p.n = vectors->count;
    p.D = vectors->D;
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
        // LDS sets the nodes of a CU (160 KB on gfx950), at most 16 one-wave workgroups
        const size_t lds = xb_lds_bytes(C, maxDegree);
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / (lds + 256)));
        const int rc = launch_exact_retain(ctx->stream, p, sizeof(XbParams), kvsf, xb_lds_limit(ctx), std::min(P, ctx->num_cus * per_cu));
        if (rc != JV_OK) {
            set_error("%s: the prune kernel refused its launch parameters (%d)", who, rc);
            return rc;
        }
    }
    JV_HIP_CHECK(hipMemcpyAsync(selected_out, p.selected_out, sel_bytes, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipMemcpyAsync(n_selected_out, p.n_selected_out, cnt_bytes, hipMemcpyDefault, ctx->stream));
    if (short_edges_out) JV_HIP_CHECK(hipMemcpyAsync(short_edges_out, p.short_edges_out, sizeof(float) * (size_t)P, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx_stat_add(ctx, "exact_retain_calls", 1);
    ctx_stat_add(ctx, "exact_retain_nodes", P);
    return JV_OK;
}

int jv_hip_exact_graph_search_nodes(jv_ctx *ctx, const jv_graph *g, const jv_vectors *vectors, const int32_t *nodes, int Q, jv_vsf vsf, int topK,
                                    int beamK, int exclude_self, int32_t *out_ids, float *out_scores, int64_t *stats)
{
    clear_error();
    JV_REQUIRE(nodes || Q <= 0, "exact_graph_search_nodes: NULL buffer");
    return exact_graph_search_run(ctx, "exact_graph_search_nodes", g, vectors, nullptr, nodes, exclude_self, Q, vsf, topK, beamK, nullptr, 0, out_ids,
                                  out_scores, stats);
}

}  // extern "C"
