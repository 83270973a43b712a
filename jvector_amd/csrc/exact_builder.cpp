// exact_builder.cpp — batched Vamana construction from the float rows alone, behind the C ABI (include/jvector_exact_builder.h): the
// REFERENCE ORDER pipeline of bl_host.h (shared with builder.cpp and bq_builder.cpp) driven by the two exact scoring calls.  Here: the
// search, the prune handed to the shared steps, the capacity checks, the row gather and the entry point of the layered build.
//
// One insert_batch = B concurrent addGraphNode calls (GraphIndexBuilder.java:605-659) that do not see each other:
//   1. candidates = the search from each node's own row (topK = beam) over the graph so far   jv_hip_exact_graph_search_nodes
//   2. robust prune of every candidate list                                                   jv_hip_exact_retain_diverse
//   3. insertDiverse on the new nodes' empty lists, back edges emitted with their scores       launch_bl_ro_apply_selection
//   4. back edges sorted by (target, edge index)                                              launch_bl_sort_edges
//   5. per target: Neighbors.insert in batch order; lists past the hard maximum handed over    launch_bl_ro_backlink_merge
//   6. those lists: retainDiverse(list, diverseBefore) over the STORED scores, row rewritten   jv_hip_exact_retain_diverse,
//                                                                                             launch_bl_ro_rewrite_rows
// VectorSimilarityFunction.compare is symmetric bit for bit: the score the search gives a neighbour IS the score its back link is stored
// under and the score the prune tests against, so there is nothing to re-score and this builder has one list discipline, the
// reference's.  Steps 3 - 6 never look at what a score means: they are bl_host.h (bl_ro_insert) over k_builder.hip / bl_body.h as they
// stand.  With one node per batch the lists equal the one-thread restatement of GraphIndexBuilder byte for byte
// (tests/test_zz_exact_builder_gpu.py).  Everything runs on the context's stream; the host reads back the search statuses and one counter
// per batch.
#include <algorithm>
#include <vector>

#include "bl_body.h"
#include "bl_host.h"
#include "gs_params.h"
#include "jv_device.h"
#include "jv_internal.h"
#include "xm_params.h"
#include "../../include/jvector_exact_builder.h"

using namespace jv;

struct jv_exact_builder : BlBuilderState {
    const jv_vectors *vectors = nullptr;
    jv_vsf vsf = JV_EUCLIDEAN;
};

namespace {

bool known_vsf(jv_vsf vsf) { return vsf == JV_EUCLIDEAN || vsf == JV_DOT_PRODUCT || vsf == JV_COSINE; }

// what the scoring kernels cannot take is refused before anything is allocated: a list is never truncated to fit
int check_capacity(jv_ctx *ctx, const char *who, const jv_vectors *vectors, const jv_graph *g, int max_degree, int beam_width, int R)
{
    int max_k = 0, max_c = 0;
    JV_TRY(jv_hip_exact_graph_max_beam_k(ctx, g, vectors->D, &max_k));
    if (beam_width > max_k) {
        set_error("%s: beamWidth %d above the %d results the traversal kernel's LDS block holds", who, beam_width, max_k);
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(jv_hip_exact_retain_diverse_max_candidates(ctx, vectors, max_degree, &max_c));
    const int need = std::max(beam_width + R, 3 * R);   // improve: row + candidates; back links: row + 2 R appended entries
    if (need > max_c) {
        set_error("%s: lists of %d entries (beamWidth %d, working rows of %d) above the %d candidates the prune kernel's LDS block holds at maxDegree %d",
                  who, need, beam_width, R, max_c, max_degree);
        return JV_ERR_UNSUPPORTED;
    }
    return JV_OK;
}

// the robust prune the steps of bl_host.h run: over the float rows, under the builder's similarity, maxDegree and alpha
auto retain_of(jv_ctx *ctx, const jv_exact_builder *b)
{
    return [=](const int32_t *d_list, const float *d_sc, const int32_t *d_count, const int32_t *d_before, int P, int L, int32_t *d_sel, int32_t *d_nsel) {
        return jv_hip_exact_retain_diverse(ctx, b->vectors, b->vsf, P, L, d_list, d_sc, d_count, d_before, b->Rf, b->alpha, d_sel, d_nsel, nullptr);
    };
}

// 1: GraphSearcher.search(searchProviderFor(node), k, k) from each node's own row over the graph built so far -> d_cand / d_csc [B][k]
int search_candidates(jv_ctx *ctx, jv_exact_builder *b, const int32_t *d_nodes, int B, int k, bool exclude_self)
{
    const int search_chunk = 65536;
    JV_TRY(b->d_cand.reserve(sizeof(int32_t) * (size_t)B * k));
    JV_TRY(b->d_csc.reserve(sizeof(float) * (size_t)B * k));
    int32_t *d_cand = (int32_t *)b->d_cand.ptr;
    float *d_csc = (float *)b->d_csc.ptr;
    const double t0 = bl_now_s();
    for (int s = 0; s < B; s += search_chunk) {
        const int bc = std::min(search_chunk, B - s);
        b->h_stats.resize(2 * (size_t)bc);
        JV_TRY(jv_hip_exact_graph_search_nodes(ctx, b->graph, b->vectors, d_nodes + s, bc, b->vsf, k, k, exclude_self ? 1 : 0, d_cand + (size_t)s * k,
                                               d_csc + (size_t)s * k, b->h_stats.data()));
        for (int q = 0; q < bc; ++q) {
            b->visited += b->h_stats[2 * (size_t)q];
            b->expanded += b->h_stats[2 * (size_t)q + 1];
        }
    }
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->search_s += bl_now_s() - t0;
    return JV_OK;
}

// the launchers of k_exact_builder.hip return a status and no text (they are a library of their own)
int xm_launched(int rc, const char *what)
{
    if (rc != JV_OK)
        set_error("exact builder kernels (%s): %s", what,
                  rc == JV_ERR_INVALID ? "bad launch parameters, or libjvector_hip_xm.so was built from another xm_params.h" : "the launch failed");
    return rc;
}

// rows d_ids[0 .. count) of `vectors` into the fresh set *out
int gather_rows(jv_ctx *ctx, const jv_vectors *vectors, const int32_t *d_ids, int64_t count, jv_vectors **out)
{
    jv_vectors *sub = nullptr;
    JV_TRY(jv_hip_vectors_create(ctx, count, vectors->D, &sub));
    XmGatherParams p{};
    p.rows = vectors->d_vecs;
    p.n = vectors->count;
    p.D = vectors->D;
    p.ids = d_ids;
    p.count = count;
    p.out = sub->d_vecs;
    int rc = xm_launched(launch_xm_gather_rows(ctx->stream, p, sizeof(XmGatherParams)), "gather rows");
    if (rc == JV_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        set_error("exact builder: the row gather failed");
        rc = JV_ERR_HIP;
    }
    if (rc != JV_OK) {
        jv_hip_vectors_destroy(sub);
        return rc;
    }
    *out = sub;
    return JV_OK;
}

}  // namespace

extern "C" {

int jv_hip_exact_builder_create(jv_ctx *ctx, const jv_vectors *vectors, jv_vsf vsf, int max_degree, int beam_width, float alpha, float neighbor_overflow,
                                jv_exact_builder **out)
{
    clear_error();
    const char *who = "exact_builder_create";
    JV_REQUIRE(ctx && vectors && out, "%s: NULL argument", who);
    *out = nullptr;
    JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", who, vectors->device, ctx->device);
    JV_REQUIRE(known_vsf(vsf), "%s: unknown similarity %d", who, (int)vsf);
    JV_REQUIRE(vectors->count >= 1 && vectors->count <= 0x7fffffffLL, "%s: %lld nodes", who, (long long)vectors->count);
    JV_TRY(bl_check_parameters(who, max_degree, beam_width, alpha, neighbor_overflow));
    JV_FLOAT_ROWS(vectors, who);
    JV_TRY(use_device(ctx->device));
    jv_exact_builder *b = new jv_exact_builder();
    b->device = ctx->device;
    b->vectors = vectors;
    b->vsf = vsf;
    b->n = vectors->count;
    bl_set_parameters(b, max_degree, beam_width, alpha, neighbor_overflow);
    auto fail = [&](int rc) {
        jv_hip_exact_builder_destroy(b);
        return rc;
    };
    int rc = jv_hip_graph_create(ctx, b->n, 1, &b->graph);
    if (rc == JV_OK) rc = check_capacity(ctx, who, vectors, b->graph, max_degree, beam_width, b->R);
    if (rc != JV_OK) return fail(rc);
    const size_t cells = (size_t)b->n * b->R;
    if (hipMalloc((void **)&b->d_nbrs, sizeof(int32_t) * cells) != hipSuccess || hipMalloc((void **)&b->d_nsc, sizeof(float) * cells) != hipSuccess ||
        hipMalloc((void **)&b->d_db, sizeof(int32_t) * (size_t)b->n) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: cannot allocate the %lld x %d adjacency and its score rows", who, (long long)b->n, b->R);
        return fail(JV_ERR_OOM);
    }
    if (hipMemsetAsync(b->d_nbrs, 0xFF, sizeof(int32_t) * cells, ctx->stream) != hipSuccess ||
        hipMemsetAsync(b->d_nsc, 0, sizeof(float) * cells, ctx->stream) != hipSuccess ||
        hipMemsetAsync(b->d_db, 0, sizeof(int32_t) * (size_t)b->n, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: cannot clear the adjacency", who);
        return fail(JV_ERR_HIP);
    }
    rc = jv_hip_graph_set_level0_device(ctx, b->graph, b->d_nbrs, b->R);
    if (rc == JV_OK) rc = b->d_ctr.reserve(256);
    if (rc != JV_OK) return fail(rc);
    *out = b;
    return JV_OK;
}

int jv_hip_exact_builder_destroy(jv_exact_builder *b)
{
    if (!b) return JV_OK;
    (void)hipSetDevice(b->device);
    if (b->graph) jv_hip_graph_destroy(b->graph);
    if (b->d_nbrs) (void)hipFree(b->d_nbrs);
    if (b->d_nsc) (void)hipFree(b->d_nsc);
    if (b->d_db) (void)hipFree(b->d_db);
    delete b;
    return JV_OK;
}

int jv_hip_exact_builder_seed(jv_ctx *ctx, jv_exact_builder *b, int32_t node)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_seed: NULL argument");
    JV_REQUIRE(node >= 0 && node < b->n, "exact_builder_seed: node %d outside [0, %lld)", node, (long long)b->n);
    JV_REQUIRE(b->inserted == 0, "exact_builder_seed: the graph already has nodes");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_seed: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    JV_TRY(jv_hip_graph_set_entry(b->graph, node, 0));
    b->entry = node;
    b->inserted = 1;   // its (empty) row exists; the first batch links to it
    return JV_OK;
}

int jv_hip_exact_builder_insert_batch(jv_ctx *ctx, jv_exact_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_insert_batch: NULL argument");
    JV_REQUIRE(B >= 0, "exact_builder_insert_batch: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "exact_builder_insert_batch: NULL nodes");
    JV_REQUIRE(b->entry >= 0, "exact_builder_insert_batch: seed the graph first (jv_hip_exact_builder_seed)");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_insert_batch: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const int k = (int)std::min<int64_t>(b->beam, b->inserted);   // cannot ask for more candidates than the graph holds
    // ids must lie inside the adjacency rows, which are the float rows, none twice
    JV_TRY(bl_check_batch(ctx, nodes, B, b->Rf, (long long)b->n, "exact_builder_insert_batch"));
    JV_TRY(bl_stage_batch(ctx, b, nodes, B));
    JV_TRY(search_candidates(ctx, b, (const int32_t *)b->d_nodes.ptr, B, k, false));   // 1
    return bl_ro_insert(ctx, b, B, k, retain_of(ctx, b), true);                        // 2 - 6
}

// improveConnections (GraphIndexBuilder.java:510-560) for nodes that are IN the graph: the search excludes the node itself
// (ExcludingBits :518), its results are merged with the neighbours the node has (insertDiverse :104-163) under the stored / search
// scores, pruned, the row rewritten, and every member of the new row linked back
int jv_hip_exact_builder_improve_batch(jv_ctx *ctx, jv_exact_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_improve_batch: NULL argument");
    JV_REQUIRE(B >= 0, "exact_builder_improve_batch: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "exact_builder_improve_batch: NULL nodes");
    JV_REQUIRE(b->entry >= 0 && b->inserted >= 2, "exact_builder_improve_batch: nothing to improve in an empty graph");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_improve_batch: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const int k = (int)std::min<int64_t>(b->beam, b->inserted);
    JV_TRY(bl_check_batch(ctx, nodes, B, b->Rf, (long long)b->n, "exact_builder_improve_batch"));
    JV_TRY(bl_stage_batch(ctx, b, nodes, B));
    JV_TRY(search_candidates(ctx, b, (const int32_t *)b->d_nodes.ptr, B, k, true));
    // the merged lists hold R + k <= R + beam entries: create checked that against the prune's candidate limit
    return bl_ro_improve(ctx, b, B, k, (const int32_t *)b->d_cand.ptr, (const float *)b->d_csc.ptr, 1, bl_now_s(), retain_of(ctx, b), true);
}

int jv_hip_exact_builder_finish(jv_ctx *ctx, jv_exact_builder *b, int32_t *neighbors_out)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_finish: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_finish: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const double t0 = bl_now_s();
    if (b->R > b->Rf) JV_TRY(bl_ro_enforce_degree(ctx, b, retain_of(ctx, b), true));   // GraphIndexBuilder.cleanup -> enforceDegree
    JV_TRY(bl_copy_rows_out(ctx, b, neighbors_out));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->backlink_s += bl_now_s() - t0;
    return JV_OK;
}

int jv_hip_exact_builder_stats(const jv_exact_builder *b, double *seconds3, int64_t *counts5)
{
    clear_error();
    JV_REQUIRE(b, "exact_builder_stats: NULL argument");
    bl_fill_stats(b, seconds3, counts5);
    return JV_OK;
}

int jv_hip_exact_builder_working_lists(jv_ctx *ctx, const jv_exact_builder *b, int32_t *ids_out, float *scores_out, int32_t *diverse_before_out)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_working_lists: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_working_lists: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    return bl_copy_working_lists(ctx, b, ids_out, scores_out, diverse_before_out);
}

const int32_t *jv_hip_exact_builder_neighbors_device(const jv_exact_builder *b, int *row_width)
{
    if (!b) return nullptr;
    if (row_width) *row_width = b->R;
    return b->d_nbrs;
}

int jv_hip_exact_gather_rows(jv_ctx *ctx, const jv_vectors *vectors, const int32_t *ids, int64_t count, jv_vectors **out)
{
    clear_error();
    const char *who = "exact_gather_rows";
    JV_REQUIRE(ctx && vectors && ids && out, "%s: NULL argument", who);
    *out = nullptr;
    JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", who, vectors->device, ctx->device);
    JV_REQUIRE(count >= 1 && count <= 0x7fffffffLL, "%s: %lld rows", who, (long long)count);
    JV_FLOAT_ROWS(vectors, who);
    JV_TRY(use_device(ctx->device));
    if (is_device_ptr(ids)) return gather_rows(ctx, vectors, ids, count, out);
    for (int64_t i = 0; i < count; ++i)
        JV_REQUIRE(ids[i] >= 0 && ids[i] < vectors->count, "%s: id %d (position %lld) outside [0, %lld)", who, ids[i], (long long)i, (long long)vectors->count);
    Buffer d_ids;
    int rc = d_ids.reserve(sizeof(int32_t) * (size_t)count);
    if (rc == JV_OK && hipMemcpyAsync(d_ids.ptr, ids, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: cannot stage the ids", who);
        rc = JV_ERR_HIP;
    }
    if (rc == JV_OK) rc = gather_rows(ctx, vectors, (const int32_t *)d_ids.ptr, count, out);   // (returns after the stream has drained)
    d_ids.release();
    return rc;
}

}  // extern "C"

// ---- the whole layered build behind one call: jv_hip_build_layered (builder.cpp) over float rows ----
namespace {

// one level: a builder over `vectors` — n_l nodes with LOCAL ids 0..n_l-1 — inserts in a seeded order, improve passes, enforceDegree; rows
// to out_rows (host or device memory, n_l x max_degree)
int build_one_level(jv_ctx *ctx, const jv_vectors *vectors, jv_vsf vsf, int max_degree, int beam, float alpha, float overflow, int max_batch,
                    int improve_passes, uint64_t seed, int32_t *out_rows, jv_layered *acc)
{
    jv_exact_builder *b = nullptr;
    JV_TRY(jv_hip_exact_builder_create(ctx, vectors, vsf, max_degree, beam, alpha, overflow, &b));
    const BlLevelOps<jv_exact_builder> ops{jv_hip_exact_builder_seed, jv_hip_exact_builder_insert_batch, jv_hip_exact_builder_improve_batch,
                                           jv_hip_exact_builder_finish};
    const int rc = bl_build_one_level(ctx, ops, b, vectors->count, max_batch, improve_passes, seed, alpha, beam, out_rows, acc);
    jv_hip_exact_builder_destroy(b);
    return rc;
}

}  // namespace

extern "C" int jv_hip_exact_build_layered(jv_ctx *ctx, const jv_vectors *vectors, jv_vsf vsf, int max_degree, int beam_width, float alpha,
                                          float neighbor_overflow, int max_batch, int improve_passes, uint64_t seed, int min_top, jv_layered **out)
{
    clear_error();
    const char *who = "exact_build_layered";
    JV_REQUIRE(ctx && vectors && out, "%s: NULL argument", who);
    *out = nullptr;
    JV_REQUIRE(vectors->device == ctx->device, "%s: the vectors live on device %d, the context on %d", who, vectors->device, ctx->device);
    JV_REQUIRE(known_vsf(vsf), "%s: unknown similarity %d", who, (int)vsf);
    JV_REQUIRE(max_batch >= 1 && improve_passes >= 0 && improve_passes <= 8 && min_top >= 1, "%s: bad schedule (max_batch %d, improve passes %d, min_top %d)",
               who, max_batch, improve_passes, min_top);
    JV_REQUIRE(vectors->count >= 1 && vectors->count <= 0x7fffffffLL, "%s: %lld nodes", who, (long long)vectors->count);
    JV_TRY(bl_check_parameters(who, max_degree, beam_width, alpha, neighbor_overflow));
    JV_FLOAT_ROWS(vectors, who);
    JV_TRY(use_device(ctx->device));
    // level 0 over every row (the first builder's create runs every capacity check); an upper level: the members' rows gathered into a
    // set of their own
    auto build_level = [&](const std::vector<int32_t> *members, uint64_t level_seed, int32_t *out_rows, jv_layered *acc) -> int {
        if (!members)
            return build_one_level(ctx, vectors, vsf, max_degree, beam_width, alpha, neighbor_overflow, max_batch, improve_passes, level_seed, out_rows, acc);
        jv_vectors *sub = nullptr;
        JV_TRY(jv_hip_exact_gather_rows(ctx, vectors, members->data(), (int64_t)members->size(), &sub));
        const int rc = build_one_level(ctx, sub, vsf, max_degree, beam_width, alpha, neighbor_overflow, max_batch, improve_passes, level_seed, out_rows, acc);
        jv_hip_vectors_destroy(sub);
        return rc;
    };
    // the entry point: the top level's member nearest to the top level's mean row (k_exact_builder.hip); nothing but the key comes back
    auto pick_entry = [&](const std::vector<int32_t> &ids, int32_t *entry) -> int {
        const int cnt = (int)ids.size();
        Buffer d_ids, d_work;
        auto pick = [&]() -> int {
            // xm_body.h reads nothing outside the rows and would take a member it was not given as row 0: name none
            for (int32_t id : ids) JV_REQUIRE(id >= 0 && id < vectors->count, "%s: top-level member %d outside the %lld rows", who, id, (long long)vectors->count);
            const int kvsf = to_kernel_vsf(vsf);
            if (kvsf == VSF_COS) JV_TRY(ensure_vector_norms(ctx, const_cast<jv_vectors *>(vectors)));
            JV_TRY(d_ids.reserve(sizeof(int32_t) * ids.size()));
            JV_TRY(d_work.reserve(xm_entry_work_bytes(vectors->D)));
            JV_HIP_CHECK(hipMemcpyAsync(d_ids.ptr, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice, ctx->stream));
            XmEntryParams p{};
            p.rows = vectors->d_vecs;
            p.vnorm = kvsf == VSF_COS ? vectors->d_sqnorm : nullptr;
            p.n = vectors->count;
            p.D = vectors->D;
            p.ids = (const int32_t *)d_ids.ptr;
            p.count = cnt;
            p.mean = (float *)d_work.ptr;
            p.wave_best = (long long *)((char *)d_work.ptr + xm_entry_mean_bytes(vectors->D));
            p.waves = xm_entry_waves(cnt);
            p.best = p.wave_best + XM_MAX_WAVES;
            JV_TRY(xm_launched(launch_xm_entry(ctx->stream, p, sizeof(XmEntryParams), kvsf), "entry point"));
            long long key = 0;
            JV_HIP_CHECK(hipMemcpyAsync(&key, p.best, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
            JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            // an empty reduction leaves the smallest key, whose id part names no row: never hand that out as an entry
            const long long id = (long long)(int32_t) ~(uint32_t)((unsigned long long)key & 0xFFFFFFFFull);
            JV_REQUIRE(id >= 0 && id < (long long)vectors->count, "%s: the entry-point reduction named no row (key %lld)", who, key);
            *entry = (int32_t)id;
            return JV_OK;
        };
        const int rc = pick();
        d_ids.release();
        d_work.release();
        return rc;
    };
    return bl_build_layered(ctx, who, vectors->count, max_degree, seed, min_top, build_level, pick_entry, out);
}
