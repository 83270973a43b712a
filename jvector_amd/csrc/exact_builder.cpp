// exact_builder.cpp — batched Vamana construction from the float rows alone, behind the C ABI (include/jvector_exact_builder.h): the
// REFERENCE ORDER pipeline of bl_host.h (shared with builder.cpp and bq_builder.cpp) driven by the two exact scoring calls.  Here: the
// search, the prune handed to the shared steps, the capacity checks, the present / marked bits and deletion
// (include/jvector_exact_delete.h), the row gather and the entry point of the layered build.
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
#include "bq_internal.h"
#include "gs_params.h"
#include "jv_device.h"
#include "jv_internal.h"
#include "xd_params.h"
#include "xm_params.h"
#include "../../include/jvector_exact_delete.h"

using namespace jv;

struct jv_exact_builder : BlBuilderState {
    const jv_vectors *vectors = nullptr;
    jv_vsf vsf = JV_EUCLIDEAN;
    uint64_t *d_present = nullptr;   // [ceil(n / 64)] bit i: node i is in the graph (seed / insert_batch set it, remove_deleted clears it)
    uint64_t *d_marked = nullptr;    // [ceil(n / 64)] bit i: node i is marked deleted and not yet removed
    int64_t marked = 0, removed = 0;
    std::vector<uint64_t> h_removed; // bit i: node i was removed (empty until the first removal); a removed id is never taken again
    Buffer d_del_aff, d_del_tasks, d_del_ln, d_del_cn, d_del_rn, d_del_list, d_del_lsc, d_del_given, d_del_gn;
    ~jv_exact_builder()
    {
        for (Buffer *b : {&d_del_aff, &d_del_tasks, &d_del_ln, &d_del_cn, &d_del_rn, &d_del_list, &d_del_lsc, &d_del_given, &d_del_gn}) b->release();
    }
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

int64_t bit_words(int64_t n) { return (n + 63) / 64; }
bool host_bit(const std::vector<uint64_t> &bits, int64_t i) { return !bits.empty() && ((bits[(size_t)(i >> 6)] >> (i & 63)) & 1ull) != 0; }

// a removed id is never reused (nothing to look at until something has been removed)
int check_not_removed(jv_ctx *ctx, jv_exact_builder *b, const int32_t *nodes, int B, const char *what)
{
    if (b->removed == 0) return JV_OK;
    std::vector<int32_t> h((size_t)B);
    JV_HIP_CHECK(hipMemcpyAsync(h.data(), nodes, sizeof(int32_t) * (size_t)B, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < B; ++i)
        JV_REQUIRE(!host_bit(b->h_removed, h[(size_t)i]), "%s: node id %d (position %d) was removed; a removed id is not reused", what, h[(size_t)i], i);
    return JV_OK;
}

int read_bits(jv_ctx *ctx, const jv_exact_builder *b, const uint64_t *d_bits, std::vector<uint64_t> &out)
{
    out.resize((size_t)bit_words(b->n));
    JV_HIP_CHECK(hipMemcpyAsync(out.data(), d_bits, sizeof(uint64_t) * out.size(), hipMemcpyDeviceToHost, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return JV_OK;
}

// gfx950 lets one workgroup take the CU's whole 160 KB; the kernel opts in above 48 KB
size_t xd_lds_limit(const jv_ctx *ctx) { return std::min<size_t>((size_t)160 << 10, ctx->lds_per_block); }

// the merge kernel of k_exact_delete.hip over the tasks of `p` (a library of its own: a status and no text comes back)
int launch_delete_merge(jv_ctx *ctx, const jv_exact_builder *b, const XdParams &p)
{
    const size_t lds = xd_lds_bytes(p.R);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / (lds + 256)));
    const int rc = launch_exact_delete_merge(ctx->stream, p, sizeof(XdParams), to_kernel_vsf(b->vsf), xd_lds_limit(ctx), std::min(p.P, ctx->num_cus * per_cu));
    if (rc != JV_OK)
        set_error("exact_builder_remove_deleted: the merge kernel %s (%d)",
                  rc == JV_ERR_UNSUPPORTED ? "needs more LDS than a workgroup has" : "refused its launch parameters, or libjvector_hip_xd.so was built from another xd_params.h",
                  rc);
    return rc;
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
        hipMalloc((void **)&b->d_db, sizeof(int32_t) * (size_t)b->n) != hipSuccess ||
        hipMalloc((void **)&b->d_present, sizeof(uint64_t) * (size_t)bit_words(b->n)) != hipSuccess ||
        hipMalloc((void **)&b->d_marked, sizeof(uint64_t) * (size_t)bit_words(b->n)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: cannot allocate the %lld x %d adjacency and its score rows", who, (long long)b->n, b->R);
        return fail(JV_ERR_OOM);
    }
    if (hipMemsetAsync(b->d_nbrs, 0xFF, sizeof(int32_t) * cells, ctx->stream) != hipSuccess ||
        hipMemsetAsync(b->d_nsc, 0, sizeof(float) * cells, ctx->stream) != hipSuccess ||
        hipMemsetAsync(b->d_db, 0, sizeof(int32_t) * (size_t)b->n, ctx->stream) != hipSuccess ||
        hipMemsetAsync(b->d_present, 0, sizeof(uint64_t) * (size_t)bit_words(b->n), ctx->stream) != hipSuccess ||
        hipMemsetAsync(b->d_marked, 0, sizeof(uint64_t) * (size_t)bit_words(b->n), ctx->stream) != hipSuccess) {
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
    if (b->d_present) (void)hipFree(b->d_present);
    if (b->d_marked) (void)hipFree(b->d_marked);
    delete b;
    return JV_OK;
}

int jv_hip_exact_builder_seed(jv_ctx *ctx, jv_exact_builder *b, int32_t node)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_seed: NULL argument");
    JV_REQUIRE(node >= 0 && node < b->n, "exact_builder_seed: node %d outside [0, %lld)", node, (long long)b->n);
    JV_REQUIRE(b->inserted == 0, "exact_builder_seed: the graph already has nodes");
    JV_REQUIRE(!host_bit(b->h_removed, node), "exact_builder_seed: node id %d was removed; a removed id is not reused", node);
    JV_REQUIRE(ctx->device == b->device, "exact_builder_seed: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    JV_TRY(jv_hip_graph_set_entry(b->graph, node, 0));
    JV_TRY(b->d_nodes.reserve(sizeof(int32_t)));
    JV_HIP_CHECK(hipMemcpyAsync(b->d_nodes.ptr, &node, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    JV_TRY(launch_bq_delete_set_bits(ctx->stream, (const int32_t *)b->d_nodes.ptr, 1, b->n, b->d_present));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
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
    // ids must lie inside the adjacency rows, which are the float rows, none twice, none removed
    JV_TRY(bl_check_batch(ctx, nodes, B, b->Rf, (long long)b->n, "exact_builder_insert_batch"));
    JV_TRY(check_not_removed(ctx, b, nodes, B, "exact_builder_insert_batch"));
    JV_TRY(bl_stage_batch(ctx, b, nodes, B));
    const int32_t *d_nodes = (const int32_t *)b->d_nodes.ptr;
    JV_TRY(search_candidates(ctx, b, d_nodes, B, k, false));                          // 1
    JV_TRY(bl_ro_insert(ctx, b, B, k, retain_of(ctx, b), true));                      // 2 - 6
    return launch_bq_delete_set_bits(ctx->stream, d_nodes, B, b->n, b->d_present);    // the batch is in the graph
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
    JV_TRY(check_not_removed(ctx, b, nodes, B, "exact_builder_improve_batch"));
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

// ---- deletions: GraphIndexBuilder.markNodeDeleted / removeDeletedNodes (GraphIndexBuilder.java:678-799) for the builder's one level
// (include/jvector_exact_delete.h).  The bitmaps, the affected list and the retire step are k_bq_delete.hip's, which read the adjacency and
// the bits only; the scoring half is k_exact_delete.hip ----

int jv_hip_exact_builder_mark_deleted(jv_ctx *ctx, jv_exact_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_mark_deleted: NULL argument");
    JV_REQUIRE(B >= 0, "exact_builder_mark_deleted: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "exact_builder_mark_deleted: NULL nodes");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_mark_deleted: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    // the ids are looked at on the host, against copies of the two bitmaps: a refused call has changed nothing
    std::vector<int32_t> h((size_t)B);
    JV_HIP_CHECK(hipMemcpyAsync(h.data(), nodes, sizeof(int32_t) * (size_t)B, hipMemcpyDefault, ctx->stream));
    std::vector<uint64_t> present, marked;
    JV_TRY(read_bits(ctx, b, b->d_present, present));
    JV_TRY(read_bits(ctx, b, b->d_marked, marked));
    int64_t fresh = 0;
    for (int i = 0; i < B; ++i) {
        const int32_t v = h[(size_t)i];
        JV_REQUIRE(v >= 0 && v < b->n, "exact_builder_mark_deleted: node id %d (position %d) outside [0, %lld)", v, i, (long long)b->n);
        JV_REQUIRE(!host_bit(b->h_removed, v), "exact_builder_mark_deleted: node id %d (position %d) was already removed", v, i);
        JV_REQUIRE(host_bit(present, v), "exact_builder_mark_deleted: node id %d (position %d) was never seeded or inserted", v, i);
        if (!host_bit(marked, v)) {
            marked[(size_t)(v >> 6)] |= 1ull << (v & 63);
            ++fresh;
        }
    }
    JV_TRY(bl_stage_batch(ctx, b, h.data(), B));
    JV_TRY(launch_bq_delete_set_bits(ctx->stream, (const int32_t *)b->d_nodes.ptr, B, b->n, b->d_marked));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->marked += fresh;
    return JV_OK;
}

int jv_hip_exact_builder_deleted_count(const jv_exact_builder *b, int64_t *marked, int64_t *removed)
{
    clear_error();
    JV_REQUIRE(b, "exact_builder_deleted_count: NULL argument");
    if (marked) *marked = b->marked;
    if (removed) *removed = b->removed;
    return JV_OK;
}

int jv_hip_exact_builder_live_bits(jv_ctx *ctx, jv_exact_builder *b, uint64_t *bits_out)
{
    clear_error();
    JV_REQUIRE(ctx && b && bits_out, "exact_builder_live_bits: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_live_bits: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    OutStage os;
    JV_TRY(stage_out_begin(ctx, bits_out, sizeof(uint64_t) * (size_t)bit_words(b->n), ctx->d_out, &os));
    JV_TRY(launch_bq_delete_live_bits(ctx->stream, b->d_present, b->d_marked, b->n, (uint64_t *)os.dev));
    JV_TRY(stage_out_end(ctx, os));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return JV_OK;
}

int32_t jv_hip_exact_builder_entry(const jv_exact_builder *b) { return b ? b->entry : -1; }

int jv_hip_exact_builder_remove_deleted(jv_ctx *ctx, jv_exact_builder *b, uint64_t seed, int64_t *counts4)
{
    clear_error();
    JV_REQUIRE(ctx && b, "exact_builder_remove_deleted: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "exact_builder_remove_deleted: the builder lives on device %d", b->device);
    if (counts4) counts4[0] = counts4[1] = counts4[2] = counts4[3] = 0;
    if (b->marked == 0) return JV_OK;
    JV_TRY(use_device(ctx->device));
    const double t0 = bl_now_s();
    const int R = b->R, Rf = b->Rf;
    const int64_t n = b->n;
    const int kvsf = to_kernel_vsf(b->vsf);
    if (kvsf == VSF_COS) JV_TRY(ensure_vector_norms(ctx, const_cast<jv_vectors *>(b->vectors)));

    // ---- the affected nodes: live, with a marked neighbour; ascending ----
    JV_TRY(b->d_del_aff.reserve(sizeof(uint64_t) * (size_t)bit_words(n)));
    JV_TRY(b->d_del_tasks.reserve(sizeof(int32_t) * (size_t)n));
    BxParams ap{};   // (what launch_bq_delete_affected reads: the adjacency and the bits)
    ap.n = n;
    ap.nbrs = b->d_nbrs;
    ap.nsc = b->d_nsc;
    ap.R = R;
    ap.present = b->d_present;
    ap.marked = b->d_marked;
    ap.affected = (uint64_t *)b->d_del_aff.ptr;
    ap.tasks = (int32_t *)b->d_del_tasks.ptr;
    ap.task_count = (uint32_t *)b->d_ctr.ptr;
    JV_TRY(launch_bq_delete_affected(ctx->stream, ap));
    unsigned int n_aff = 0;
    JV_TRY(bl_read_counter(ctx, b->d_ctr.ptr, &n_aff));
    const int P = (int)std::min<int64_t>(n_aff, n);
    std::vector<uint64_t> present, marked;   // the two bitmaps as they are when the call starts: the fallback's draws and the new entry
    JV_TRY(read_bits(ctx, b, b->d_present, present));
    JV_TRY(read_bits(ctx, b, b->d_marked, marked));

    XdParams xp{};
    xp.rows = b->vectors->d_vecs;
    xp.vnorm = kvsf == VSF_COS ? b->vectors->d_sqnorm : nullptr;
    xp.n = n;
    xp.D = b->vectors->D;
    xp.nbrs = b->d_nbrs;
    xp.nsc = b->d_nsc;
    xp.R = R;
    xp.marked = b->d_marked;
    xp.tasks = ap.tasks;

    // ---- first pass: the exact merged length and the candidate count of every affected node; nothing is written but these ----
    std::vector<int32_t> tasks((size_t)P), ln((size_t)P), cn((size_t)P), rn((size_t)P);
    int max_len = 0, max_at = -1;
    double t_count = 0, t_merge = 0, t_prune = 0;
    if (P > 0) {
        const double tc = bl_now_s();
        JV_TRY(b->d_del_ln.reserve(sizeof(int32_t) * (size_t)P));
        JV_TRY(b->d_del_cn.reserve(sizeof(int32_t) * (size_t)P));
        JV_TRY(b->d_del_rn.reserve(sizeof(int32_t) * (size_t)P));
        xp.P = P;
        xp.ln = (int32_t *)b->d_del_ln.ptr;
        xp.cn = (int32_t *)b->d_del_cn.ptr;
        xp.rn = (int32_t *)b->d_del_rn.ptr;
        JV_TRY(launch_delete_merge(ctx, b, xp));
        JV_HIP_CHECK(hipMemcpyAsync(tasks.data(), xp.tasks, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipMemcpyAsync(ln.data(), xp.ln, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipMemcpyAsync(cn.data(), xp.cn, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipMemcpyAsync(rn.data(), xp.rn, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        xp.rn = nullptr;
        t_count = bl_now_s() - tc;
        for (int t = 0; t < P; ++t)
            if (ln[(size_t)t] > max_len) {   // the tasks ascend: the smallest node among the longest
                max_len = ln[(size_t)t];
                max_at = t;
            }
        int max_c = 0;
        JV_TRY(jv_hip_exact_retain_diverse_max_candidates(ctx, b->vectors, Rf, &max_c));
        if (max_len > max_c) {
            set_error("exact_builder_remove_deleted: node %d would merge %d surviving neighbours and candidates, above the %d entries the prune "
                      "kernel's LDS block holds at maxDegree %d; remove the marked nodes in smaller sets",
                      tasks[(size_t)max_at], max_len, max_c, Rf);
            return JV_ERR_UNSUPPORTED;
        }
    }

    // ---- the fallback (candidates.size() == 0): up to 2 maxDegree seeded draws per node, on the host ----
    std::vector<int32_t> order, given, given_n;   // tasks with candidates first, then the fallback's
    int64_t scored = 0, raw = 0, distinct = 0;   // (raw / distinct: the gathered two-hop entries of the nodes that had any)
    int n_fall = 0;
    for (int t = 0; t < P; ++t)
        if (cn[(size_t)t] > 0) {
            order.push_back(tasks[(size_t)t]);
            scored += cn[(size_t)t];
            raw += rn[(size_t)t];
            distinct += cn[(size_t)t];
        }
    const int n_norm = (int)order.size();
    for (int t = 0; t < P; ++t) {
        if (cn[(size_t)t] > 0) continue;
        const int32_t node = tasks[(size_t)t];
        order.push_back(node);
        uint64_t st = seed + (uint64_t)(uint32_t)node * 0x9E3779B97F4A7C15ull;
        const size_t at = given.size();
        given.resize(at + (size_t)Rf, -1);
        int got = 0;
        for (int d = 0; d < 2 * Rf && got < Rf; ++d) {
            int64_t r = (int64_t)(splitmix64(st) % (uint64_t)n);
            for (int again = 0; again < 64 && host_bit(marked, r); ++again) r = (int64_t)(splitmix64(st) % (uint64_t)n);
            if (host_bit(marked, r) || r == node || !host_bit(present, r)) continue;
            if (std::find(given.begin() + (long)at, given.begin() + (long)at + got, (int32_t)r) != given.begin() + (long)at + got) continue;
            given[at + (size_t)got++] = (int32_t)r;
        }
        given_n.push_back(got);
        scored += got;
        ++n_fall;
    }

    // ---- second pass: merged lists, prune, rows rewritten.  In pieces of nodes to bound the scratch: a live row is read by its own task
    // only, and the marked rows every task reads are not touched before all of them are done ----
    if (P > 0) {
        int32_t *d_tasks = (int32_t *)b->d_del_tasks.ptr;
        JV_HIP_CHECK(hipMemcpyAsync(d_tasks, order.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, ctx->stream));
        if (n_fall > 0) {
            JV_TRY(b->d_del_given.reserve(sizeof(int32_t) * given.size()));
            JV_TRY(b->d_del_gn.reserve(sizeof(int32_t) * given_n.size()));
            JV_HIP_CHECK(hipMemcpyAsync(b->d_del_given.ptr, given.data(), sizeof(int32_t) * given.size(), hipMemcpyHostToDevice, ctx->stream));
            JV_HIP_CHECK(hipMemcpyAsync(b->d_del_gn.ptr, given_n.data(), sizeof(int32_t) * given_n.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the host vectors may go
        for (int part = 0; part < 2; ++part) {
            const int first = part == 0 ? 0 : n_norm, count = part == 0 ? n_norm : n_fall;
            const int L = part == 0 ? std::max(1, max_len) : R + Rf;   // (R + maxDegree <= 3 R: create checked it against the prune's limit)
            const int piece = (int)std::max<int64_t>(1, std::min<int64_t>(count, ((int64_t)256 << 20) / (8 * (int64_t)L)));
            for (int s = 0; s < count; s += piece) {
                const int pc = std::min(piece, count - s);
                JV_TRY(b->d_del_list.reserve(sizeof(int32_t) * (size_t)pc * L));
                JV_TRY(b->d_del_lsc.reserve(sizeof(float) * (size_t)pc * L));
                XdParams mp = xp;
                mp.tasks = d_tasks + first + s;
                mp.P = pc;
                mp.L = L;
                mp.list = (int32_t *)b->d_del_list.ptr;
                mp.lsc = (float *)b->d_del_lsc.ptr;
                mp.ln = xp.ln + first + s;
                mp.cn = xp.cn + first + s;
                if (part == 1) {
                    mp.given = (const int32_t *)b->d_del_given.ptr + (size_t)s * Rf;
                    mp.given_n = (const int32_t *)b->d_del_gn.ptr + s;
                    mp.G = Rf;
                }
                const double tm = bl_now_s();
                JV_TRY(launch_delete_merge(ctx, b, mp));
                JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
                const double tp = bl_now_s();
                JV_TRY(bl_reprune_lists_ro(ctx, b, mp.tasks, mp.list, mp.lsc, mp.ln, nullptr, pc, L, retain_of(ctx, b)));
                JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
                t_merge += tp - tm;
                t_prune += bl_now_s() - tp;
            }
        }
    }

    // ---- the marked nodes leave: rows blank, bits cleared, the entry moved if it was one of them ----
    JV_TRY(launch_bq_delete_retire(ctx->stream, b->d_present, b->d_marked, n, R, b->d_nbrs, b->d_nsc, b->d_db));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (b->h_removed.empty()) b->h_removed.assign((size_t)bit_words(n), 0ull);
    for (size_t w = 0; w < marked.size(); ++w) b->h_removed[w] |= marked[w];
    if (b->entry >= 0 && host_bit(marked, b->entry)) {
        int32_t fresh = -1;   // the smallest id in the graph and not marked
        for (size_t w = 0; w < present.size() && fresh < 0; ++w) {
            const uint64_t live = present[w] & ~marked[w];
            if (live) fresh = (int32_t)(w * 64 + (size_t)__builtin_ctzll(live));
        }
        b->entry = fresh;
        if (fresh >= 0) JV_TRY(jv_hip_graph_set_entry(b->graph, fresh, 0));
    }
    if (counts4) {
        counts4[0] = b->marked;
        counts4[1] = P;
        counts4[2] = scored;
        counts4[3] = n_fall;
    }
    b->inserted -= b->marked;
    b->removed += b->marked;
    b->marked = 0;
    b->backlink_s += bl_now_s() - t0;
    // where the time went and what the de-duplication saved, for whoever measures (HipContext.stat)
    ctx_stat_add(ctx, "exact_delete_count_us", (long long)(t_count * 1e6));
    ctx_stat_add(ctx, "exact_delete_merge_us", (long long)(t_merge * 1e6));
    ctx_stat_add(ctx, "exact_delete_prune_us", (long long)(t_prune * 1e6));
    ctx_stat_add(ctx, "exact_delete_raw_entries", (long long)raw);
    ctx_stat_add(ctx, "exact_delete_distinct", (long long)distinct);
    return JV_OK;
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
