// bq_builder.cpp — batched Vamana construction from binary-quantized rows alone, behind the C ABI (include/jvector_bq_builder.h):
// the REFERENCE ORDER pipeline of bl_host.h (shared with builder.cpp) driven by the two BQ scoring calls.  Here: the search, the prune
// handed to the shared steps, the capacity checks, the present / marked bits, deletion and compaction.
//
// One insert_batch = B concurrent addGraphNode calls (GraphIndexBuilder.java:605-659) that do not see each other:
//   1. candidates = the search from each node's own row (topK = beam) over the graph so far   jv_hip_bq_graph_search_nodes
//   2. robust prune of every candidate list                                                   jv_hip_bq_retain_diverse
//   3. insertDiverse on the new nodes' empty lists, back edges emitted with their scores       launch_bl_ro_apply_selection
//   4. back edges sorted by (target, edge index)                                              launch_bl_sort_edges
//   5. per target: Neighbors.insert in batch order; lists past the hard maximum handed over    launch_bl_ro_backlink_merge
//   6. those lists: retainDiverse(list, diverseBefore) over the STORED scores, row rewritten   jv_hip_bq_retain_diverse,
//                                                                                             launch_bl_ro_rewrite_rows
// BQVectors.similarityBetween is symmetric: the score the search gives a neighbour IS the score its back link is stored under and the
// score the prune tests against, so there is nothing to re-score and this builder has one list discipline, the reference's (every
// entry keeps the score it was inserted under, NodeArray order, the diverseBefore mark).  Steps 3 - 6 never look at what a score
// means: they are bl_host.h (bl_ro_insert) over k_builder.hip / bl_body.h as they stand.  With one node per batch the lists equal the one-thread restatement of
// GraphIndexBuilder byte for byte (tests/test_zz_bq_builder_gpu.py).  Everything runs on the context's stream; the host reads back the
// search statuses and one counter per batch.
#include <algorithm>
#include <chrono>
#include <vector>

#include "bl_body.h"
#include "bl_host.h"
#include "bq_internal.h"
#include "gs_params.h"
#include "jv_internal.h"
#include "../../include/jvector_bq_builder.h"
#include "../../include/jvector_bq_compact.h"

using namespace jv;

struct jv_bq_builder : BlBuilderState {
    const jv_bq_vectors *bq = nullptr;
    float overflow = 1.25f;
    uint64_t *d_present = nullptr;   // [ceil(n / 64)] bit i: node i is in the graph (seed / insert_batch set it, remove_deleted clears it)
    uint64_t *d_marked = nullptr;    // [ceil(n / 64)] bit i: node i is marked deleted and not yet removed
    int64_t marked = 0, removed = 0;
    std::vector<uint64_t> h_removed; // bit i: node i was removed (empty until the first removal); a removed id is never taken again
    Buffer d_del_aff, d_del_tasks, d_del_ln, d_del_cn, d_del_list, d_del_lsc, d_del_given, d_del_gn;
    ~jv_bq_builder()
    {
        for (Buffer *b : {&d_del_aff, &d_del_tasks, &d_del_ln, &d_del_cn, &d_del_list, &d_del_lsc, &d_del_given, &d_del_gn}) b->release();
    }
};

namespace {

// what the scoring kernels cannot take is refused before anything is allocated: a list is never truncated to fit
int check_capacity(jv_ctx *ctx, const char *who, const jv_bq_vectors *bq, const jv_graph *g, int max_degree, int beam_width, int R)
{
    if (bq->D > kBqMaxDim) {
        set_error("%s: dimension %d above %d", who, bq->D, kBqMaxDim);
        return JV_ERR_UNSUPPORTED;
    }
    int max_k = 0, max_c = 0;
    JV_TRY(jv_hip_bq_graph_max_rerank_k(ctx, g, &max_k));
    if (beam_width > max_k) {
        set_error("%s: beamWidth %d above the %d results the traversal kernel's LDS block holds", who, beam_width, max_k);
        return JV_ERR_UNSUPPORTED;
    }
    JV_TRY(jv_hip_bq_retain_diverse_max_candidates(ctx, bq, max_degree, &max_c));
    const int need = std::max(beam_width + R, 3 * R);   // improve: row + candidates; back links: row + 2 R appended entries
    if (need > max_c) {
        set_error("%s: lists of %d entries (beamWidth %d, working rows of %d) above the %d candidates of %d words the prune kernel's LDS block holds", who,
                  need, beam_width, R, max_c, bq->W);
        return JV_ERR_UNSUPPORTED;
    }
    return JV_OK;
}

// the robust prune the steps of bl_host.h run: over the BQ rows, under the builder's maxDegree and alpha
auto retain_of(jv_ctx *ctx, const jv_bq_builder *b)
{
    return [=](const int32_t *d_list, const float *d_sc, const int32_t *d_count, const int32_t *d_before, int P, int L, int32_t *d_sel, int32_t *d_nsel) {
        return jv_hip_bq_retain_diverse(ctx, b->bq, P, L, d_list, d_sc, d_count, d_before, b->Rf, b->alpha, d_sel, d_nsel, nullptr);
    };
}

// 1: GraphSearcher.search(searchProviderFor(node), k, k) from each node's own row over the graph built so far -> d_cand / d_csc [B][k]
int search_candidates(jv_ctx *ctx, jv_bq_builder *b, const int32_t *d_nodes, int B, int k, bool exclude_self)
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
        JV_TRY(jv_hip_bq_graph_search_nodes(ctx, b->graph, b->bq, d_nodes + s, bc, k, exclude_self ? 1 : 0, d_cand + (size_t)s * k,
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
int check_not_removed(jv_ctx *ctx, jv_bq_builder *b, const int32_t *nodes, int B, const char *what)
{
    if (b->removed == 0) return JV_OK;
    std::vector<int32_t> h((size_t)B);
    JV_HIP_CHECK(hipMemcpyAsync(h.data(), nodes, sizeof(int32_t) * (size_t)B, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < B; ++i)
        JV_REQUIRE(!host_bit(b->h_removed, h[(size_t)i]), "%s: node id %d (position %d) was removed; a removed id is not reused", what, h[(size_t)i], i);
    return JV_OK;
}

int read_bits(jv_ctx *ctx, const jv_bq_builder *b, const uint64_t *d_bits, std::vector<uint64_t> &out)
{
    out.resize((size_t)bit_words(b->n));
    JV_HIP_CHECK(hipMemcpyAsync(out.data(), d_bits, sizeof(uint64_t) * out.size(), hipMemcpyDeviceToHost, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return JV_OK;
}

}  // namespace

extern "C" {

// create, for the entry point `who`: rows [first_blank, count) are blanked here, rows [0, first_blank) are the caller's to fill
// (compact gathers them: no cell is written twice); both bitmaps are cleared
static int create_builder(jv_ctx *ctx, const char *who, const jv_bq_vectors *bq, int max_degree, int beam_width, float alpha, float neighbor_overflow,
                          int64_t first_blank, jv_bq_builder **out)
{
    JV_REQUIRE(bq->device == ctx->device, "%s: the BQ vectors live on device %d, the context on %d", who, bq->device, ctx->device);
    JV_REQUIRE(bq->count >= 1 && bq->count <= 0x7fffffffLL, "%s: %lld nodes", who, (long long)bq->count);
    JV_TRY(bl_check_parameters(who, max_degree, beam_width, alpha, neighbor_overflow));
    JV_TRY(use_device(ctx->device));
    jv_bq_builder *b = new jv_bq_builder();
    b->device = ctx->device;
    b->bq = bq;
    b->n = bq->count;
    bl_set_parameters(b, max_degree, beam_width, alpha, neighbor_overflow);
    b->overflow = neighbor_overflow;
    auto fail = [&](int rc) {
        jv_hip_bq_builder_destroy(b);
        return rc;
    };
    int rc = jv_hip_graph_create(ctx, b->n, 1, &b->graph);
    if (rc == JV_OK) rc = check_capacity(ctx, who, bq, b->graph, max_degree, beam_width, b->R);
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
    const size_t skip = (size_t)std::min<int64_t>(std::max<int64_t>(first_blank, 0), b->n), blank = (size_t)b->n - skip;
    if ((blank > 0 && (hipMemsetAsync(b->d_nbrs + skip * b->R, 0xFF, sizeof(int32_t) * blank * b->R, ctx->stream) != hipSuccess ||
                       hipMemsetAsync(b->d_nsc + skip * b->R, 0, sizeof(float) * blank * b->R, ctx->stream) != hipSuccess ||
                       hipMemsetAsync(b->d_db + skip, 0, sizeof(int32_t) * blank, ctx->stream) != hipSuccess)) ||
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

int jv_hip_bq_builder_create(jv_ctx *ctx, const jv_bq_vectors *bq, int max_degree, int beam_width, float alpha, float neighbor_overflow,
                             jv_bq_builder **out)
{
    clear_error();
    JV_REQUIRE(ctx && bq && out, "bq_builder_create: NULL argument");
    *out = nullptr;
    return create_builder(ctx, "bq_builder_create", bq, max_degree, beam_width, alpha, neighbor_overflow, 0, out);
}

int jv_hip_bq_builder_destroy(jv_bq_builder *b)
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

int jv_hip_bq_builder_seed(jv_ctx *ctx, jv_bq_builder *b, int32_t node)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_seed: NULL argument");
    JV_REQUIRE(node >= 0 && node < b->n, "bq_builder_seed: node %d outside [0, %lld)", node, (long long)b->n);
    JV_REQUIRE(b->inserted == 0, "bq_builder_seed: the graph already has nodes");
    JV_REQUIRE(!host_bit(b->h_removed, node), "bq_builder_seed: node id %d was removed; a removed id is not reused", node);
    JV_REQUIRE(ctx->device == b->device, "bq_builder_seed: the builder lives on device %d", b->device);
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

int jv_hip_bq_builder_insert_batch(jv_ctx *ctx, jv_bq_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_insert_batch: NULL argument");
    JV_REQUIRE(B >= 0, "bq_builder_insert_batch: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "bq_builder_insert_batch: NULL nodes");
    JV_REQUIRE(b->entry >= 0, "bq_builder_insert_batch: seed the graph first (jv_hip_bq_builder_seed)");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_insert_batch: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const int k = (int)std::min<int64_t>(b->beam, b->inserted);   // cannot ask for more candidates than the graph holds
    // ids must lie inside the adjacency rows, which are the BQ rows, none twice, none removed
    JV_TRY(bl_check_batch(ctx, nodes, B, b->Rf, (long long)b->n, "bq_builder_insert_batch"));
    JV_TRY(check_not_removed(ctx, b, nodes, B, "bq_builder_insert_batch"));
    JV_TRY(bl_stage_batch(ctx, b, nodes, B));
    const int32_t *d_nodes = (const int32_t *)b->d_nodes.ptr;
    JV_TRY(search_candidates(ctx, b, d_nodes, B, k, false));                          // 1
    JV_TRY(bl_ro_insert(ctx, b, B, k, retain_of(ctx, b), true));                      // 2 - 6
    return launch_bq_delete_set_bits(ctx->stream, d_nodes, B, b->n, b->d_present);    // the batch is in the graph
}

// improveConnections (GraphIndexBuilder.java:510-560) for nodes that are IN the graph: the search excludes the node itself
// (ExcludingBits :518), its results are merged with the neighbours the node has (insertDiverse :104-163) under the stored / search
// scores, pruned, the row rewritten, and every member of the new row linked back
int jv_hip_bq_builder_improve_batch(jv_ctx *ctx, jv_bq_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_improve_batch: NULL argument");
    JV_REQUIRE(B >= 0, "bq_builder_improve_batch: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "bq_builder_improve_batch: NULL nodes");
    JV_REQUIRE(b->entry >= 0 && b->inserted >= 2, "bq_builder_improve_batch: nothing to improve in an empty graph");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_improve_batch: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const int k = (int)std::min<int64_t>(b->beam, b->inserted);
    JV_TRY(bl_check_batch(ctx, nodes, B, b->Rf, (long long)b->n, "bq_builder_improve_batch"));
    JV_TRY(check_not_removed(ctx, b, nodes, B, "bq_builder_improve_batch"));
    JV_TRY(bl_stage_batch(ctx, b, nodes, B));
    JV_TRY(search_candidates(ctx, b, (const int32_t *)b->d_nodes.ptr, B, k, true));
    // the merged lists hold R + k <= R + beam entries: create checked that against the prune's candidate limit
    return bl_ro_improve(ctx, b, B, k, (const int32_t *)b->d_cand.ptr, (const float *)b->d_csc.ptr, 1, bl_now_s(), retain_of(ctx, b), true);
}

int jv_hip_bq_builder_finish(jv_ctx *ctx, jv_bq_builder *b, int32_t *neighbors_out)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_finish: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_finish: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const double t0 = bl_now_s();
    if (b->R > b->Rf) JV_TRY(bl_ro_enforce_degree(ctx, b, retain_of(ctx, b), true));   // GraphIndexBuilder.cleanup -> enforceDegree
    JV_TRY(bl_copy_rows_out(ctx, b, neighbors_out));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->backlink_s += bl_now_s() - t0;
    return JV_OK;
}

int jv_hip_bq_builder_stats(const jv_bq_builder *b, double *seconds3, int64_t *counts5)
{
    clear_error();
    JV_REQUIRE(b, "bq_builder_stats: NULL argument");
    bl_fill_stats(b, seconds3, counts5);
    return JV_OK;
}

int jv_hip_bq_builder_working_lists(jv_ctx *ctx, const jv_bq_builder *b, int32_t *ids_out, float *scores_out, int32_t *diverse_before_out)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_working_lists: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_working_lists: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    return bl_copy_working_lists(ctx, b, ids_out, scores_out, diverse_before_out);
}

const int32_t *jv_hip_bq_builder_neighbors_device(const jv_bq_builder *b, int *row_width)
{
    if (!b) return nullptr;
    if (row_width) *row_width = b->R;
    return b->d_nbrs;
}

// ---- deletions: GraphIndexBuilder.markNodeDeleted / removeDeletedNodes (GraphIndexBuilder.java:678-799) for the builder's one level ----

int jv_hip_bq_builder_mark_deleted(jv_ctx *ctx, jv_bq_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_mark_deleted: NULL argument");
    JV_REQUIRE(B >= 0, "bq_builder_mark_deleted: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "bq_builder_mark_deleted: NULL nodes");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_mark_deleted: the builder lives on device %d", b->device);
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
        JV_REQUIRE(v >= 0 && v < b->n, "bq_builder_mark_deleted: node id %d (position %d) outside [0, %lld)", v, i, (long long)b->n);
        JV_REQUIRE(!host_bit(b->h_removed, v), "bq_builder_mark_deleted: node id %d (position %d) was already removed", v, i);
        JV_REQUIRE(host_bit(present, v), "bq_builder_mark_deleted: node id %d (position %d) was never seeded or inserted", v, i);
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

int jv_hip_bq_builder_deleted_count(const jv_bq_builder *b, int64_t *marked, int64_t *removed)
{
    clear_error();
    JV_REQUIRE(b, "bq_builder_deleted_count: NULL argument");
    if (marked) *marked = b->marked;
    if (removed) *removed = b->removed;
    return JV_OK;
}

int jv_hip_bq_builder_live_bits(jv_ctx *ctx, jv_bq_builder *b, uint64_t *bits_out)
{
    clear_error();
    JV_REQUIRE(ctx && b && bits_out, "bq_builder_live_bits: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_live_bits: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    OutStage os;
    JV_TRY(stage_out_begin(ctx, bits_out, sizeof(uint64_t) * (size_t)bit_words(b->n), ctx->d_out, &os));
    JV_TRY(launch_bq_delete_live_bits(ctx->stream, b->d_present, b->d_marked, b->n, (uint64_t *)os.dev));
    JV_TRY(stage_out_end(ctx, os));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return JV_OK;
}

int32_t jv_hip_bq_builder_entry(const jv_bq_builder *b) { return b ? b->entry : -1; }

int jv_hip_bq_builder_remove_deleted(jv_ctx *ctx, jv_bq_builder *b, uint64_t seed, int64_t *counts4)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_remove_deleted: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_remove_deleted: the builder lives on device %d", b->device);
    if (counts4) counts4[0] = counts4[1] = counts4[2] = counts4[3] = 0;
    if (b->marked == 0) return JV_OK;
    JV_TRY(use_device(ctx->device));
    const double t0 = bl_now_s();
    const int R = b->R, Rf = b->Rf;
    const int64_t n = b->n;

    // ---- the affected nodes: live, with a marked neighbour; ascending ----
    JV_TRY(b->d_del_aff.reserve(sizeof(uint64_t) * (size_t)bit_words(n)));
    JV_TRY(b->d_del_tasks.reserve(sizeof(int32_t) * (size_t)n));
    BxParams bp{};
    bp.rows = b->bq->d_rows;
    bp.n = n;
    bp.D = b->bq->D;
    bp.W = b->bq->W;
    bp.nbrs = b->d_nbrs;
    bp.nsc = b->d_nsc;
    bp.R = R;
    bp.present = b->d_present;
    bp.marked = b->d_marked;
    bp.affected = (uint64_t *)b->d_del_aff.ptr;
    bp.tasks = (int32_t *)b->d_del_tasks.ptr;
    bp.task_count = (uint32_t *)b->d_ctr.ptr;
    JV_TRY(launch_bq_delete_affected(ctx->stream, bp));
    unsigned int n_aff = 0;
    JV_TRY(bl_read_counter(ctx, b->d_ctr.ptr, &n_aff));
    const int P = (int)std::min<int64_t>(n_aff, n);
    std::vector<uint64_t> present, marked;   // the two bitmaps as they are when the call starts: the fallback's draws and the new entry
    JV_TRY(read_bits(ctx, b, b->d_present, present));
    JV_TRY(read_bits(ctx, b, b->d_marked, marked));

    // ---- first pass: the exact merged length and the candidate count of every affected node; nothing is written but these ----
    std::vector<int32_t> tasks((size_t)P), ln((size_t)P), cn((size_t)P);
    int max_len = 0, max_at = -1;
    if (P > 0) {
        JV_TRY(b->d_del_ln.reserve(sizeof(int32_t) * (size_t)P));
        JV_TRY(b->d_del_cn.reserve(sizeof(int32_t) * (size_t)P));
        bp.P = P;
        bp.ln = (int32_t *)b->d_del_ln.ptr;
        bp.cn = (int32_t *)b->d_del_cn.ptr;
        JV_TRY(launch_bq_delete_merge(ctx->stream, ctx, bp));
        JV_HIP_CHECK(hipMemcpyAsync(tasks.data(), bp.tasks, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipMemcpyAsync(ln.data(), bp.ln, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipMemcpyAsync(cn.data(), bp.cn, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int t = 0; t < P; ++t)
            if (ln[(size_t)t] > max_len) {   // the tasks ascend: the smallest node among the longest
                max_len = ln[(size_t)t];
                max_at = t;
            }
        int max_c = 0;
        JV_TRY(jv_hip_bq_retain_diverse_max_candidates(ctx, b->bq, Rf, &max_c));
        if (max_len > max_c) {
            set_error("bq_builder_remove_deleted: node %d would merge %d surviving neighbours and candidates, above the %d entries of %d words the prune "
                      "kernel's LDS block holds; remove the marked nodes in smaller sets",
                      tasks[(size_t)max_at], max_len, max_c, b->bq->W);
            return JV_ERR_UNSUPPORTED;
        }
    }

    // ---- the fallback (candidates.size() == 0): up to 2 maxDegree seeded draws per node, on the host ----
    std::vector<int32_t> order, given, given_n;   // tasks with candidates first, then the fallback's
    int64_t scored = 0;
    int n_fall = 0;
    for (int t = 0; t < P; ++t)
        if (cn[(size_t)t] > 0) {
            order.push_back(tasks[(size_t)t]);
            scored += cn[(size_t)t];
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
        JV_HIP_CHECK(hipMemcpyAsync(bp.tasks, order.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, ctx->stream));
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
                BxParams mp = bp;
                mp.tasks = bp.tasks + first + s;
                mp.P = pc;
                mp.L = L;
                mp.list = (int32_t *)b->d_del_list.ptr;
                mp.lsc = (float *)b->d_del_lsc.ptr;
                mp.ln = bp.ln + first + s;
                mp.cn = bp.cn + first + s;
                if (part == 1) {
                    mp.given = (const int32_t *)b->d_del_given.ptr + (size_t)s * Rf;
                    mp.given_n = (const int32_t *)b->d_del_gn.ptr + s;
                    mp.G = Rf;
                }
                JV_TRY(launch_bq_delete_merge(ctx->stream, ctx, mp));
                JV_TRY(bl_reprune_lists_ro(ctx, b, mp.tasks, mp.list, mp.lsc, mp.ln, nullptr, pc, L, retain_of(ctx, b)));
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
    return JV_OK;
}

// ---- compaction: AbstractGraphIndexWriter.sequentialRenumbering (AbstractGraphIndexWriter.java:146-159) of the working graph, and a new
// builder holding the graph under it (include/jvector_bq_compact.h).  The maps are made, and the rows moved, on the device ----

struct CompactScratch {
    Buffer base, ctr, o2n, n2o;
    ~CompactScratch()
    {
        for (Buffer *s : {&base, &ctr, &o2n, &n2o}) s->release();
    }
};

// the launchers of k_bq_compact.hip return a status and no text (they are a library of their own)
static int compact_launched(int rc, const char *what)
{
    if (rc != JV_OK) set_error("bq compact kernels (%s): %s", what, rc == JV_ERR_INVALID ? "bad launch parameters, or libjvector_hip_bqc.so was built from another bc_params.h" : "the launch failed");
    return rc;
}

// the two maps of b's graph into the scratch (new_to_old has room for every row: the kernel writes one id per set bit, however many the
// builder believes there are); p keeps the rank's parameters for the gathers; a count that contradicts the builder's is refused
static int rank_nodes(jv_ctx *ctx, const char *who, const jv_bq_builder *b, CompactScratch &s, BcParams &p)
{
    JV_TRY(s.base.reserve(sizeof(uint32_t) * (size_t)bc_scan_blocks(b->n)));
    JV_TRY(s.ctr.reserve(sizeof(uint32_t) * 4));
    JV_TRY(s.o2n.reserve(sizeof(int32_t) * (size_t)b->n));
    JV_TRY(s.n2o.reserve(sizeof(int32_t) * (size_t)b->n));
    p = BcParams{};
    p.present = b->d_present;
    p.n = b->n;
    p.block_base = (uint32_t *)s.base.ptr;
    p.counters = (uint32_t *)s.ctr.ptr;
    p.old_to_new = (int32_t *)s.o2n.ptr;
    p.new_to_old = (int32_t *)s.n2o.ptr;
    JV_TRY(compact_launched(launch_bq_compact_rank(ctx->stream, p), "rank"));
    uint32_t live = 0;
    JV_HIP_CHECK(hipMemcpyAsync(&live, p.counters, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if ((int64_t)live != b->inserted) {
        set_error("%s: the present bits name %lld nodes, the builder counts %lld", who, (long long)live, (long long)b->inserted);
        return JV_ERR_INTERNAL;
    }
    p.live = live;
    return JV_OK;
}

static int copy_maps_out(jv_ctx *ctx, const BcParams &p, int32_t *old_to_new, int32_t *new_to_old, int64_t *live_out)
{
    if (old_to_new) JV_HIP_CHECK(hipMemcpyAsync(old_to_new, p.old_to_new, sizeof(int32_t) * (size_t)p.n, hipMemcpyDefault, ctx->stream));
    if (new_to_old && p.live > 0)
        JV_HIP_CHECK(hipMemcpyAsync(new_to_old, p.new_to_old, sizeof(int32_t) * (size_t)p.live, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (live_out) *live_out = p.live;
    return JV_OK;
}

int jv_hip_bq_builder_renumbering(jv_ctx *ctx, const jv_bq_builder *b, int32_t *old_to_new, int32_t *new_to_old, int64_t *live_out)
{
    clear_error();
    JV_REQUIRE(ctx && b, "bq_builder_renumbering: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "bq_builder_renumbering: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    CompactScratch s;
    BcParams p{};
    JV_TRY(rank_nodes(ctx, "bq_builder_renumbering", b, s, p));
    return copy_maps_out(ctx, p, old_to_new, new_to_old, live_out);
}

int jv_hip_bq_builder_compact(jv_ctx *ctx, const jv_bq_builder *src, jv_bq_vectors *dst_bq, int32_t *old_to_new, int32_t *new_to_old,
                              int64_t *live_out, jv_bq_builder **out)
{
    clear_error();
    JV_REQUIRE(ctx && src && dst_bq && out, "bq_builder_compact: NULL argument");
    *out = nullptr;
    JV_REQUIRE(ctx->device == src->device, "bq_builder_compact: the builder lives on device %d", src->device);
    JV_REQUIRE(ctx->device == dst_bq->device, "bq_builder_compact: the destination BQ vectors live on device %d, the context on %d", dst_bq->device,
               ctx->device);
    JV_REQUIRE(src->marked == 0, "bq_builder_compact: %lld nodes are marked and not yet removed; call jv_hip_bq_builder_remove_deleted first",
               (long long)src->marked);
    JV_REQUIRE(dst_bq != src->bq && dst_bq->d_rows != src->bq->d_rows, "bq_builder_compact: the destination is the builder's own BQ vectors");
    JV_REQUIRE(dst_bq->D == src->bq->D, "bq_builder_compact: the destination has dimension %d, the builder's rows %d", dst_bq->D, src->bq->D);
    const int64_t live = src->inserted, capacity = dst_bq->count;
    JV_REQUIRE(capacity >= std::max<int64_t>(live, 1), "bq_builder_compact: %lld destination rows for %lld nodes", (long long)capacity, (long long)live);
    JV_TRY(use_device(ctx->device));

    // ---- the maps; nothing of the destination exists yet ----
    CompactScratch s;
    BcParams p{};
    JV_TRY(rank_nodes(ctx, "bq_builder_compact", src, s, p));

    // ---- the new builder: rows [live, capacity) blank, rows [0, live) gathered ----
    jv_bq_builder *b = nullptr;
    JV_TRY(create_builder(ctx, "bq_builder_compact", dst_bq, src->Rf, src->beam, src->alpha, src->overflow, live, &b));
    auto run = [&]() -> int {
        p.R = src->R;
        p.src_nbrs = src->d_nbrs;
        p.src_nsc = src->d_nsc;
        p.src_db = src->d_db;
        p.dst_nbrs = b->d_nbrs;
        p.dst_nsc = b->d_nsc;
        p.dst_db = b->d_db;
        JV_REQUIRE(b->R == src->R, "bq_builder_compact: row width %d became %d", src->R, b->R);
        JV_TRY(compact_launched(launch_bq_compact_rows(ctx->stream, p), "rows"));
        uint32_t bad[2] = {0, 0};   // counters[1], [2]: ids without an image, the first new row holding one
        int32_t entry = -1;
        JV_HIP_CHECK(hipMemcpyAsync(bad, p.counters + 1, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
        if (live > 0 && src->entry >= 0)
            JV_HIP_CHECK(hipMemcpyAsync(&entry, p.old_to_new + src->entry, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (bad[0] != 0) {
            set_error("bq_builder_compact: %u stored ids name rows that are not in the graph, the first in new row %u; nothing was compacted", bad[0],
                      bad[1]);
            return JV_ERR_INTERNAL;
        }
        if (live > 0 && entry < 0) {
            set_error("bq_builder_compact: the entry node %d is not in the graph", src->entry);
            return JV_ERR_INTERNAL;
        }
        // ---- every refusal (JV_ERR_INVALID, JV_ERR_INTERNAL) lies behind: from here on dst_bq is written, and only a failing HIP call
        // can still end the call (rule 11 does not cover that) ----
        p.W = src->bq->W;
        p.src_rows = src->bq->d_rows;
        p.dst_rows = dst_bq->d_rows;
        JV_TRY(compact_launched(launch_bq_compact_bq_rows(ctx->stream, p), "bq rows"));
        JV_TRY(compact_launched(launch_bq_compact_fill_bits(ctx->stream, b->d_present, b->n, live), "fill bits"));
        if (entry >= 0) JV_TRY(jv_hip_graph_set_entry(b->graph, entry, 0));
        b->entry = entry;
        b->inserted = live;
        return copy_maps_out(ctx, p, old_to_new, new_to_old, live_out);
    };
    const int rc = run();
    if (rc != JV_OK) {
        jv_hip_bq_builder_destroy(b);
        return rc;
    }
    *out = b;
    return JV_OK;
}

}  // extern "C"

// ---- the whole layered build behind one call: jv_hip_build_layered (builder.cpp) over BQ rows ----
namespace {

// one level: a builder over `bq` — n_l nodes with LOCAL ids 0..n_l-1 — inserts in a seeded order, improve passes, enforceDegree; rows to
// out_rows (host or device memory, n_l x max_degree)
int build_one_level(jv_ctx *ctx, const jv_bq_vectors *bq, int max_degree, int beam, float alpha, float overflow, int max_batch, int improve_passes,
                    uint64_t seed, int32_t *out_rows, jv_layered *acc)
{
    jv_bq_builder *b = nullptr;
    JV_TRY(jv_hip_bq_builder_create(ctx, bq, max_degree, beam, alpha, overflow, &b));
    const BlLevelOps<jv_bq_builder> ops{jv_hip_bq_builder_seed, jv_hip_bq_builder_insert_batch, jv_hip_bq_builder_improve_batch,
                                        jv_hip_bq_builder_finish};
    const int rc = bl_build_one_level(ctx, ops, b, bq->count, max_batch, improve_passes, seed, alpha, beam, out_rows, acc);
    jv_hip_bq_builder_destroy(b);
    return rc;
}

}  // namespace

extern "C" int jv_hip_bq_build_layered(jv_ctx *ctx, const jv_bq_vectors *bq, int max_degree, int beam_width, float alpha, float neighbor_overflow,
                                       int max_batch, int improve_passes, uint64_t seed, int min_top, jv_layered **out)
{
    clear_error();
    JV_REQUIRE(ctx && bq && out, "bq_build_layered: NULL argument");
    *out = nullptr;
    JV_REQUIRE(bq->device == ctx->device, "bq_build_layered: the BQ vectors live on device %d, the context on %d", bq->device, ctx->device);
    JV_REQUIRE(max_batch >= 1 && improve_passes >= 0 && improve_passes <= 8 && min_top >= 1, "bq_build_layered: bad schedule (max_batch %d, improve passes %d, min_top %d)",
               max_batch, improve_passes, min_top);
    JV_REQUIRE(bq->count >= 1 && bq->count <= 0x7fffffffLL, "bq_build_layered: %lld nodes", (long long)bq->count);
    JV_TRY(bl_check_parameters("bq_build_layered", max_degree, beam_width, alpha, neighbor_overflow));
    JV_TRY(use_device(ctx->device));
    const int W = bq->W;
    // level 0 over every row (the first builder's create runs every capacity check); an upper level: the members' rows gathered into a
    // set of their own
    auto build_level = [&](const std::vector<int32_t> *members, uint64_t level_seed, int32_t *out_rows, jv_layered *acc) -> int {
        if (!members)
            return build_one_level(ctx, bq, max_degree, beam_width, alpha, neighbor_overflow, max_batch, improve_passes, level_seed, out_rows, acc);
        const std::vector<int32_t> &ids = *members;
        const int64_t nl = (int64_t)ids.size();
        jv_bq_vectors *sub = nullptr;
        Buffer d_ids;
        auto level = [&]() -> int {
            JV_TRY(jv_hip_bq_create(ctx, bq->D, nl, &sub));
            JV_TRY(d_ids.reserve(sizeof(int32_t) * (size_t)nl));
            JV_HIP_CHECK(hipMemcpyAsync(d_ids.ptr, ids.data(), sizeof(int32_t) * (size_t)nl, hipMemcpyHostToDevice, ctx->stream));
            JV_TRY(launch_bq_gather_rows(ctx->stream, bq->d_rows, bq->count, W, (const int32_t *)d_ids.ptr, nl, sub->d_rows));
            JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            return build_one_level(ctx, sub, max_degree, beam_width, alpha, neighbor_overflow, max_batch, improve_passes, level_seed, out_rows, acc);
        };
        const int rc = level();
        if (sub) jv_hip_bq_destroy(sub);
        d_ids.release();
        return rc;
    };
    // the entry point: the top level's member nearest to the top level's bitwise-majority row (k_bq_builder.hip)
    auto pick_entry = [&](const std::vector<int32_t> &ids, int32_t *entry) -> int {
        const int cnt = (int)ids.size();
        Buffer d_ids, d_work;
        auto pick = [&]() -> int {
            // bm_body.h reads nothing outside the rows and would count a member it skipped as a row of zeros: name none
            for (int32_t id : ids) JV_REQUIRE(id >= 0 && id < bq->count, "bq_build_layered: top-level member %d outside the %lld rows", id, (long long)bq->count);
            JV_TRY(d_ids.reserve(sizeof(int32_t) * ids.size()));
            JV_TRY(d_work.reserve(bq_entry_work_bytes(W, cnt)));
            JV_HIP_CHECK(hipMemcpyAsync(d_ids.ptr, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice, ctx->stream));
            long long *d_best = nullptr;
            JV_TRY(launch_bq_entry(ctx->stream, bq->d_rows, bq->count, W, (const int32_t *)d_ids.ptr, cnt, d_work.ptr, &d_best));
            long long key = 0;
            JV_HIP_CHECK(hipMemcpyAsync(&key, d_best, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
            JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            // an empty reduction leaves the largest key, whose id part names no row: never hand that out as an entry
            JV_REQUIRE(key >= 0 && (long long)((unsigned long long)key & 0xFFFFFFFFull) < (long long)bq->count,
                       "bq_build_layered: the entry-point reduction named no row (key %lld)", key);
            *entry = (int32_t)((unsigned long long)key & 0xFFFFFFFFull);
            return JV_OK;
        };
        const int rc = pick();
        d_ids.release();
        d_work.release();
        return rc;
    };
    return bl_build_layered(ctx, "bq_build_layered", bq->count, max_degree, seed, min_top, build_level, pick_entry, out);
}
