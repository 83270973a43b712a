// builder.cpp — batched Vamana construction behind the C ABI (jv_hip_builder_*; BASELINE config 5: "GPU-batched neighbor
// scoring + PQ encode", SURVEY §8 f.2 + Appendix C).
//
// The reference inserts nodes one by one from many threads (GraphIndexBuilder.addGraphNode, B/graph/GraphIndexBuilder.java:
// 605-659): search the current graph for the new node with the BuildScoreProvider's PQ score function (beamWidth candidates),
// robust-prune them (VamanaDiversityProvider.retainDiverse, B/graph/diversity/VamanaDiversityProvider.java:43-96), link, and
// backlink with a re-prune when a neighbour's list outgrows maxDegree x neighborOverflow (ConcurrentNeighborMap.insertDiverse /
// backlink, B/graph/ConcurrentNeighborMap.java:104-163, :298-322); cleanup() finally trims every list to maxDegree
// (enforceDegree, GraphIndexBuilder.java:472-508).  Its result depends on thread interleaving, so the contract here is the
// structure of the result (degree <= maxDegree, packed rows, no self loops / duplicates) and the recall of a search over it —
// not a bit-level trace.  What IS bit-exact is every score it consumes: the candidate search is the engine's GraphSearcher
// (device traversal over the builder's own mutable adjacency), the prune is jv_hip_retain_diverse's kernel, the backlink
// re-prune scores with the PQ pair table (ImmutablePQVectors.diversityFunctionFor).
//
// One insert_batch = the batch analogue of B concurrent addGraphNode calls that do not see each other:
//   1. queries = the batch's full-resolution vectors (gathered on the device)            launch_gather_rows
//   2. candidates = GraphSearcher.search(topK = rerankK = beam) on the graph so far       jv_hip_graph_search (device pointers)
//   3. robust prune of every candidate list                                              launch_retain_diverse
//   4. rows of the new nodes <- selection; back edges (target, source) emitted           bl_apply_selection
//   5. back edges sorted by (target, edge index)                                         launch_bl_sort_edges
//   6. per target: append while the row has room, else hand the merged list over          bl_backlink_merge
//   7. overflowed lists: PQ diversity scores, NodeArray order, robust prune, row rewrite  launch_pair_scores, bl_rank_sort,
//                                                                                        launch_retain_diverse, bl_rewrite_row
// Everything stays on the context's stream; the host reads back one counter per batch (how many lists overflowed).
//
// REFERENCE ORDER (context option bl_ref_order = 1): the lists additionally carry the score every entry was inserted under, stay
// in NodeArray order and keep ConcurrentNeighborMap's diverseBefore mark (bl_body.h "REFERENCE ORDER"); steps 4, 6 and 7 become
// insertDiverse / Neighbors.insert / retainDiverse(diverseBefore) as the reference performs them — nothing is re-scored or
// re-sorted — and a build whose batches hold ONE node is addGraphNode + cleanup's enforceDegree operation for operation: the
// adjacency equals the CPU checker's one-thread restatement of GraphIndexBuilder byte for byte (tests/test_builder_reference_order.py
// on the CPU mock, tests/test_zz_builder_reference_order_gpu.py on the MI355X).  That pipeline — and everything else about a batch, a
// level and a layered build that does not depend on the score — lives in bl_host.h, shared with the builder over BQ rows; this file keeps
// the candidate search, run_retain (the prune handed to those steps), the classic path and the sorted-lists pre-steps.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "bl_body.h"
#include "bl_host.h"
#include "gs_params.h"
#include "jv_internal.h"
#include "rd_params.h"

using namespace jv;

struct jv_builder : BlBuilderState {   // (d_nsc / d_db exist only if `stored`)
    const jv_pq *pq = nullptr;
    const jv_codes *codes = nullptr;
    const jv_vectors *vectors = nullptr;
    jv_vsf vsf = JV_EUCLIDEAN;
    bool stored = false;             // d_nsc / d_db exist, rows are NodeArray-ordered under the stored scores (sorted lists / reference order)
    bool use_db = false;             // stored: prunes of back-linked lists and enforceDegree start behind the diverseBefore mark (reference order: yes;
                                     // sorted lists: no, unless bl_sorted_lists = 2; bl_ref_order = 2 switches it off there — the two ablations of DESIGN.md §7)
    bool sym = false;                // stored && sym: SORTED LISTS — the classic path's symmetric PQ diversity scores, stored; every prune re-tests the
                                     // whole list (diverseBefore unused).  stored && !sym: REFERENCE ORDER
    jv_luts *luts = nullptr;
    int luts_cap = 0;
    jv_pair_table *tri = nullptr;
    Buffer d_q, d_sorted_ids, d_sorted_sc;
    ~jv_builder()
    {
        for (Buffer *b : {&d_q, &d_sorted_ids, &d_sorted_sc}) b->release();
    }
};

namespace {

constexpr long long kBlRefOrderDefault = 0;
constexpr long long kBlSortedListsDefault = 0;

int run_retain(jv_ctx *ctx, jv_builder *b, const int32_t *d_cand, const float *d_sc, const int32_t *d_count, int P, int C, int32_t *d_sel,
               int32_t *d_nsel, const int32_t *d_before = nullptr)
{
    RdParams p{};
    p.tri = b->tri->d_tri;
    p.sq = pair_table_square(ctx, b->tri);
    p.codebooks = retain_diverse_table_free(ctx, b->pq) ? b->pq->d_codebooks : nullptr;
    p.codes = b->codes->d_codes;
    p.n = b->codes->count;
    p.cand_nodes = d_cand;
    p.cand_scores = d_sc;
    p.cand_count = d_count;
    p.diverse_before = d_before;
    p.P = P;
    p.C = C;
    p.M = b->codes->M;
    p.k = b->pq->k;
    p.vsf = to_kernel_vsf(b->vsf);
    p.maxDegree = b->Rf;
    p.alpha = b->alpha;
    p.chunk = retain_diverse_chunk(ctx);
    p.split = ctx_opt(ctx, "rd_split", 1) != 0 ? 1 : 0;
    p.wide_stage = ctx_opt(ctx, "rd_wide_stage", 1) != 0 ? 1 : 0;
    p.selected_out = d_sel;
    p.n_selected_out = d_nsel;
    p.short_edges_out = nullptr;
    if (!ctx->d_rd_counts.ptr) {   // (zeroed once per context: the counters accumulate; jv_hip_ctx_get_stat "rd_tests" / "rd_pairs" reads them)
        JV_TRY(ctx->d_rd_counts.reserve(2 * sizeof(unsigned long long)));
        JV_HIP_CHECK(hipMemsetAsync(ctx->d_rd_counts.ptr, 0, 2 * sizeof(unsigned long long), ctx->stream));
    }
    p.counts = (unsigned long long *)ctx->d_rd_counts.ptr;
    ProfScope ps(ctx, R_PRUNE);   // (its own region: the pair-score kernel of the backlinks stays under "adc")
    return launch_retain_diverse(ctx->stream, ctx, p);
}

// lists d_list [P][L] of targets d_tgt: score against the target (PQ diversity function), NodeArray order, robust prune, rewrite
int reprune_lists(jv_ctx *ctx, jv_builder *b, const int32_t *d_tgt, const int32_t *d_list, int P, int L)
{
    if (P == 0) return JV_OK;
    const size_t cells = (size_t)P * L;
    JV_TRY(b->d_over_sc.reserve(sizeof(float) * cells));
    JV_TRY(b->d_sorted_ids.reserve(sizeof(int32_t) * cells));
    JV_TRY(b->d_sorted_sc.reserve(sizeof(float) * cells));
    JV_TRY(b->d_count.reserve(sizeof(int32_t) * (size_t)P));
    JV_TRY(b->d_sel.reserve(sizeof(int32_t) * (size_t)P * b->Rf));
    JV_TRY(b->d_nsel.reserve(sizeof(int32_t) * (size_t)P));
    {
        ProfScope ps(ctx, R_ADC);
        JV_TRY(launch_pair_scores(ctx->stream, b->tri->d_tri, to_kernel_vsf(b->vsf), b->codes, d_tgt, P, d_list, L, (float *)b->d_over_sc.ptr));
    }
    BlSortParams sp{};
    sp.ids = d_list;
    sp.scores = (const float *)b->d_over_sc.ptr;
    sp.P = P;
    sp.L = L;
    sp.out_ids = (int32_t *)b->d_sorted_ids.ptr;
    sp.out_scores = (float *)b->d_sorted_sc.ptr;
    sp.out_count = (int32_t *)b->d_count.ptr;
    JV_TRY(launch_bl_rank_sort(ctx->stream, sp));
    JV_TRY(run_retain(ctx, b, sp.out_ids, sp.out_scores, sp.out_count, P, L, (int32_t *)b->d_sel.ptr, (int32_t *)b->d_nsel.ptr));
    BlRowsParams rp{};
    rp.tgt = d_tgt;
    rp.lst = sp.out_ids;
    rp.sel = (const int32_t *)b->d_sel.ptr;
    rp.P = P;
    rp.L = L;
    rp.Rf = b->Rf;
    rp.R = b->R;
    rp.nbrs = b->d_nbrs;
    JV_TRY(launch_bl_rewrite_rows(ctx->stream, rp));
    b->reprunes += P;
    return JV_OK;
}

// the robust prune the reference-order steps of bl_host.h run
auto retain_of(jv_ctx *ctx, jv_builder *b)
{
    return [=](const int32_t *d_list, const float *d_sc, const int32_t *d_count, const int32_t *d_before, int P, int L, int32_t *d_sel, int32_t *d_nsel) {
        return run_retain(ctx, b, d_list, d_sc, d_count, P, L, d_sel, d_nsel, d_before);
    };
}

}  // namespace

extern "C" {

int jv_hip_builder_create(jv_ctx *ctx, const jv_pq *pq, const jv_codes *codes, const jv_vectors *vectors, jv_vsf vsf, int max_degree,
                          int beam_width, float alpha, float neighbor_overflow, jv_builder **out)
{
    clear_error();
    JV_REQUIRE(ctx && pq && codes && vectors && out, "builder_create: NULL argument");
    *out = nullptr;
    JV_FLOAT_ROWS(vectors, "builder_create");
    JV_REQUIRE(vsf == JV_EUCLIDEAN || vsf == JV_DOT_PRODUCT || vsf == JV_COSINE, "Unsupported similarity function %d", (int)vsf);
    JV_REQUIRE(codes->pq == pq, "builder_create: the code store belongs to another quantizer");
    JV_REQUIRE(vectors->D == pq->D && vectors->count >= codes->count, "builder_create: vectors do not match the codes (%lld x %d vs %lld x %d)",
               (long long)vectors->count, vectors->D, (long long)codes->count, pq->D);
    JV_REQUIRE(codes->count >= 1 && codes->count <= 0x7fffffffLL, "builder_create: %lld nodes", (long long)codes->count);
    JV_TRY(bl_check_parameters("builder_create", max_degree, beam_width, alpha, neighbor_overflow));
    JV_TRY(use_device(ctx->device));
    jv_builder *b = new jv_builder();
    b->device = ctx->device;
    b->pq = pq;
    b->codes = codes;
    b->vectors = vectors;
    b->vsf = vsf;
    b->n = codes->count;
    bl_set_parameters(b, max_degree, beam_width, alpha, neighbor_overflow);
    auto fail = [&](int rc) {
        jv_hip_builder_destroy(b);
        return rc;
    };
    if (hipMalloc((void **)&b->d_nbrs, sizeof(int32_t) * (size_t)b->n * b->R) != hipSuccess) {
        (void)hipGetLastError();
        set_error("builder_create: cannot allocate the %lld x %d adjacency", (long long)b->n, b->R);
        return fail(JV_ERR_OOM);
    }
    if (hipMemsetAsync(b->d_nbrs, 0xFF, sizeof(int32_t) * (size_t)b->n * b->R, ctx->stream) != hipSuccess) return fail(JV_ERR_HIP);
    const long long ref_opt = ctx_opt(ctx, "bl_ref_order", kBlRefOrderDefault), sorted_opt = ctx_opt(ctx, "bl_sorted_lists", kBlSortedListsDefault);
    const bool ref_order = ref_opt != 0;
    b->sym = !ref_order && sorted_opt != 0;
    b->stored = ref_order || b->sym;
    b->use_db = ref_order ? ref_opt != 2 : sorted_opt == 2;
    if (b->stored) {
        if (hipMalloc((void **)&b->d_nsc, sizeof(float) * (size_t)b->n * b->R) != hipSuccess ||
            hipMalloc((void **)&b->d_db, sizeof(int32_t) * (size_t)b->n) != hipSuccess) {
            (void)hipGetLastError();
            set_error("builder_create: cannot allocate the %lld x %d score rows", (long long)b->n, b->R);
            return fail(JV_ERR_OOM);
        }
        if (hipMemsetAsync(b->d_nsc, 0, sizeof(float) * (size_t)b->n * b->R, ctx->stream) != hipSuccess ||
            hipMemsetAsync(b->d_db, 0, sizeof(int32_t) * (size_t)b->n, ctx->stream) != hipSuccess)
            return fail(JV_ERR_HIP);
    }
    int rc = jv_hip_graph_create(ctx, b->n, 1, &b->graph);
    if (rc == JV_OK) rc = jv_hip_graph_set_level0_device(ctx, b->graph, b->d_nbrs, b->R);
    if (rc == JV_OK) rc = jv_hip_graph_set_traversal(b->graph, JV_TRAVERSAL_DEVICE);
    if (rc == JV_OK) rc = jv_hip_pair_table_create(ctx, pq, vsf, &b->tri);
    if (rc == JV_OK) rc = b->d_ctr.reserve(256);
    if (rc != JV_OK) return fail(rc);
    *out = b;
    return JV_OK;
}

int jv_hip_builder_destroy(jv_builder *b)
{
    if (!b) return JV_OK;
    (void)hipSetDevice(b->device);
    if (b->luts) jv_hip_luts_destroy(b->luts);
    if (b->graph) jv_hip_graph_destroy(b->graph);
    if (b->tri) jv_hip_pair_table_destroy(b->tri);
    if (b->d_nbrs) (void)hipFree(b->d_nbrs);
    if (b->d_nsc) (void)hipFree(b->d_nsc);
    if (b->d_db) (void)hipFree(b->d_db);
    delete b;
    return JV_OK;
}

int jv_hip_builder_seed(jv_ctx *ctx, jv_builder *b, int32_t node)
{
    clear_error();
    JV_REQUIRE(ctx && b, "builder_seed: NULL argument");
    JV_REQUIRE(node >= 0 && node < b->n, "builder_seed: node %d outside [0, %lld)", node, (long long)b->n);
    JV_REQUIRE(b->inserted == 0, "builder_seed: the graph already has nodes");
    b->entry = node;
    b->inserted = 1;  // its (empty) row exists; the first batch links to it
    return jv_hip_graph_set_entry(b->graph, node, 0);
}

// ---- shared steps of insert_batch / improve_batch ----
static int check_batch(jv_ctx *ctx, jv_builder *b, const int32_t *nodes, int B, const char *what)
{
    // ids must lie inside the adjacency rows, the code rows and the vector rows, none twice (bl_host.h)
    const long long limit = std::min<long long>({(long long)b->n, (long long)b->codes->count, (long long)b->vectors->count});
    return bl_check_batch(ctx, nodes, B, b->Rf, limit, what);
}

// 1 + 2: the batch's vectors as queries, GraphSearcher.search(topK = rerankK = k) over the graph built so far -> d_cand / d_csc [B][k]
static int search_candidates(jv_ctx *ctx, jv_builder *b, const int32_t *d_nodes, int B, int k, bool exclude_self = false)
{
    const int D = b->pq->D;
    const int search_chunk = 65536;
    if (!b->luts || b->luts_cap < std::min(B, search_chunk)) {
        if (b->luts) jv_hip_luts_destroy(b->luts);
        b->luts = nullptr;
        b->luts_cap = std::min(search_chunk, std::max(1024, 2 * B));
        JV_TRY(jv_hip_luts_create(ctx, b->pq, b->luts_cap, &b->luts));
    }
    JV_TRY(b->d_cand.reserve(sizeof(int32_t) * (size_t)B * k));
    JV_TRY(b->d_csc.reserve(sizeof(float) * (size_t)B * k));
    JV_TRY(b->d_q.reserve(sizeof(float) * (size_t)std::min(B, search_chunk) * D));
    int32_t *d_cand = (int32_t *)b->d_cand.ptr;
    float *d_csc = (float *)b->d_csc.ptr;
    const double t0 = bl_now_s();
    for (int s = 0; s < B; s += search_chunk) {
        const int bc = std::min(search_chunk, B - s);
        JV_TRY(launch_gather_rows(ctx->stream, b->vectors->d_vecs, b->vectors->count, D, d_nodes + s, bc, (float *)b->d_q.ptr, nullptr, 0));
        b->h_stats.resize(2 * (size_t)bc);
        if (exclude_self)   // acceptOrds = ExcludingBits(node) (improveConnections :518): the node is traversed, never returned
            JV_TRY(graph_search_excluding(ctx, b->graph, b->luts, b->codes, (const float *)b->d_q.ptr, bc, b->vsf, k, k, d_nodes + s,
                                          d_cand + (size_t)s * k, d_csc + (size_t)s * k, b->h_stats.data()));
        else
            JV_TRY(jv_hip_graph_search(ctx, b->graph, b->luts, b->codes, nullptr, nullptr, (const float *)b->d_q.ptr, bc, b->vsf, k, k,
                                       d_cand + (size_t)s * k, d_csc + (size_t)s * k, b->h_stats.data()));
        for (int q = 0; q < bc; ++q) {
            b->visited += b->h_stats[2 * (size_t)q];
            b->expanded += b->h_stats[2 * (size_t)q + 1];
        }
    }
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->search_s += bl_now_s() - t0;
    return JV_OK;
}

// 5 - 7: the E back edges in d_keys / d_src: sorted by (target, edge index), appended while rows have room, overflowed lists re-pruned
static int link_back_edges(jv_ctx *ctx, jv_builder *b, long long E)
{
    const int R = b->R;
    const double t0 = bl_now_s();
    JV_TRY(bl_sort_edges(ctx, b, E));
    const int Knew = 2 * R, L = R + Knew;
    const unsigned int over_cap = (unsigned int)std::min<long long>(E, b->n);  // at most one overflow per distinct target
    JV_TRY(b->d_over_tgt.reserve(sizeof(int32_t) * (size_t)over_cap));
    JV_TRY(b->d_over_list.reserve(sizeof(int32_t) * (size_t)over_cap * L));
    JV_HIP_CHECK(hipMemsetAsync(b->d_ctr.ptr, 0, sizeof(unsigned int), ctx->stream));
    BlMergeParams mp{};
    mp.keys = (const unsigned long long *)b->d_keys2.ptr;
    mp.src = (const int32_t *)b->d_src2.ptr;
    mp.E = E;
    mp.R = R;
    mp.Knew = Knew;
    mp.nbrs = b->d_nbrs;
    mp.over_tgt = (int32_t *)b->d_over_tgt.ptr;
    mp.over_list = (int32_t *)b->d_over_list.ptr;
    mp.over_count = (unsigned int *)b->d_ctr.ptr;
    mp.over_cap = over_cap;
    JV_TRY(launch_bl_backlink_merge(ctx->stream, mp));
    unsigned int n_over = 0;
    JV_TRY(bl_read_counter(ctx, b->d_ctr.ptr, &n_over));
    n_over = std::min(n_over, over_cap);
    JV_TRY(reprune_lists(ctx, b, mp.over_tgt, mp.over_list, (int)n_over, L));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->backlink_s += bl_now_s() - t0;
    return JV_OK;
}

int jv_hip_builder_insert_batch(jv_ctx *ctx, jv_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "builder_insert_batch: NULL argument");
    JV_REQUIRE(B >= 0, "builder_insert_batch: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "builder_insert_batch: NULL nodes");
    JV_REQUIRE(b->entry >= 0, "builder_insert_batch: seed the graph first (jv_hip_builder_seed)");
    JV_REQUIRE(ctx->device == b->device, "builder_insert_batch: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const int Rf = b->Rf, R = b->R;
    const int k = (int)std::min<int64_t>(b->beam, b->inserted);  // cannot ask for more candidates than the graph holds
    JV_TRY(check_batch(ctx, b, nodes, B, "builder_insert_batch"));
    JV_TRY(bl_stage_batch(ctx, b, nodes, B));
    const int32_t *d_nodes = (const int32_t *)b->d_nodes.ptr;

    // ---- 1 + 2. candidate search on the graph built so far ----
    JV_TRY(search_candidates(ctx, b, d_nodes, B, k));
    // reference order: insertDiverse on the new nodes' empty lists, then backlink -> Neighbors.insert (bl_host.h)
    if (b->stored && !b->sym) return bl_ro_insert(ctx, b, B, k, retain_of(ctx, b), b->use_db);
    const int32_t *d_cand = (const int32_t *)b->d_cand.ptr;
    const float *d_csc = (const float *)b->d_csc.ptr;

    // ---- 3 + 4. robust prune of every new node's candidates (best first), rows + back edges ----
    double t0 = bl_now_s();
    JV_TRY(b->d_count.reserve(sizeof(int32_t) * (size_t)B));
    JV_TRY(b->d_sel.reserve(sizeof(int32_t) * (size_t)B * Rf));
    JV_TRY(b->d_nsel.reserve(sizeof(int32_t) * (size_t)B));
    JV_TRY(launch_bl_count_valid(ctx->stream, d_cand, k, (int32_t *)b->d_count.ptr, B));
    JV_TRY(run_retain(ctx, b, d_cand, d_csc, (const int32_t *)b->d_count.ptr, B, k, (int32_t *)b->d_sel.ptr, (int32_t *)b->d_nsel.ptr));
    const long long E = (long long)B * Rf;
    JV_TRY(bl_reserve_edges(b, E, b->sym));   // (the classic path stores no scores)
    if (b->sym) {   // sorted lists: the row under the symmetric scores (what the classic path's first re-prune of it would compute), sorted
        JV_TRY(b->d_imp_list.reserve(sizeof(int32_t) * (size_t)E));
        JV_TRY(b->d_over_sc.reserve(sizeof(float) * (size_t)E));
        JV_TRY(b->d_sorted_ids.reserve(sizeof(int32_t) * (size_t)E));
        JV_TRY(b->d_sorted_sc.reserve(sizeof(float) * (size_t)E));
        JV_TRY(b->d_over_n.reserve(sizeof(int32_t) * (size_t)B));
        BlSelIdsParams ip{};
        ip.nodes = d_nodes;
        ip.cand = d_cand;
        ip.sel = (const int32_t *)b->d_sel.ptr;
        ip.B = B;
        ip.C = k;
        ip.Rf = Rf;
        ip.out_ids = (int32_t *)b->d_imp_list.ptr;
        JV_TRY(launch_bl_sel_ids(ctx->stream, ip));
        {
            ProfScope ps(ctx, R_ADC);
            JV_TRY(launch_pair_scores(ctx->stream, b->tri->d_tri, to_kernel_vsf(b->vsf), b->codes, d_nodes, B, ip.out_ids, Rf, (float *)b->d_over_sc.ptr));
        }
        BlSortParams sp{};
        sp.ids = ip.out_ids;
        sp.scores = (const float *)b->d_over_sc.ptr;
        sp.P = B;
        sp.L = Rf;
        sp.out_ids = (int32_t *)b->d_sorted_ids.ptr;
        sp.out_scores = (float *)b->d_sorted_sc.ptr;
        sp.out_count = (int32_t *)b->d_over_n.ptr;
        JV_TRY(launch_bl_rank_sort(ctx->stream, sp));
        BlRoApplySortedParams rp{};
        rp.nodes = d_nodes;
        rp.ids = sp.out_ids;
        rp.sc = sp.out_scores;
        rp.B = B;
        rp.Rf = Rf;
        rp.R = R;
        rp.nbrs = b->d_nbrs;
        rp.nsc = b->d_nsc;
        rp.db = b->d_db;
        rp.edge_keys = (unsigned long long *)b->d_keys.ptr;
        rp.edge_src = (int32_t *)b->d_src.ptr;
        rp.edge_sc = (float *)b->d_esc.ptr;
        JV_TRY(launch_bl_ro_apply_sorted(ctx->stream, rp));
        JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        b->prune_s += bl_now_s() - t0;
        JV_TRY(bl_link_back_edges_ro(ctx, b, E, retain_of(ctx, b), b->use_db));
        b->inserted += B;
        b->batches += 1;
        return JV_OK;
    }
    BlApplyParams ap{};
    ap.nodes = d_nodes;
    ap.cand = d_cand;
    ap.sel = (const int32_t *)b->d_sel.ptr;
    ap.B = B;
    ap.C = k;
    ap.Rf = Rf;
    ap.R = R;
    ap.nbrs = b->d_nbrs;
    ap.edge_keys = (unsigned long long *)b->d_keys.ptr;
    ap.edge_src = (int32_t *)b->d_src.ptr;
    JV_TRY(launch_bl_apply_selection(ctx->stream, ap));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->prune_s += bl_now_s() - t0;

    // ---- 5 - 7. backlinks ----
    JV_TRY(link_back_edges(ctx, b, E));
    b->inserted += B;
    b->batches += 1;
    return JV_OK;
}

// improveConnections for a batch of nodes that are IN the graph (GraphIndexBuilder.java:510-560, called by cleanup() :472-508 — the
// reference runs it for the nodes of the upper layers and calls a pass over every node "empirically unnecessary"; here any node may be
// given): search the finished graph for the node (beamWidth candidates, PQ scores), MERGE them with the neighbours it already has
// (ConcurrentNeighborMap.insertDiverse :104-163 — a re-insertion that REPLACED the row measured worse), score the merged
// list against the node with the PQ diversity function, robust-prune it to maxDegree, rewrite the row, then backlink the row's members
// like an insert does (an edge its target already holds is dropped by the merge step).
int jv_hip_builder_improve_batch(jv_ctx *ctx, jv_builder *b, const int32_t *nodes, int B)
{
    clear_error();
    JV_REQUIRE(ctx && b, "builder_improve_batch: NULL argument");
    JV_REQUIRE(B >= 0, "builder_improve_batch: negative batch");
    if (B == 0) return JV_OK;
    JV_REQUIRE(nodes, "builder_improve_batch: NULL nodes");
    JV_REQUIRE(b->entry >= 0 && b->inserted >= 2, "builder_improve_batch: nothing to improve in an empty graph");

    JV_REQUIRE(ctx->device == b->device, "builder_improve_batch: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const int Rf = b->Rf, R = b->R;
    const int k = (int)std::min<int64_t>(b->beam, b->inserted);
    {   // the merged lists (row + beam candidates) must fit the robust prune's LDS block: refused up front, not after the searches
        const size_t need = retain_diverse_lds_bytes(R + k, b->codes->M);
        JV_REQUIRE(need <= ctx->lds_per_block, "builder_improve_batch: lists of %d + %d candidates x %d code bytes need %zu bytes of LDS (limit %zu); lower the beam width",
                   R, k, b->codes->M, need, ctx->lds_per_block);
    }
    JV_TRY(check_batch(ctx, b, nodes, B, "builder_improve_batch"));
    JV_TRY(bl_stage_batch(ctx, b, nodes, B));
    const int32_t *d_nodes = (const int32_t *)b->d_nodes.ptr;
    JV_TRY(search_candidates(ctx, b, d_nodes, B, k, b->stored && !b->sym));

    double t0 = bl_now_s();
    const int L = R + k;
    if (b->stored) {   // insertDiverse(merge(list, candidates)) with the stored / search scores, then backlink every member of the new list (bl_host.h)
        const int32_t *cand_ids = (const int32_t *)b->d_cand.ptr;
        const float *cand_sc = (const float *)b->d_csc.ptr;
        if (b->sym) {   // the candidates under the symmetric score against their node, in NodeArray order (the classic path scores and sorts row + candidates)
            JV_TRY(b->d_over_sc.reserve(sizeof(float) * (size_t)B * L));   // (the width the merge needs: not reallocated under the kernels below)
            JV_TRY(b->d_over_n.reserve(sizeof(int32_t) * (size_t)B));
            JV_TRY(b->d_sorted_ids.reserve(sizeof(int32_t) * (size_t)B * k));
            JV_TRY(b->d_sorted_sc.reserve(sizeof(float) * (size_t)B * k));
            {
                ProfScope ps(ctx, R_ADC);
                JV_TRY(launch_pair_scores(ctx->stream, b->tri->d_tri, to_kernel_vsf(b->vsf), b->codes, d_nodes, B, cand_ids, k, (float *)b->d_over_sc.ptr));
            }
            BlSortParams sp{};
            sp.ids = cand_ids;
            sp.scores = (const float *)b->d_over_sc.ptr;
            sp.P = B;
            sp.L = k;
            sp.out_ids = (int32_t *)b->d_sorted_ids.ptr;
            sp.out_scores = (float *)b->d_sorted_sc.ptr;
            sp.out_count = (int32_t *)b->d_over_n.ptr;
            JV_TRY(launch_bl_rank_sort(ctx->stream, sp));
            cand_ids = sp.out_ids;
            cand_sc = sp.out_scores;
        }
        return bl_ro_improve(ctx, b, B, k, cand_ids, cand_sc, b->sym ? 0 : 1, t0, retain_of(ctx, b), b->use_db);
    }
    JV_TRY(b->d_imp_list.reserve(sizeof(int32_t) * (size_t)B * L));
    BlImproveParams ip{};
    ip.nodes = d_nodes;
    ip.cand = (const int32_t *)b->d_cand.ptr;
    ip.B = B;
    ip.C = k;
    ip.R = R;
    ip.nbrs = b->d_nbrs;
    ip.list = (int32_t *)b->d_imp_list.ptr;
    JV_TRY(launch_bl_improve_list(ctx->stream, ip));
    JV_TRY(reprune_lists(ctx, b, d_nodes, ip.list, B, L));
    const long long E = (long long)B * Rf;
    JV_TRY(bl_reserve_edges(b, E, false));
    BlRowEdgesParams ep{};
    ep.nodes = d_nodes;
    ep.B = B;
    ep.Rf = Rf;
    ep.R = R;
    ep.nbrs = b->d_nbrs;
    ep.edge_keys = (unsigned long long *)b->d_keys.ptr;
    ep.edge_src = (int32_t *)b->d_src.ptr;
    JV_TRY(launch_bl_row_edges(ctx->stream, ep));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->prune_s += bl_now_s() - t0;
    JV_TRY(link_back_edges(ctx, b, E));
    b->batches += 1;
    return JV_OK;
}

int jv_hip_builder_finish(jv_ctx *ctx, jv_builder *b, int32_t *neighbors_out)
{
    clear_error();
    JV_REQUIRE(ctx && b, "builder_finish: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "builder_finish: the builder lives on device %d", b->device);
    JV_TRY(use_device(ctx->device));
    const double t0 = bl_now_s();
    if (b->R > b->Rf && b->stored) {   // GraphIndexBuilder.cleanup -> enforceDegree over the stored scores (bl_host.h)
        JV_TRY(bl_ro_enforce_degree(ctx, b, retain_of(ctx, b), b->use_db));
    } else if (b->R > b->Rf) {   // ... the classic path's: lists still above maxDegree are re-scored and pruned back
        unsigned int n_over = 0;
        JV_TRY(bl_list_over_degree(ctx, b, &n_over));
        JV_TRY(b->d_over_list.reserve(sizeof(int32_t) * (size_t)std::min<unsigned int>(n_over, kBlEnforcePiece) * b->R));
        for (unsigned int s = 0; s < n_over; s += kBlEnforcePiece) {
            const int P = (int)std::min<unsigned int>(kBlEnforcePiece, n_over - s);
            const int32_t *tgt = (const int32_t *)b->d_over_tgt.ptr + s;
            JV_TRY(launch_bl_copy_rows(ctx->stream, b->d_nbrs, b->R, tgt, P, (int32_t *)b->d_over_list.ptr));
            JV_TRY(reprune_lists(ctx, b, tgt, (const int32_t *)b->d_over_list.ptr, P, b->R));
        }
    }
    JV_TRY(bl_copy_rows_out(ctx, b, neighbors_out));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->backlink_s += bl_now_s() - t0;
    return JV_OK;
}

int jv_hip_builder_stats(const jv_builder *b, double *seconds3, int64_t *counts5)
{
    clear_error();
    JV_REQUIRE(b, "builder_stats: NULL argument");
    bl_fill_stats(b, seconds3, counts5);
    return JV_OK;
}

// ---- the whole layered build behind one call (verdict r3 #7: the hierarchy used to be assembled by the Python mirror) ----
// GraphIndexBuilder with addHierarchy: a node's top level is floor(-ln(U) / ln(maxDegree)) (getRandomGraphLevel :562-575, HNSW's
// sampling), a node is present on every level up to its own, each level is a Vamana graph over its nodes (here: one jv_builder per
// level — inserts in a seeded random order, prefix-doubling batches — then `improve_passes` passes of improveConnections over every
// node of the level, then enforceDegree), the entry point is a node of the top level (here: the one most similar to the mean of the
// top level's vectors under the index's own similarity function — the reference re-centres its entry on the medoid).  The draws
// come from a seeded splitmix64 instead of the reference's SplittableRandom: the build is a function of (data, parameters, seed).
// (struct jv_layered, the splitmix64 draws, the seeded permutation and the level draw: jv_internal.h, shared with bq_builder.cpp)
}  // extern "C"

namespace {
// one level: a builder over (codes, vectors) — n_l nodes with LOCAL ids 0..n_l-1 — inserts in `order`, improve passes, enforceDegree;
// rows to out_rows (host or device memory, n_l x max_degree)
int build_one_level(jv_ctx *ctx, const jv_pq *pq, const jv_codes *codes, const jv_vectors *vectors, jv_vsf vsf, int max_degree, int beam,
                    float alpha, float overflow, int max_batch, int improve_passes, uint64_t seed, int32_t *out_rows, jv_layered *acc)
{
    jv_builder *b = nullptr;
    JV_TRY(jv_hip_builder_create(ctx, pq, codes, vectors, vsf, max_degree, beam, alpha, overflow, &b));
    // experiment knobs: another alpha for the insert phase (DiskANN builds its first pass with alpha = 1), another
    // beam for the improve passes; unset = the call's alpha / beam throughout
    const long long ins_alpha = ctx_opt(ctx, "bl_insert_alpha_x100", 0), imp_beam = ctx_opt(ctx, "bl_improve_beam", 0);
    const BlLevelOps<jv_builder> ops{jv_hip_builder_seed, jv_hip_builder_insert_batch, jv_hip_builder_improve_batch, jv_hip_builder_finish};
    const int rc = bl_build_one_level(ctx, ops, b, codes->count, max_batch, improve_passes, seed,
                                      ins_alpha >= 100 && ins_alpha <= 6400 ? (float)ins_alpha / 100.0f : alpha,
                                      imp_beam >= 1 && imp_beam <= 4096 ? (int)imp_beam : beam, out_rows, acc);
    jv_hip_builder_destroy(b);
    return rc;
}
}  // namespace

extern "C" {

int jv_hip_build_layered(jv_ctx *ctx, const jv_pq *pq, const jv_codes *codes, const jv_vectors *vectors, jv_vsf vsf, int max_degree,
                         int beam_width, float alpha, float neighbor_overflow, int max_batch, int improve_passes, uint64_t seed, int min_top,
                         jv_layered **out)
{
    clear_error();
    JV_REQUIRE(ctx && pq && codes && vectors && out, "build_layered: NULL argument");
    *out = nullptr;
    JV_FLOAT_ROWS(vectors, "build_layered");
    JV_REQUIRE(max_batch >= 1 && improve_passes >= 0 && improve_passes <= 8 && min_top >= 1, "build_layered: bad schedule (max_batch %d, improve passes %d, min_top %d)",
               max_batch, improve_passes, min_top);
    JV_REQUIRE(max_degree >= 2 && max_degree <= 64, "build_layered: maxDegree %d outside 2..64", max_degree);
    if (improve_passes > 0) {   // (the improve pass prunes row + beam candidates: checked before the insert phase runs)
        const int Rw = bl_working_width(max_degree, neighbor_overflow);
        const size_t need = retain_diverse_lds_bytes(Rw + beam_width, codes->M);
        JV_REQUIRE(need <= ctx->lds_per_block, "build_layered: an improveConnections pass over lists of %d + %d candidates x %d code bytes needs %zu bytes of LDS (limit %zu); "
                   "lower the beam width or pass improve_passes = 0", Rw, beam_width, codes->M, need, ctx->lds_per_block);
    }
    JV_REQUIRE(codes->count >= 1 && codes->count <= 0x7fffffffLL && vectors->count >= codes->count, "build_layered: %lld nodes", (long long)codes->count);
    JV_TRY(use_device(ctx->device));
    const int D = pq->D;
    // level 0 over every node (rows in device memory: jv_hip_fused_build reads them there); an upper level: the members' rows of the
    // vectors gathered into a set of their own, encoded with the same quantizer (the same codes as their level-0 rows)
    auto build_level = [&](const std::vector<int32_t> *members, uint64_t level_seed, int32_t *out_rows, jv_layered *acc) -> int {
        if (!members)
            return build_one_level(ctx, pq, codes, vectors, vsf, max_degree, beam_width, alpha, neighbor_overflow, max_batch, improve_passes,
                                   level_seed, out_rows, acc);
        const std::vector<int32_t> &ids = *members;
        const int64_t nl = (int64_t)ids.size();
        jv_vectors *sv = nullptr;
        jv_codes *sc = nullptr;
        Buffer d_ids;
        auto level = [&]() -> int {
            JV_TRY(jv_hip_vectors_create(ctx, nl, D, &sv));
            JV_TRY(d_ids.reserve(sizeof(int32_t) * (size_t)nl));
            JV_HIP_CHECK(hipMemcpyAsync(d_ids.ptr, ids.data(), sizeof(int32_t) * (size_t)nl, hipMemcpyHostToDevice, ctx->stream));
            for (int64_t s0 = 0; s0 < nl; s0 += (1 << 20)) {
                const int pc = (int)std::min<int64_t>(1 << 20, nl - s0);
                JV_TRY(launch_gather_rows(ctx->stream, vectors->d_vecs, vectors->count, D, (const int32_t *)d_ids.ptr + s0, pc,
                                          sv->d_vecs + (size_t)s0 * D, nullptr, 0));
            }
            JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            JV_TRY(jv_hip_vectors_invalidate(sv));
            JV_TRY(jv_hip_codes_create(ctx, pq, nl, &sc));
            JV_TRY(jv_hip_pq_encode_into(ctx, pq, sv, 0, nl, sc));
            return build_one_level(ctx, pq, sc, sv, vsf, max_degree, beam_width, alpha, neighbor_overflow, max_batch, improve_passes, level_seed,
                                   out_rows, acc);
        };
        const int rc = level();
        if (sc) jv_hip_codes_destroy(sc);
        if (sv) jv_hip_vectors_destroy(sv);
        d_ids.release();
        return rc;
    };
    // the entry point: the top level's node most similar to the mean of (up to 4096 of) the top level's vectors
    auto pick_entry = [&](const std::vector<int32_t> &ids, int32_t *entry) -> int {
        const int cnt = (int)std::min<size_t>(ids.size(), 4096);
        std::vector<float> rowsf((size_t)cnt * D), mean((size_t)D);
        Buffer d_ids, d_rows, d_sc;
        auto pick = [&]() -> int {
            JV_TRY(d_ids.reserve(sizeof(int32_t) * ids.size()));
            JV_TRY(d_rows.reserve(sizeof(float) * (size_t)cnt * D));
            JV_TRY(d_sc.reserve(sizeof(float) * ids.size()));
            JV_HIP_CHECK(hipMemcpyAsync(d_ids.ptr, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice, ctx->stream));
            JV_TRY(launch_gather_rows(ctx->stream, vectors->d_vecs, vectors->count, D, (const int32_t *)d_ids.ptr, cnt, (float *)d_rows.ptr, nullptr, 0));
            JV_HIP_CHECK(hipMemcpyAsync(rowsf.data(), d_rows.ptr, sizeof(float) * (size_t)cnt * D, hipMemcpyDeviceToHost, ctx->stream));
            JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            for (int d = 0; d < D; ++d) {
                double acc = 0.0;
                for (int r = 0; r < cnt; ++r) acc += (double)rowsf[(size_t)r * D + d];
                mean[(size_t)d] = (float)(acc / cnt);
            }
            std::vector<float> sc(ids.size());
            JV_TRY(jv_hip_exact_scores(ctx, vectors, mean.data(), 1, vsf, (const int32_t *)d_ids.ptr, (int)ids.size(), (float *)d_sc.ptr));
            JV_HIP_CHECK(hipMemcpyAsync(sc.data(), d_sc.ptr, sizeof(float) * ids.size(), hipMemcpyDeviceToHost, ctx->stream));
            JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            size_t best = 0;
            for (size_t i = 1; i < ids.size(); ++i)
                if (sc[i] > sc[best]) best = i;   // (a NaN never wins; ties keep the smaller id)
            *entry = ids[best];
            return JV_OK;
        };
        const int rc = pick();
        d_ids.release();
        d_rows.release();
        d_sc.release();
        return rc;
    };
    return bl_build_layered(ctx, "build_layered", codes->count, max_degree, seed, min_top, build_level, pick_entry, out);
}

int jv_hip_layered_info(const jv_layered *l, int *n_levels, int32_t *entry_node, int *entry_level, int64_t *level_counts)
{
    clear_error();
    JV_REQUIRE(l, "layered_info: NULL argument");
    if (n_levels) *n_levels = (int)l->level_counts.size();
    if (entry_node) *entry_node = l->entry;
    if (entry_level) *entry_level = l->entry_level;
    if (level_counts)
        for (size_t i = 0; i < l->level_counts.size(); ++i) level_counts[i] = l->level_counts[i];
    return JV_OK;
}

int jv_hip_layered_level(jv_ctx *ctx, const jv_layered *l, int level, int32_t *nodes_out, int32_t *neighbors_out)
{
    clear_error();
    JV_REQUIRE(ctx && l, "layered_level: NULL argument");
    JV_REQUIRE(level >= 0 && level < (int)l->level_counts.size(), "layered_level: level %d of %d", level, (int)l->level_counts.size());
    if (level == 0) {
        JV_REQUIRE(!nodes_out, "layered_level: level 0 holds every ordinal (nodes_out must be NULL)");
        if (neighbors_out) {
            JV_REQUIRE(ctx->device == l->device, "layered_level: the graph lives on device %d", l->device);
            JV_TRY(use_device(ctx->device));
            JV_HIP_CHECK(hipMemcpyAsync(neighbors_out, l->d_level0, sizeof(int32_t) * (size_t)l->n * l->max_degree, hipMemcpyDefault, ctx->stream));
            JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
        return JV_OK;
    }
    const std::vector<int32_t> &ids = l->nodes[(size_t)level], &rows = l->nbrs[(size_t)level];
    if (nodes_out) memcpy(nodes_out, ids.data(), sizeof(int32_t) * ids.size());
    if (neighbors_out) memcpy(neighbors_out, rows.data(), sizeof(int32_t) * rows.size());
    return JV_OK;
}

const int32_t *jv_hip_layered_level0_device(const jv_layered *l) { return l ? l->d_level0 : nullptr; }

int jv_hip_layered_stats(const jv_layered *l, double *seconds4, int64_t *counts5)
{
    clear_error();
    JV_REQUIRE(l, "layered_stats: NULL argument");
    if (seconds4) {
        for (int i = 0; i < 3; ++i) seconds4[i] = l->seconds[i];
        seconds4[3] = l->total_s;
    }
    if (counts5)
        for (int i = 0; i < 5; ++i) counts5[i] = l->counts[i];
    return JV_OK;
}

int jv_hip_layered_destroy(jv_layered *l)
{
    if (!l) return JV_OK;
    if (l->d_level0) (void)hipFree(l->d_level0);
    delete l;
    return JV_OK;
}

int jv_hip_builder_working_lists(jv_ctx *ctx, const jv_builder *b, int32_t *ids_out, float *scores_out, int32_t *diverse_before_out)
{
    clear_error();
    JV_REQUIRE(ctx && b, "builder_working_lists: NULL argument");
    JV_REQUIRE(ctx->device == b->device, "builder_working_lists: the builder lives on device %d", b->device);
    JV_REQUIRE(b->stored || (!scores_out && !diverse_before_out), "builder_working_lists: scores and marks exist with sorted lists / in reference order only (bl_sorted_lists / bl_ref_order)");
    JV_TRY(use_device(ctx->device));
    return bl_copy_working_lists(ctx, b, ids_out, scores_out, diverse_before_out);
}

const int32_t *jv_hip_builder_neighbors_device(const jv_builder *b, int *row_width)
{
    if (!b) return nullptr;
    if (row_width) *row_width = b->R;
    return b->d_nbrs;
}

}  // extern "C"
