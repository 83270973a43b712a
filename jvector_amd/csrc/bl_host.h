// bl_host.h — the REFERENCE ORDER list discipline of the batched builders, once: the state builder.cpp (PQ codes) and bq_builder.cpp
// (BQ rows) share, and every host step of a batch that does not look at what a score means — staging and validating a batch, the
// insertDiverse of a searched batch, improveConnections' merge, the back-link merge, enforceDegree, the copies out, and the frame of a
// layered build.  The one thing that differs between the builders in these steps is the robust prune, handed in as a callable:
//   retain(list, scores, counts, before, P, L, sel, nsel) -> status     P lists of row width L, retainDiverse(list, before) -> sel / nsel
// The candidate search, the classic (re-scoring) path and the sorted-lists pre-steps stay in builder.cpp; capacity checks, the present
// bits, deletion and compaction stay in bq_builder.cpp.  Header-only; names nothing of either quantizer.
#pragma once

#include <algorithm>
#include <chrono>
#include <vector>

#include "bl_body.h"
#include "gs_params.h"
#include "jv_internal.h"

namespace jv {

inline double bl_now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// what jv_builder and jv_bq_builder both are: the working adjacency and the scratch of a batch
struct BlBuilderState {
    int device = 0;
    int64_t n = 0;
    int Rf = 32, R = 40, beam = 100;
    float alpha = 1.2f;
    int hard_max = 0;                // (int) (neighborOverflow x maxDegree), capped at R: a list longer than this is pruned
    int32_t *d_nbrs = nullptr;       // [n][R]
    float *d_nsc = nullptr;          // [n][R] the score each entry was inserted under
    int32_t *d_db = nullptr;         // [n] diverseBefore
    jv_graph *graph = nullptr;       // level 0 = d_nbrs, read in place by the traversal
    int64_t inserted = 0;            // nodes in the graph: seeded or inserted, not removed (the search cannot return more than that)
    int32_t entry = -1;
    Buffer d_nodes, d_cand, d_csc, d_count, d_sel, d_nsel, d_keys, d_keys2, d_src, d_src2, d_esc, d_sort_tmp, d_over_tgt, d_over_list, d_over_sc,
        d_over_db, d_over_n, d_imp_list, d_ctr;
    double search_s = 0, prune_s = 0, backlink_s = 0;
    int64_t reprunes = 0, batches = 0, visited = 0, expanded = 0;   // (visited / expanded: SearchResult counters summed over the searches)
    std::vector<int64_t> h_stats;
    ~BlBuilderState()
    {
        for (Buffer *b : {&d_nodes, &d_cand, &d_csc, &d_count, &d_sel, &d_nsel, &d_keys, &d_keys2, &d_src, &d_src2, &d_esc, &d_sort_tmp, &d_over_tgt,
                          &d_over_list, &d_over_sc, &d_over_db, &d_over_n, &d_imp_list, &d_ctr})
            b->release();
    }
};

// ---- parameters ----

inline int bl_check_parameters(const char *who, int max_degree, int beam_width, float alpha, float overflow)
{
    JV_REQUIRE(max_degree >= 2 && max_degree <= 64, "%s: maxDegree %d outside 2..64", who, max_degree);
    JV_REQUIRE(beam_width >= 1 && beam_width <= 4096, "%s: beamWidth %d outside 1..4096", who, beam_width);
    JV_REQUIRE(alpha == alpha && alpha >= 1.0f && alpha <= 64.0f, "%s: alpha must lie in [1, 64]", who);
    JV_REQUIRE(overflow == overflow && overflow >= 1.0f && overflow <= 8.0f, "%s: neighborOverflow must lie in [1, 8]", who);
    return JV_OK;
}

// the working row width (ConcurrentNeighborMap.java:298-322)
inline int bl_working_width(int max_degree, float overflow) { return std::max(max_degree, std::min(64, (int)(max_degree * overflow))); }

inline void bl_set_parameters(BlBuilderState *s, int max_degree, int beam_width, float alpha, float overflow)
{
    s->Rf = max_degree;
    s->R = bl_working_width(max_degree, overflow);
    s->beam = beam_width;
    s->alpha = alpha;
    s->hard_max = std::min(s->R, (int)(overflow * (float)max_degree));   // Neighbors.insert :270
}

// ---- a batch ----

// The caller's ids index the adjacency rows and the code / vector / BQ rows unguarded further down, and two inserts of one id would
// race on one row: an id outside [0, limit), or listed twice, is refused.  A batch is at most a few hundred KB: a host copy and a
// sort cost nothing next to the batch's searches.
inline int bl_check_batch(jv_ctx *ctx, const int32_t *nodes, int B, int Rf, long long limit, const char *what)
{
    JV_REQUIRE((long long)B * Rf <= 0x7fffffffll, "%s: %d nodes x %d working slots exceed the edge sorter's 32-bit count; split the batch", what, B, Rf);
    std::vector<int32_t> h((size_t)B);
    JV_HIP_CHECK(hipMemcpyAsync(h.data(), nodes, sizeof(int32_t) * (size_t)B, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < B; ++i)
        JV_REQUIRE(h[(size_t)i] >= 0 && h[(size_t)i] < limit, "%s: node id %d (position %d) outside [0, %lld)", what, h[(size_t)i], i, limit);
    std::sort(h.begin(), h.end());
    for (int i = 1; i < B; ++i) JV_REQUIRE(h[(size_t)i] != h[(size_t)i - 1], "%s: node id %d appears twice in the batch", what, h[(size_t)i]);
    return JV_OK;
}

// the batch's ids -> d_nodes
inline int bl_stage_batch(jv_ctx *ctx, BlBuilderState *s, const int32_t *nodes, int B)
{
    JV_TRY(s->d_nodes.reserve(sizeof(int32_t) * (size_t)B));
    JV_HIP_CHECK(hipMemcpyAsync(s->d_nodes.ptr, nodes, sizeof(int32_t) * (size_t)B, hipMemcpyDefault, ctx->stream));
    if (!is_device_ptr(nodes)) JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the caller may reuse its buffer
    return JV_OK;
}

// the unsigned counter at d_ctr, after everything queued on the context's stream
inline int bl_read_counter(jv_ctx *ctx, const void *d_ctr, unsigned int *out)
{
    JV_TRY(ctx->h_out.reserve(64));
    JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, d_ctr, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *out = *(const unsigned int *)ctx->h_out.ptr;
    return JV_OK;
}

// ---- back edges ----

// room for E back edges; their scores only where the lists store scores
inline int bl_reserve_edges(BlBuilderState *s, long long E, bool with_scores)
{
    JV_TRY(s->d_keys.reserve(sizeof(unsigned long long) * (size_t)E));
    JV_TRY(s->d_keys2.reserve(sizeof(unsigned long long) * (size_t)E));
    JV_TRY(s->d_src.reserve(sizeof(int32_t) * (size_t)E));
    JV_TRY(s->d_src2.reserve(sizeof(int32_t) * (size_t)E));
    if (with_scores) JV_TRY(s->d_esc.reserve(sizeof(float) * (size_t)E));
    return JV_OK;
}

// the E back edges of d_keys / d_src sorted by (target, edge index) into d_keys2 / d_src2
inline int bl_sort_edges(jv_ctx *ctx, BlBuilderState *s, long long E)
{
    size_t tmp_bytes = 0;
    JV_TRY(launch_bl_sort_edges(ctx->stream, nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, E, 64));
    JV_TRY(s->d_sort_tmp.reserve(tmp_bytes + 256));
    return launch_bl_sort_edges(ctx->stream, s->d_sort_tmp.ptr, &tmp_bytes, (const unsigned long long *)s->d_keys.ptr,
                                (unsigned long long *)s->d_keys2.ptr, (const int32_t *)s->d_src.ptr, (int32_t *)s->d_src2.ptr, E, 64);
}

// lists d_list / d_lsc [P][L] (already in NodeArray order, with the scores their entries were inserted under) of the targets d_tgt:
// retainDiverse(list, diverseBefore), the selection replaces the row, diverseBefore = size
template <class Retain>
int bl_reprune_lists_ro(jv_ctx *ctx, BlBuilderState *s, const int32_t *d_tgt, const int32_t *d_list, const float *d_lsc, const int32_t *d_n,
                        const int32_t *d_before, int P, int L, Retain retain)
{
    if (P == 0) return JV_OK;
    JV_TRY(s->d_sel.reserve(sizeof(int32_t) * (size_t)P * s->Rf));
    JV_TRY(s->d_nsel.reserve(sizeof(int32_t) * (size_t)P));
    JV_TRY(retain(d_list, d_lsc, d_n, d_before, P, L, (int32_t *)s->d_sel.ptr, (int32_t *)s->d_nsel.ptr));
    BlRoRowsParams rp{};
    rp.tgt = d_tgt;
    rp.lst = d_list;
    rp.lsc = d_lsc;
    rp.sel = (const int32_t *)s->d_sel.ptr;
    rp.P = P;
    rp.L = L;
    rp.Rf = s->Rf;
    rp.R = s->R;
    rp.nbrs = s->d_nbrs;
    rp.nsc = s->d_nsc;
    rp.db = s->d_db;
    JV_TRY(launch_bl_ro_rewrite_rows(ctx->stream, rp));
    s->reprunes += P;
    return JV_OK;
}

// the E back edges (keys / src / scores in d_keys / d_src / d_esc) -> Neighbors.insert per target, in batch order; the lists past the
// hard maximum are re-pruned, behind their diverseBefore mark if use_diverse_before
template <class Retain>
int bl_link_back_edges_ro(jv_ctx *ctx, BlBuilderState *s, long long E, Retain retain, bool use_diverse_before)
{
    const int R = s->R;
    const double t0 = bl_now_s();
    JV_TRY(bl_sort_edges(ctx, s, E));
    const int Knew = 2 * R, L = R + Knew;
    static_assert(BL_RO_MAX_LIST >= 3 * 64, "the merge step's working list holds R + 2 R entries, R <= 64");
    const unsigned int over_cap = (unsigned int)std::min<long long>(E, s->n);   // at most one overflow per distinct target
    JV_TRY(s->d_over_tgt.reserve(sizeof(int32_t) * (size_t)over_cap));
    JV_TRY(s->d_over_db.reserve(sizeof(int32_t) * (size_t)over_cap));
    JV_TRY(s->d_over_n.reserve(sizeof(int32_t) * (size_t)over_cap));
    JV_TRY(s->d_over_list.reserve(sizeof(int32_t) * (size_t)over_cap * L));
    JV_TRY(s->d_over_sc.reserve(sizeof(float) * (size_t)over_cap * L));
    JV_HIP_CHECK(hipMemsetAsync(s->d_ctr.ptr, 0, sizeof(unsigned int), ctx->stream));
    BlRoMergeParams mp{};
    mp.keys = (const unsigned long long *)s->d_keys2.ptr;
    mp.src = (const int32_t *)s->d_src.ptr;
    mp.esc = (const float *)s->d_esc.ptr;
    mp.E = E;
    mp.R = R;
    mp.hard_max = s->hard_max;
    mp.Knew = Knew;
    // a fresh node is in nobody's list, so this changes nothing for an insert; an improve pass, and a RE-insertion of a node the graph
    // already holds, rely on it not to list a node twice under two scores
    mp.dedupe_ids = 1;
    mp.nbrs = s->d_nbrs;
    mp.nsc = s->d_nsc;
    mp.db = s->d_db;
    mp.over_tgt = (int32_t *)s->d_over_tgt.ptr;
    mp.over_list = (int32_t *)s->d_over_list.ptr;
    mp.over_sc = (float *)s->d_over_sc.ptr;
    mp.over_db = (int32_t *)s->d_over_db.ptr;
    mp.over_n = (int32_t *)s->d_over_n.ptr;
    mp.over_count = (unsigned int *)s->d_ctr.ptr;
    mp.over_cap = over_cap;
    JV_TRY(launch_bl_ro_backlink_merge(ctx->stream, mp));
    unsigned int n_over = 0;
    JV_TRY(bl_read_counter(ctx, s->d_ctr.ptr, &n_over));
    n_over = std::min(n_over, over_cap);
    JV_TRY(bl_reprune_lists_ro(ctx, s, mp.over_tgt, mp.over_list, mp.over_sc, mp.over_n, use_diverse_before ? mp.over_db : nullptr, (int)n_over, L, retain));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    s->backlink_s += bl_now_s() - t0;
    return JV_OK;
}

// ---- insert and improve ----

// addGraphNode for the B nodes of d_nodes, whose candidates (best first) and scores the search left in d_cand / d_csc [B][k]: robust
// prune, insertDiverse on the new nodes' empty lists, back edges emitted with their scores, then backlink -> Neighbors.insert
template <class Retain>
int bl_ro_insert(jv_ctx *ctx, BlBuilderState *s, int B, int k, Retain retain, bool use_diverse_before)
{
    const int32_t *d_cand = (const int32_t *)s->d_cand.ptr;
    const float *d_csc = (const float *)s->d_csc.ptr;
    const double t0 = bl_now_s();
    JV_TRY(s->d_count.reserve(sizeof(int32_t) * (size_t)B));
    JV_TRY(s->d_sel.reserve(sizeof(int32_t) * (size_t)B * s->Rf));
    JV_TRY(s->d_nsel.reserve(sizeof(int32_t) * (size_t)B));
    JV_TRY(launch_bl_count_valid(ctx->stream, d_cand, k, (int32_t *)s->d_count.ptr, B));
    JV_TRY(retain(d_cand, d_csc, (const int32_t *)s->d_count.ptr, nullptr, B, k, (int32_t *)s->d_sel.ptr, (int32_t *)s->d_nsel.ptr));
    const long long E = (long long)B * s->Rf;
    JV_TRY(bl_reserve_edges(s, E, true));
    BlRoApplyParams rp{};
    rp.nodes = (const int32_t *)s->d_nodes.ptr;
    rp.cand = d_cand;
    rp.cand_sc = d_csc;
    rp.sel = (const int32_t *)s->d_sel.ptr;
    rp.B = B;
    rp.C = k;
    rp.Rf = s->Rf;
    rp.R = s->R;
    rp.nbrs = s->d_nbrs;
    rp.nsc = s->d_nsc;
    rp.db = s->d_db;
    rp.edge_keys = (unsigned long long *)s->d_keys.ptr;
    rp.edge_src = (int32_t *)s->d_src.ptr;
    rp.edge_sc = (float *)s->d_esc.ptr;
    JV_TRY(launch_bl_ro_apply_selection(ctx->stream, rp));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    s->prune_s += bl_now_s() - t0;
    JV_TRY(bl_link_back_edges_ro(ctx, s, E, retain, use_diverse_before));
    s->inserted += B;
    s->batches += 1;
    return JV_OK;
}

// improveConnections for the B nodes of d_nodes, which are IN the graph: insertDiverse(merge(list, candidates)) under the stored scores
// and the candidates' (cand_ids / cand_sc [B][k]: the search's, or the caller's re-scoring of them), the row rewritten, every member of
// the new row linked back.  t0: when the caller's prune phase began.
template <class Retain>
int bl_ro_improve(jv_ctx *ctx, BlBuilderState *s, int B, int k, const int32_t *cand_ids, const float *cand_sc, int skip_empty, double t0,
                  Retain retain, bool use_diverse_before)
{
    const int32_t *d_nodes = (const int32_t *)s->d_nodes.ptr;
    const int L = s->R + k;
    JV_TRY(s->d_imp_list.reserve(sizeof(int32_t) * (size_t)B * L));
    JV_TRY(s->d_over_sc.reserve(sizeof(float) * (size_t)B * L));
    JV_TRY(s->d_over_n.reserve(sizeof(int32_t) * (size_t)B));
    BlRoImproveParams ip{};
    ip.nodes = d_nodes;
    ip.cand = cand_ids;
    ip.cand_sc = cand_sc;
    ip.skip_empty = skip_empty;
    ip.B = B;
    ip.C = k;
    ip.R = s->R;
    ip.nbrs = s->d_nbrs;
    ip.nsc = s->d_nsc;
    ip.list = (int32_t *)s->d_imp_list.ptr;
    ip.lsc = (float *)s->d_over_sc.ptr;
    ip.ln = (int32_t *)s->d_over_n.ptr;
    JV_TRY(launch_bl_ro_improve_list(ctx->stream, ip));
    JV_TRY(bl_reprune_lists_ro(ctx, s, d_nodes, ip.list, ip.lsc, ip.ln, nullptr, B, L, retain));
    const long long E = (long long)B * s->Rf;
    JV_TRY(bl_reserve_edges(s, E, true));
    BlRoRowEdgesParams ep{};
    ep.nodes = d_nodes;
    ep.B = B;
    ep.Rf = s->Rf;
    ep.R = s->R;
    ep.nbrs = s->d_nbrs;
    ep.nsc = s->d_nsc;
    ep.edge_keys = (unsigned long long *)s->d_keys.ptr;
    ep.edge_src = (int32_t *)s->d_src.ptr;
    ep.edge_sc = (float *)s->d_esc.ptr;
    JV_TRY(launch_bl_ro_row_edges(ctx->stream, ep));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    s->prune_s += bl_now_s() - t0;
    JV_TRY(bl_link_back_edges_ro(ctx, s, E, retain, use_diverse_before));
    s->batches += 1;
    return JV_OK;
}

// ---- finish ----

// the rows still above maxDegree -> d_over_tgt, their number -> *n_over
inline int bl_list_over_degree(jv_ctx *ctx, BlBuilderState *s, unsigned int *n_over)
{
    JV_TRY(s->d_over_tgt.reserve(sizeof(int32_t) * (size_t)s->n));
    JV_HIP_CHECK(hipMemsetAsync(s->d_ctr.ptr, 0, sizeof(unsigned int), ctx->stream));
    BlOverParams op{};
    op.nbrs = s->d_nbrs;
    op.N = s->n;
    op.R = s->R;
    op.Rf = s->Rf;
    op.over_tgt = (int32_t *)s->d_over_tgt.ptr;
    op.over_count = (unsigned int *)s->d_ctr.ptr;
    op.over_cap = (unsigned int)s->n;
    JV_TRY(launch_bl_list_over_degree(ctx->stream, op));
    return bl_read_counter(ctx, s->d_ctr.ptr, n_over);
}

constexpr int kBlEnforcePiece = 1 << 20;   // enforceDegree re-prunes this many rows at a time

// GraphIndexBuilder.cleanup -> enforceDegree: retainDiverse(copy, diverseBefore) over the stored scores (ConcurrentNeighborMap.java:190-200)
template <class Retain>
int bl_ro_enforce_degree(jv_ctx *ctx, BlBuilderState *s, Retain retain, bool use_diverse_before)
{
    unsigned int n_over = 0;
    JV_TRY(bl_list_over_degree(ctx, s, &n_over));
    const size_t pc = (size_t)std::min<unsigned int>(n_over, kBlEnforcePiece);
    JV_TRY(s->d_over_list.reserve(sizeof(int32_t) * pc * s->R));
    JV_TRY(s->d_over_sc.reserve(sizeof(float) * pc * s->R));
    JV_TRY(s->d_over_db.reserve(sizeof(int32_t) * pc));
    JV_TRY(s->d_over_n.reserve(sizeof(int32_t) * pc));
    for (unsigned int at = 0; at < n_over; at += kBlEnforcePiece) {
        const int P = (int)std::min<unsigned int>(kBlEnforcePiece, n_over - at);
        BlRoCopyParams cp{};
        cp.tgt = (const int32_t *)s->d_over_tgt.ptr + at;
        cp.P = P;
        cp.R = s->R;
        cp.nbrs = s->d_nbrs;
        cp.nsc = s->d_nsc;
        cp.db = s->d_db;
        cp.lst = (int32_t *)s->d_over_list.ptr;
        cp.lsc = (float *)s->d_over_sc.ptr;
        cp.ldb = (int32_t *)s->d_over_db.ptr;
        cp.ln = (int32_t *)s->d_over_n.ptr;
        JV_TRY(launch_bl_ro_copy_rows(ctx->stream, cp));
        JV_TRY(bl_reprune_lists_ro(ctx, s, cp.tgt, cp.lst, cp.lsc, cp.ln, use_diverse_before ? cp.ldb : nullptr, P, s->R, retain));
    }
    return JV_OK;
}

// the first maxDegree cells of every working row -> neighbors_out [n][maxDegree] (host or device memory; NULL: nothing)
inline int bl_copy_rows_out(jv_ctx *ctx, const BlBuilderState *s, int32_t *neighbors_out)
{
    if (!neighbors_out) return JV_OK;
    OutStage os;
    JV_TRY(stage_out_begin(ctx, neighbors_out, sizeof(int32_t) * (size_t)s->n * s->Rf, ctx->d_out, &os));
    JV_TRY(launch_bl_strided_copy(ctx->stream, s->d_nbrs, s->R, s->Rf, s->n, (int32_t *)os.dev));
    return stage_out_end(ctx, os);
}

// ---- reading a builder ----

inline void bl_fill_stats(const BlBuilderState *s, double *seconds3, int64_t *counts5)
{
    if (seconds3) {
        seconds3[0] = s->search_s;
        seconds3[1] = s->prune_s;
        seconds3[2] = s->backlink_s;
    }
    if (counts5) {
        counts5[0] = s->batches;
        counts5[1] = s->reprunes;
        counts5[2] = s->inserted;
        counts5[3] = s->visited;
        counts5[4] = s->expanded;
    }
}

inline int bl_copy_working_lists(jv_ctx *ctx, const BlBuilderState *s, int32_t *ids_out, float *scores_out, int32_t *diverse_before_out)
{
    const size_t cells = (size_t)s->n * s->R;
    if (ids_out) JV_HIP_CHECK(hipMemcpyAsync(ids_out, s->d_nbrs, sizeof(int32_t) * cells, hipMemcpyDefault, ctx->stream));
    if (scores_out) JV_HIP_CHECK(hipMemcpyAsync(scores_out, s->d_nsc, sizeof(float) * cells, hipMemcpyDefault, ctx->stream));
    if (diverse_before_out) JV_HIP_CHECK(hipMemcpyAsync(diverse_before_out, s->d_db, sizeof(int32_t) * (size_t)s->n, hipMemcpyDefault, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return JV_OK;
}

// ---- the layered build ----

// the four entry points of a builder that a level's schedule calls
template <class Builder>
struct BlLevelOps {
    int (*seed)(jv_ctx *, Builder *, int32_t);
    int (*insert_batch)(jv_ctx *, Builder *, const int32_t *, int);
    int (*improve_batch)(jv_ctx *, Builder *, const int32_t *, int);
    int (*finish)(jv_ctx *, Builder *, int32_t *);
};

// one level over the fresh builder b — n nodes with LOCAL ids 0..n-1: inserts in a seeded order, improve passes, enforceDegree; rows to
// out_rows (host or device memory, n x maxDegree), the builder's timers and counters added to acc.  The insert phase runs under
// insert_alpha and the improve passes under improve_beam (the PQ build's experiment knobs; otherwise the builder's own alpha / beam).
template <class Builder>
int bl_build_one_level(jv_ctx *ctx, const BlLevelOps<Builder> &ops, Builder *b, int64_t n, int max_batch, int improve_passes, uint64_t seed,
                       float insert_alpha, int improve_beam, int32_t *out_rows, jv_layered *acc)
{
    const std::vector<int32_t> perm = seeded_permutation(n, seed);
    JV_TRY(ops.seed(ctx, b, perm[0]));
    const float alpha = b->alpha;
    b->alpha = insert_alpha;
    int64_t lo = 1;
    while (lo < n) {   // prefix doubling: a batch never exceeds what the graph already holds
        const int64_t hi = std::min<int64_t>(n, lo + std::min<int64_t>(max_batch, lo));
        JV_TRY(ops.insert_batch(ctx, b, perm.data() + lo, (int)(hi - lo)));
        lo = hi;
    }
    b->alpha = alpha;
    b->beam = improve_beam;
    for (int pass = 0; pass < improve_passes && n >= 2; ++pass)
        for (int64_t at = 0; at < n; at += max_batch)
            JV_TRY(ops.improve_batch(ctx, b, perm.data() + at, (int)std::min<int64_t>(max_batch, n - at)));
    JV_TRY(ops.finish(ctx, b, out_rows));
    double sec[3];
    int64_t cnt[5];
    bl_fill_stats(b, sec, cnt);
    for (int i = 0; i < 3; ++i) acc->seconds[i] += sec[i];
    for (int i = 0; i < 5; ++i) acc->counts[i] += cnt[i];
    return JV_OK;
}

// GraphIndexBuilder with addHierarchy over n nodes: getRandomGraphLevel per node (seeded; levels with fewer than min_top nodes fold into
// the one below), a node present on every level up to its own, each level a graph of its own:
//   build_level(ids, seed, out_rows, acc)   ids == nullptr: level 0 over every node, rows into device memory; else an upper level over the
//                                           members *ids (ascending) under LOCAL ids, rows into host memory — mapped back to global ids here
//   pick_entry(ids, &entry)                 the entry node among the top level's members (a flat graph is entered where its construction
//                                           started)
template <class BuildLevel, class PickEntry>
int bl_build_layered(jv_ctx *ctx, const char *who, int64_t n, int max_degree, uint64_t seed, int min_top, BuildLevel build_level, PickEntry pick_entry,
                     jv_layered **out)
{
    const double t_start = bl_now_s();
    jv_layered *L = new jv_layered();
    L->device = ctx->device;
    L->max_degree = max_degree;
    L->n = n;
    auto run = [&]() -> int {
        std::vector<int8_t> lvl;
        const int top = layered_draw_levels(n, max_degree, seed, min_top, GS_MAX_LEVELS, lvl);
        L->nodes.resize((size_t)top + 1);
        L->nbrs.resize((size_t)top + 1);
        L->level_counts.assign((size_t)top + 1, 0);
        L->level_counts[0] = n;
        for (int l = 1; l <= top; ++l) {
            for (int64_t i = 0; i < n; ++i)
                if (lvl[(size_t)i] >= l) L->nodes[(size_t)l].push_back((int32_t)i);
            L->level_counts[(size_t)l] = (int64_t)L->nodes[(size_t)l].size();
        }
        if (hipMalloc((void **)&L->d_level0, sizeof(int32_t) * (size_t)n * max_degree) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: cannot allocate the %lld x %d level-0 rows", who, (long long)n, max_degree);
            return JV_ERR_OOM;
        }
        JV_TRY(build_level((const std::vector<int32_t> *)nullptr, seed, L->d_level0, L));
        for (int l = 1; l <= top; ++l) {
            const std::vector<int32_t> &ids = L->nodes[(size_t)l];
            std::vector<int32_t> &rows = L->nbrs[(size_t)l];
            rows.assign(ids.size() * (size_t)max_degree, -1);
            JV_TRY(build_level(&ids, seed + (uint64_t)l, rows.data(), L));
            for (int32_t &x : rows)
                if (x >= 0) x = ids[(size_t)x];
        }
        L->entry_level = top;
        if (top == 0) L->entry = seeded_permutation(n, seed)[0];
        else JV_TRY(pick_entry(L->nodes[(size_t)top], &L->entry));
        return JV_OK;
    };
    const int rc = run();
    if (rc != JV_OK) {
        jv_hip_layered_destroy(L);
        return rc;
    }
    L->total_s = bl_now_s() - t_start;
    *out = L;
    return JV_OK;
}

}  // namespace jv
