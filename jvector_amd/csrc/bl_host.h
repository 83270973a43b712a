// bl_host.h — the score-agnostic host steps of the batched builders (builder.cpp over PQ codes, bq_builder.cpp over BQ rows): what
// validates a batch, reads the one counter a batch leaves behind, and drives the reference-order back-link merge.  None of it looks
// at what a score means; the one step that does — the re-prune of the lists that overflowed — is handed in by the caller.  The
// templates are written over the field names the two builder structs share (n, R, hard_max, the d_* buffers, backlink_s).
#pragma once

#include <algorithm>
#include <chrono>
#include <vector>

#include "bl_body.h"
#include "jv_internal.h"

namespace jv {

inline double bl_now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

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

// the unsigned counter at d_ctr, after everything queued on the context's stream
inline int bl_read_counter(jv_ctx *ctx, const void *d_ctr, unsigned int *out)
{
    JV_TRY(ctx->h_out.reserve(64));
    JV_HIP_CHECK(hipMemcpyAsync(ctx->h_out.ptr, d_ctr, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *out = *(const unsigned int *)ctx->h_out.ptr;
    return JV_OK;
}

// reference order: the E back edges (keys / src / scores in d_keys / d_src / d_esc) -> Neighbors.insert per target, in batch order;
// the lists past the hard maximum go to reprune(over_tgt, over_list, over_sc, over_n, over_db, P, L)
template <class Builder, class Reprune>
int bl_link_back_edges_ro(jv_ctx *ctx, Builder *b, long long E, int dedupe_ids, Reprune reprune)
{
    const int R = b->R;
    const double t0 = bl_now_s();
    size_t tmp_bytes = 0;
    JV_TRY(launch_bl_sort_edges(ctx->stream, nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, E, 64));
    JV_TRY(b->d_sort_tmp.reserve(tmp_bytes + 256));
    JV_TRY(launch_bl_sort_edges(ctx->stream, b->d_sort_tmp.ptr, &tmp_bytes, (const unsigned long long *)b->d_keys.ptr,
                                (unsigned long long *)b->d_keys2.ptr, (const int32_t *)b->d_src.ptr, (int32_t *)b->d_src2.ptr, E, 64));
    const int Knew = 2 * R, L = R + Knew;
    static_assert(BL_RO_MAX_LIST >= 3 * 64, "the merge step's working list holds R + 2 R entries, R <= 64");
    const unsigned int over_cap = (unsigned int)std::min<long long>(E, b->n);   // at most one overflow per distinct target
    JV_TRY(b->d_over_tgt.reserve(sizeof(int32_t) * (size_t)over_cap));
    JV_TRY(b->d_over_db.reserve(sizeof(int32_t) * (size_t)over_cap));
    JV_TRY(b->d_over_n.reserve(sizeof(int32_t) * (size_t)over_cap));
    JV_TRY(b->d_over_list.reserve(sizeof(int32_t) * (size_t)over_cap * L));
    JV_TRY(b->d_over_sc.reserve(sizeof(float) * (size_t)over_cap * L));
    JV_HIP_CHECK(hipMemsetAsync(b->d_ctr.ptr, 0, sizeof(unsigned int), ctx->stream));
    BlRoMergeParams mp{};
    mp.keys = (const unsigned long long *)b->d_keys2.ptr;
    mp.src = (const int32_t *)b->d_src.ptr;
    mp.esc = (const float *)b->d_esc.ptr;
    mp.E = E;
    mp.R = R;
    mp.hard_max = b->hard_max;
    mp.Knew = Knew;
    mp.dedupe_ids = dedupe_ids;
    mp.nbrs = b->d_nbrs;
    mp.nsc = b->d_nsc;
    mp.db = b->d_db;
    mp.over_tgt = (int32_t *)b->d_over_tgt.ptr;
    mp.over_list = (int32_t *)b->d_over_list.ptr;
    mp.over_sc = (float *)b->d_over_sc.ptr;
    mp.over_db = (int32_t *)b->d_over_db.ptr;
    mp.over_n = (int32_t *)b->d_over_n.ptr;
    mp.over_count = (unsigned int *)b->d_ctr.ptr;
    mp.over_cap = over_cap;
    JV_TRY(launch_bl_ro_backlink_merge(ctx->stream, mp));
    unsigned int n_over = 0;
    JV_TRY(bl_read_counter(ctx, b->d_ctr.ptr, &n_over));
    n_over = std::min(n_over, over_cap);
    JV_TRY(reprune(mp.over_tgt, mp.over_list, mp.over_sc, mp.over_n, mp.over_db, (int)n_over, L));
    JV_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    b->backlink_s += bl_now_s() - t0;
    return JV_OK;
}

}  // namespace jv
