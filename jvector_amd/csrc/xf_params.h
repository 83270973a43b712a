// xf_params.h — launch parameters of the exact flat search's kernels (k_exact_flat.hip), shared with the host driver in exact_flat.cpp.
// Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace jv {

constexpr int XF_TILE = 128;   // rows and queries of a tile: ED_TN and ED_TQ of ed_body.h (k_exact_flat.hip asserts it)

// One pass of exact_select_kernel over the row tiles tile_offset + b * tile_stride, b = 0 .. tiles - 1, for every query tile.
struct XfParams {
    const float *vecs;         // [n][D]
    const float *queries;      // [Q][D]
    const uint64_t *bits;      // nullptr: every row is accepted.  Mask q starts at bits + q * stride_words; only bits below n are read
    int64_t stride_words;      // 0: one mask for every query
    int64_t n;
    int64_t tiles, tile_stride, tile_offset;
    int D, Q;
    // the sample epilogue: samp[q * S + 128 b + j] = score of row 128 (tile_offset + b * tile_stride) + j, -INFINITY where the row
    // is rejected or lies at or beyond n
    float *samp;
    int64_t S;                 // 128 * tiles
    // the select epilogue: (row, score) joins query q's list when the row is accepted and !(score < tau[q * tau_stride])
    const float *tau;
    int tau_stride;
    int32_t *cand_ids;         // [Q][cap]
    float *cand_scores;        // [Q][cap]
    unsigned int *cand_count;  // [Q], zero on entry; may end above cap (the entries past cap are dropped, the caller checks)
    int cap;
};

// the chunked route's ids: ids[q * count + j] = first + j where query q accepts that row, -1 where it does not
struct XfIdsParams {
    const uint64_t *bits;
    int64_t stride_words;
    int64_t first, count;
    int32_t *ids;
    int Q;
};

// {some list overflowed, sum of the list lengths}: what the host reads back after the select pass
struct XfCheck {
    unsigned long long over, listed;
};

}  // namespace jv
