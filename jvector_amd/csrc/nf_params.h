// nf_params.h — launch parameters of the NVQ flat search's kernel (k_nvq_flat.hip), shared with the host driver in nvq_flat.cpp.
// Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace jv {

constexpr int NF_TILE = 128;   // rows and queries of a tile: ED_TN and ED_TQ of ed_body.h (k_nvq_flat.hip asserts it)

// One pass of nvq_select_kernel over the row tiles tile_offset + b * tile_stride, b = 0 .. tiles - 1, for every query tile.
struct NfParams {
    const uint8_t *bytes;      // [n][ld]: one byte per dimension, ld = D rounded up to 16
    const float *derived;      // [n][subs][4] = {1 / scaledGrowthRate, scaledMidpoint, logisticScale, logisticBias}
    const float *cosnorm;      // [n]; COSINE only
    const float *mean;         // [D]; COSINE only
    const float *queries;      // [Q][D], the A operand: the queries; EUCLIDEAN: qwork = query - globalMean
    const float *qaux;         // [Q]; DOT: dot(query, globalMean); COSINE: |query|
    const uint64_t *bits;      // nullptr: every row is accepted.  Mask q starts at bits + q * stride_words; only bits below n are read
    int64_t stride_words;      // 0: one mask for every query
    int64_t n;
    int64_t tiles, tile_stride, tile_offset;
    int ld, D, subs, Q;
    // the sample epilogue: samp[q * S + 128 b + j] = score of row 128 (tile_offset + b * tile_stride) + j, -INFINITY where the row
    // is rejected or lies at or beyond n; columns at and beyond S are not written
    float *samp;
    int64_t S;                 // 128 (tiles - 1) < S <= 128 tiles
    // the select epilogue: (row, score) joins query q's list when the row is accepted and !(score < tau[q * tau_stride])
    const float *tau;
    int tau_stride;
    int32_t *cand_ids;         // [Q][cap]
    float *cand_scores;        // [Q][cap]
    unsigned int *cand_count;  // [Q], zero on entry; may end above cap (the entries past cap are dropped, the caller checks)
    int cap;
};

}  // namespace jv
