// bd_params.h — launch parameters of the batched robust prune over binary-quantized rows (bd_body.h / k_bq_retain.hip), shared with
// the host driver in bq_build.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace jv {

// the largest alpha taken (jv_hip_retain_diverse's bound): currentAlpha is an f32 stepped by 0.2f, which stops moving at 2^22, so
// the rounds need an end of their own; the host refuses a larger alpha and the body clamps its loop bound to this
constexpr float BD_MAX_ALPHA = 64.0f;
constexpr int BD_MAX_CANDIDATES = 4096;   // the selected set is one 64-bit word per lane: bit t of lane l = candidate 64 t + l

struct BdParams {
    const uint64_t *rows;            // [n][W] BQ rows
    int64_t n;                       // rows a candidate ordinal may name; an ordinal outside scores -INFINITY against everything
    int32_t D, W;
    const int32_t *cand_nodes;       // [P][C] the NodeArrays: ordinals ...
    const float *cand_scores;        // [P][C] ... and scores; entries >= count are ignored
    const int32_t *cand_count;       // [P] or nullptr (= C)
    const int32_t *diverse_before;   // [P] or nullptr (= 0)
    int32_t P, C, maxDegree;
    float alpha;
    int32_t *selected_out;           // [P][maxDegree] selected candidate POSITIONS in ascending order, -1 padded
    int32_t *n_selected_out;         // [P]
    float *short_edges_out;          // [P] or nullptr: nSelected after the alpha = 1.0 round / maxDegree (NaN if the loop never ran)
};

// LDS of one wavefront: [C][W] candidate rows | [W][64] the selected slots' rows, word-major (lane j reads word w of slot j at
// [w * 64 + j]: 64 consecutive 8-byte words) | [C] candidate ordinals | [C] candidate scores
constexpr size_t bd_lds_bytes(int C, int W) { return sizeof(uint64_t) * (size_t)W * ((size_t)C + 64) + 8 * (size_t)C; }

}  // namespace jv
