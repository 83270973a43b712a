// xb_params.h — launch parameters of the exact-score robust prune (xb_body.h / k_exact_retain.hip), shared with the host driver in
// exact_build.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

struct ihipStream_t;

namespace jv {

constexpr int XB_TILE_FLOATS = 64 * 68;   // the score phase's LDS tile: 64 rows x (64 columns + 4 of padding)
constexpr int XB_MAX_CANDIDATES = 2048;   // 32 groups of 64 candidates: a lane keeps one bit per group in a 32-bit register
constexpr float XB_MAX_ALPHA = 64.0f;     // the host refuses a larger alpha; the kernel clamps to it (the rounds are a loop on the device)

struct XbParams {
    const float *rows;           // [n][D] float rows
    const float *vnorm;          // [n] per-row sums of squares (launch_row_sqnorms); COSINE only
    int64_t n;                   // rows an ordinal may name
    int32_t D;
    const int32_t *cand_nodes;   // [P][C]
    const float *cand_scores;    // [P][C]
    const int32_t *cand_count;   // [P] or nullptr (C each)
    const int32_t *diverse_before;   // [P] or nullptr (0 each)
    int32_t P, C, maxDegree;
    float alpha;
    int32_t *selected_out;       // [P][maxDegree] ascending positions, -1 padded
    int32_t *n_selected_out;     // [P]
    float *short_edges_out;      // [P] or nullptr
};

constexpr int xb_padded(int C) { return (C + 63) & ~63; }
constexpr int xb_slots(int C, int maxDegree) { return maxDegree < C ? maxDegree : C; }

// LDS bytes of one node's prune: [score tile][pair matrix slots x Cp][ids, scores, norms, own-id stops: 4 x Cp][slot positions 64]
constexpr size_t xb_lds_bytes(int C, int maxDegree)
{
    return sizeof(float) * ((size_t)XB_TILE_FLOATS + (size_t)xb_slots(C, maxDegree) * xb_padded(C) + 4 * (size_t)xb_padded(C) + 64);
}

// largest C whose block fits `limit` bytes of LDS (0: not even 64 candidates)
constexpr int xb_max_candidates(size_t limit, int maxDegree)
{
    const size_t fixed = sizeof(float) * ((size_t)XB_TILE_FLOATS + 64);
    if (limit <= fixed) return 0;
    const size_t cp = (limit - fixed) / (sizeof(float) * ((size_t)maxDegree + 4)) / 64 * 64;
    return (int)(cp < (size_t)XB_MAX_CANDIDATES ? cp : (size_t)XB_MAX_CANDIDATES);
}

// k_exact_retain.hip (libjvector_hip_xb.so).  vsf: VSF_L2 / VSF_DOT / VSF_COS.  lds_limit: the device's LDS bytes per workgroup;
// blocks: persistent workgroups (one wavefront each) striding over the P nodes.  Returns JV_OK, JV_ERR_INVALID (bad parameters),
// JV_ERR_UNSUPPORTED (LDS) or JV_ERR_HIP.
int launch_exact_retain(ihipStream_t *s, const XbParams &p, size_t p_bytes, int vsf, size_t lds_limit, int blocks);

}  // namespace jv
