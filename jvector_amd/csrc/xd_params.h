// xd_params.h — launch parameters of the exact-score builder's deletion kernel (xd_body.h / k_exact_delete.hip), shared with the host
// driver in exact_builder.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

#include "xg_params.h"

struct ihipStream_t;

namespace jv {

struct XdParams {
    const float *rows;          // [n][D] float rows
    const float *vnorm;         // [n] per-row sums of squares (launch_row_sqnorms); COSINE only
    int64_t n;                  // nodes = rows; an id outside [0, n) found in an adjacency row is skipped, never followed
    int32_t D;
    const int32_t *nbrs;        // [n][R] working adjacency, -1 padded
    const float *nsc;           // [n][R] the score each entry was inserted under
    int32_t R;                  // <= 64
    const uint64_t *marked;     // [ceil(n / 64)] bit i: node i is marked deleted
    const int32_t *tasks;       // [P] the affected nodes, every one inside [0, n)
    int32_t P;
    const int32_t *given;       // [P][G] nullptr: the candidates are gathered from the marked neighbours' rows; else the ids to take ...
    const int32_t *given_n;     // [P]   ... and how many (the fallback's draws)
    int32_t G;                  // <= 64
    int32_t L;                  // row width of list / lsc
    int32_t *list;              // [P][L] the merged lists, -1 padded; nullptr: count only
    float *lsc;                 // [P][L]
    int32_t *ln;                // [P] merged length
    int32_t *cn;                // [P] distinct candidates
    int32_t *rn;                // [P] two-hop entries before the duplicates are dropped; nullable
};

// the entries of one node: every entry of every marked neighbour's row, R x R at most, rounded up to the power of two the sorts take
constexpr int xd_capacity(int R)
{
    int c = 64;
    while (c < R * R) c <<= 1;
    return c;
}

// LDS of one wavefront: [score tile][capacity 64-bit keys, the 32-bit id array in their upper half][64 survivor ids | 64 survivor
// scores | 64 dropped positions | 64 dropped candidates].  51 KB at R = 64: three nodes per CU
constexpr size_t xd_lds_bytes(int R) { return sizeof(float) * (size_t)XG_TILE_FLOATS + 8 * (size_t)xd_capacity(R) + 4 * 64 * 4; }

// k_exact_delete.hip (libjvector_hip_xd.so).  vsf: VSF_L2 / VSF_DOT / VSF_COS.  lds_limit: the device's LDS bytes per workgroup;
// blocks: persistent workgroups (one wavefront each) striding over the P nodes.  Returns JV_OK, JV_ERR_INVALID (bad parameters),
// JV_ERR_UNSUPPORTED (LDS) or JV_ERR_HIP; nothing is read back.
int launch_exact_delete_merge(ihipStream_t *s, const XdParams &p, size_t p_bytes, int vsf, size_t lds_limit, int blocks);

}  // namespace jv
