// bx_params.h — launch parameters of the BQ builder's deletion kernels (bx_body.h / k_bq_delete.hip), shared with the host driver in
// bq_builder.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace jv {

struct BxParams {
    const uint64_t *rows;       // [n][W] BQ rows
    int64_t n;                  // nodes = rows; an id outside [0, n) found in an adjacency row is skipped, never followed
    int32_t D, W;
    const int32_t *nbrs;        // [n][R] working adjacency, -1 padded
    const float *nsc;           // [n][R] the score each entry was inserted under
    int32_t R;                  // <= 64
    const uint64_t *present;    // [ceil(n / 64)] bit i: node i is in the graph
    const uint64_t *marked;     // [ceil(n / 64)] bit i: node i is marked deleted
    uint64_t *affected;         // [ceil(n / 64)] bit i: node i is live and has a marked neighbour (bx_affected_word writes, bx_compact reads)
    int32_t *tasks;             // [P] the affected nodes, ascending (bx_compact writes, bx_node reads)
    uint32_t *task_count;       // [1] (bx_compact)
    int32_t P;
    const int32_t *given;       // [P][G] nullptr: the candidates are gathered from the marked neighbours' rows; else the ids to take ...
    const int32_t *given_n;     // [P]   ... and how many (the fallback's draws: distinct, live, in the graph, not the node itself)
    int32_t G;                  // <= 64
    int32_t L;                  // row width of list / lsc
    int32_t *list;              // [P][L] the merged lists, -1 padded; nullptr: count only
    float *lsc;                 // [P][L]
    int32_t *ln;                // [P] merged length
    int32_t *cn;                // [P] distinct candidates
};

// the key array of one node: every entry of every marked neighbour's row, R x R at most, rounded up to the power of two the sort takes
constexpr int bx_key_capacity(int R)
{
    int c = 64;
    while (c < R * R) c <<= 1;
    return c;
}

// LDS of one wavefront: [capacity] keys | [64] survivor ids | [64] survivor scores | [64] dropped positions | [64] dropped candidates
// | generic row widths only: the node's own W words
constexpr size_t bx_lds_bytes(int R, int W_generic) { return 8 * (size_t)bx_key_capacity(R) + 4 * 64 * 4 + 8 * (size_t)W_generic; }

}  // namespace jv
