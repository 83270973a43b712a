// bc_params.h — launch parameters of the BQ builder's compaction kernels (bc_body.h / k_bq_compact.hip), shared with the host driver in
// bq_builder.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace jv {

// the rank is an exclusive scan over the present words in three steps; one scan block is this many nodes (words: / 64)
constexpr int BC_SCAN_NODES = 16384;
constexpr int BC_SCAN_WORDS = BC_SCAN_NODES / 64;   // 256: four words per lane in the sums, four waves of 64 words in the write-out
// cells (adjacency entries, BQ words) one wavefront of the two gathers moves: 64 at a time, consecutive
constexpr int BC_WAVE_CELLS = 512;

struct BcParams {
    // ---- rank ----
    const uint64_t *present;   // [ceil(n / 64)] bit i: node i is in the graph; bits at and beyond n count as clear
    int64_t n;                 // rows of the source builder
    uint32_t *block_base;      // [ceil(n / BC_SCAN_NODES)] bc_rank_sums: nodes of the block; bc_rank_scan: nodes before the block
    uint32_t *counters;        // [0] live nodes (bc_rank_scan) [1] stored ids without an image [2] the first new row with one (bc_rows)
    int32_t *old_to_new;       // [n] -1 for a row not in the graph
    int32_t *new_to_old;       // [live] (nullable in the rank)
    // ---- rows ----
    int64_t live;              // rows [0, live) of the destination are gathered
    int32_t R;                 // row width of both adjacencies, <= 64
    const int32_t *src_nbrs;   // [n][R]
    const float *src_nsc;      // [n][R]
    const int32_t *src_db;     // [n]
    int32_t *dst_nbrs;         // [>= live][R]
    float *dst_nsc;            // [>= live][R]
    int32_t *dst_db;           // [>= live]
    // ---- BQ rows ----
    int32_t W;
    const uint64_t *src_rows;  // [n][W]
    uint64_t *dst_rows;        // [>= live][W]
};

constexpr int64_t bc_scan_blocks(int64_t n) { return (n + BC_SCAN_NODES - 1) / BC_SCAN_NODES; }
constexpr int64_t bc_wave_count(int64_t cells) { return (cells + BC_WAVE_CELLS - 1) / BC_WAVE_CELLS; }

}  // namespace jv
