// fa_params.h — launch parameters of the filtered flat search's kernels (fa_body.h / k_flat_accept.hip), shared with the host driver in
// flat_accept.cpp and with the lane emulator of the CPU tests.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace jv {

// the mask -> list compaction is an exclusive scan over the accept words in three steps; one scan block is this many rows (words: / 64)
constexpr int FA_SCAN_ROWS = 16384;
constexpr int FA_SCAN_WORDS = FA_SCAN_ROWS / 64;   // 256: four words per lane in the sums, four waves of 64 words in the write-out
constexpr int FA_SEG_ROWS = 64 * 64;               // rows one wavefront of the write-out covers
constexpr int FA_CLUSTERS = 256;                   // ProductQuantization.DEFAULT_CLUSTERS: entries per subspace of an ADC table
constexpr int FA_P = 4;                            // queries whose tables share one LDS entry in the list ADC kernel
constexpr int FA_THREADS = 1024;                   // its workgroup

// 16-byte vectors the bodies move whole (ds_read_b128 / global_load_dwordx4 on the device, plain structs on the emulator)
struct alignas(16) FaF4 {
    float x, y, z, w;
};
struct alignas(16) FaU4 {
    uint32_t x, y, z, w;
};

struct FaScanParams {
    const uint64_t *bits;      // mask m starts at bits + m * stride_words; bits at and beyond n and words past ceil(n / 64) are never used
    int64_t stride_words;      // 0: one mask, shared by every list row
    int64_t n;                 // rows of the code set
    int64_t blocks;            // ceil(n / FA_SCAN_ROWS)
    uint32_t *block_base;      // [masks][blocks] fa_sums: accepted rows of the block; fa_scan: accepted rows before the block
    uint32_t *totals;          // [masks] accepted rows (fa_scan)
    // ---- write-out ----
    int first_mask;            // list row y is written from mask first_mask + y (mask 0 when stride_words == 0)
    int32_t *lists;            // [rows][L] ascending accepted ordinals, then -1
    int64_t L;
};

struct FaAdcParams {
    const float *luts;         // [Q][M * 256]
    const float *bmag;         // [Q] (cosine)
    const uint8_t *codes;      // [n][M], 16-byte aligned, M % 16 == 0
    const float *norms;        // [n] (cosine)
    const int32_t *list;       // [count] ordinals; an entry outside [0, n) scores -inf
    float *out;                // [Q][L]: column i is list position i
    int64_t n, count, L;
    int Q, M;
};

struct FaMapParams {
    const int32_t *list;       // [count]
    int32_t *ids;              // [cells] in: list positions or -1; out: ordinals or -1
    int64_t cells, count;
};

constexpr int64_t fa_scan_blocks(int64_t n) { return (n + FA_SCAN_ROWS - 1) / FA_SCAN_ROWS; }
constexpr int64_t fa_segments(int64_t n) { return (n + FA_SEG_ROWS - 1) / FA_SEG_ROWS; }
// LDS of the list ADC kernel: one slice of 16 SLCH subspaces, four queries per entry
constexpr size_t fa_adc_lds_bytes(int slch) { return (size_t)16 * slch * FA_CLUSTERS * sizeof(FaF4); }

}  // namespace jv
