// fm_params.h — launch parameters of the dense route of the filtered flat search (k_flat_mask.hip), shared with the host driver in
// flat_accept.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

namespace jv {

constexpr int FM_P = 4;            // queries whose tables share one LDS entry
constexpr int FM_THREADS = 1024;   // the scan's workgroup: sixteen wavefronts, each owning one 64-bit accept word per row step
constexpr int FM_CLUSTERS = 256;   // ProductQuantization.DEFAULT_CLUSTERS

// the threshold scan over all n rows: (row, score) joins query q's list when bit `row` of q's mask is set and score >= tau[q]
struct FmScanParams {
    const float *luts;         // [Q][M * 256]
    const float *bmag;         // [Q] (cosine)
    const uint8_t *codes;      // [n][M], 16-byte aligned, M % 16 == 0
    const float *norms;        // [n] (cosine)
    const uint64_t *bits;      // mask q starts at bits + q * stride_words; bits at and beyond n and words past ceil(n / 64) are never used
    int64_t stride_words;      // 0: one mask for every query
    const float *tau;          // tau[q * tau_stride]
    int tau_stride;
    int32_t *cand_ids;         // [Q][cap]
    float *cand_scores;        // [Q][cap]
    unsigned int *cand_count;  // [Q], zero on entry; may end above cap (the entries past cap are dropped, the caller checks)
    int cap;
    int staged;                // collect a workgroup's survivors in LDS first (pays when a workgroup keeps dozens per query)
    int64_t n;
    int Q, M;
};

// samp[q][i] scores row i * stride: it becomes -INFINITY where q's mask rejects that row
struct FmSampleParams {
    float *samp;               // [Q][S]
    const uint64_t *bits;
    int64_t stride_words;      // 0: one mask for every query
    int64_t n, S, stride;      // (S - 1) * stride < n
    int Q;
};

// LDS of the scan: one slice of 16 SLCH subspaces, four queries per entry
constexpr size_t fm_scan_lds_bytes(int slch) { return (size_t)16 * slch * FM_CLUSTERS * 4 * sizeof(float); }

}  // namespace jv
