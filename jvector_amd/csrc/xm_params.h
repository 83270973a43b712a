// xm_params.h — launch parameters of the exact-score builder's own kernels (xm_body.h / k_exact_builder.hip), shared with the host driver
// in exact_builder.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

struct ihipStream_t;

namespace jv {

constexpr int XM_MAX_WAVES = 1024;   // one-wave workgroups of the nearest-member scan: each strides over groups of 64 members

// out[i][0 .. D) = rows[ids[i]][0 .. D): the compacted copy of a level's members (an id outside [0, n) gives a row of zeros)
struct XmGatherParams {
    const float *rows;    // [n][D]
    int64_t n;
    int32_t D;
    const int32_t *ids;   // [count]
    int64_t count;
    float *out;           // [count][D]
};

// the entry point of a layered graph: the member of `ids` that scores highest against the members' mean row
struct XmEntryParams {
    const float *rows;     // [n][D]
    const float *vnorm;    // [n] per-row sums of squares (launch_row_sqnorms); COSINE with the transposing score phase only
    int64_t n;
    int32_t D;
    const int32_t *ids;    // [count] ascending, every one inside [0, n)
    int32_t count;
    float *mean;           // [D] written by the mean kernel, read by the scan
    long long *wave_best;  // [waves] the best key of each workgroup of the scan
    int32_t waves;
    long long *best;       // [1] the best key: sortableInt(score) << 32 | ~id
};

// the device block an entry-point pick works in: [mean: D floats, padded to 256 bytes][wave_best: XM_MAX_WAVES keys][best]
constexpr size_t xm_entry_mean_bytes(int D) { return (sizeof(float) * (size_t)D + 255) & ~(size_t)255; }
constexpr size_t xm_entry_work_bytes(int D) { return xm_entry_mean_bytes(D) + sizeof(long long) * ((size_t)XM_MAX_WAVES + 1); }
// workgroups of the scan over `count` members
constexpr int xm_entry_waves(int count) { return (count + 63) / 64 < XM_MAX_WAVES ? (count + 63) / 64 : XM_MAX_WAVES; }

// k_exact_builder.hip (libjvector_hip_xm.so).  vsf: VSF_L2 / VSF_DOT / VSF_COS.  Return JV_OK, JV_ERR_INVALID (bad parameters) or
// JV_ERR_HIP; nothing is read back.
int launch_xm_gather_rows(ihipStream_t *s, const XmGatherParams &p, size_t p_bytes);
int launch_xm_entry(ihipStream_t *s, const XmEntryParams &p, size_t p_bytes, int vsf);

}  // namespace jv
