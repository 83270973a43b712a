// k_bq_builder.hip — the entry point of a graph built from binary-quantized rows (bm_body.h), for gfx950: the bitwise-majority row of the
// top level's members (one wavefront per 64-bit word) and the member at minimum Hamming distance to it, ties to the smaller id (an
// integer key per member, reduced across the wave, then across the waves by one wave of a second launch).  The top level holds a few
// thousand rows at most: correctness matters here, time does not.
#include <algorithm>

#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "bm_body.h"

namespace jv {

__global__ __launch_bounds__(64) void bq_majority_kernel(BmParams p) { bm_majority_word(p, (int)blockIdx.x); }

__global__ __launch_bounds__(64) void bq_nearest_row_kernel(BmParams p) { bm_nearest_partial(p, (int)blockIdx.x); }

__global__ __launch_bounds__(64) void bq_nearest_final_kernel(BmParams p) { bm_nearest_final(p); }

int bq_entry_waves(int n) { return std::max(1, std::min(1024, (n + 63) / 64)); }

// d_work: W words for the majority row, then bq_entry_waves(n) + 1 keys; the smallest key lands in the last of them
size_t bq_entry_work_bytes(int W, int n) { return sizeof(uint64_t) * (size_t)W + sizeof(long long) * ((size_t)bq_entry_waves(n) + 1); }

int launch_bq_entry(hipStream_t s, const uint64_t *d_rows, int64_t n_rows, int W, const int32_t *d_members, int n, void *d_work, long long **d_best)
{
    if (n < 1 || W < 1 || (reinterpret_cast<uintptr_t>(d_work) & 7) != 0) {
        set_error("bq entry kernels: bad launch parameters");
        return JV_ERR_INVALID;
    }
    BmParams p{};
    p.rows = d_rows;
    p.n_rows = n_rows;
    p.W = W;
    p.members = d_members;
    p.n = n;
    p.centroid = (uint64_t *)d_work;
    p.partial = (long long *)(p.centroid + W);
    p.waves = bq_entry_waves(n);
    p.best = p.partial + p.waves;
    hipLaunchKernelGGL(bq_majority_kernel, dim3(W), dim3(64), 0, s, p);
    JV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bq_nearest_row_kernel, dim3(p.waves), dim3(64), 0, s, p);
    JV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bq_nearest_final_kernel, dim3(1), dim3(64), 0, s, p);
    JV_HIP_CHECK(hipGetLastError());
    *d_best = p.best;
    return JV_OK;
}

}  // namespace jv
