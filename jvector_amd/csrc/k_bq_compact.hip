// k_bq_compact.hip — compacting a graph built over binary-quantized rows (bc_body.h), for gfx950: the sequential renumbering of the
// nodes in the graph as an exclusive scan over the present bitmap (per-block sums, one wavefront over the sums, the write-out with a
// lane per bit), then the adjacency rows and the BQ rows gathered under it, 64 consecutive cells per wavefront step so that every store
// is a whole line.  Streaming kernels: each byte is moved once.  The helper below them fills the present bits of the result.
//
// This file is a library of its own, jvector_amd/libjvector_hip_bqc.so, which libjvector_hip.so links: it uses nothing of the engine
// but the status codes, and its four launchers are its whole interface (bq_internal.h).  A launcher sets no error text — the caller in
// bq_builder.cpp does.  The kernels' resource baseline is tests/golden/kernel_resources_bq_compact.json.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"
#include "bc_params.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "bc_body.h"

#define BC_EXPORT __attribute__((visibility("default")))
#define BC_LAUNCHED()                                   \
    do {                                                \
        if (hipGetLastError() != hipSuccess) return JV_ERR_HIP; \
    } while (0)

namespace jv {

__global__ __launch_bounds__(64) void bq_compact_rank_sums_kernel(BcParams p) { bc_rank_sums(p, (int64_t)blockIdx.x); }

__global__ __launch_bounds__(64) void bq_compact_rank_scan_kernel(BcParams p) { bc_rank_scan(p); }

__global__ __launch_bounds__(64) void bq_compact_rank_write_kernel(BcParams p) { bc_rank_write(p, (int64_t)blockIdx.x); }

__global__ __launch_bounds__(64) void bq_compact_rows_kernel(BcParams p) { bc_rows(p, (int64_t)blockIdx.x); }

__global__ __launch_bounds__(64) void bq_compact_bq_rows_kernel(BcParams p) { bc_bq_rows(p, (int64_t)blockIdx.x); }

// bits [0, live) set, the rest of the `words` words clear
__global__ void bq_compact_fill_bits_kernel(uint64_t *bits, int64_t words, int64_t live)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    const int64_t left = live - w * 64;
    bits[w] = left >= 64 ? ~0ull : (left > 0 ? (1ull << left) - 1ull : 0ull);
}

// p.block_base (bc_scan_blocks(n) words), p.counters (3 words), p.old_to_new (n) and p.new_to_old (nullable; as many as there are live nodes) are written
BC_EXPORT int launch_bq_compact_rank(hipStream_t s, const BcParams &p, size_t p_bytes)
{
    if (p_bytes != sizeof(BcParams) || p.n < 1 || p.n > 0x7fffffffLL || !p.present || !p.block_base || !p.counters || !p.old_to_new) return JV_ERR_INVALID;
    const int64_t words = (p.n + 63) / 64;
    hipLaunchKernelGGL(bq_compact_rank_sums_kernel, dim3((unsigned)bc_scan_blocks(p.n)), dim3(64), 0, s, p);
    BC_LAUNCHED();
    hipLaunchKernelGGL(bq_compact_rank_scan_kernel, dim3(1), dim3(64), 0, s, p);
    BC_LAUNCHED();
    hipLaunchKernelGGL(bq_compact_rank_write_kernel, dim3((unsigned)((words + 63) / 64)), dim3(64), 0, s, p);
    BC_LAUNCHED();
    return JV_OK;
}

// rows [0, p.live) of the destination adjacency; p.counters[1] / [2] take the ids without an image
BC_EXPORT int launch_bq_compact_rows(hipStream_t s, const BcParams &p, size_t p_bytes)
{
    if (p_bytes != sizeof(BcParams)) return JV_ERR_INVALID;
    if (p.live == 0) return JV_OK;
    if (p.n < 1 || p.n > 0x7fffffffLL || p.live < 0 || p.live > p.n || p.R < 1 || p.R > 64 || !p.old_to_new || !p.new_to_old || !p.counters || !p.src_nbrs ||
        !p.src_nsc || !p.src_db || !p.dst_nbrs || !p.dst_nsc || !p.dst_db)
        return JV_ERR_INVALID;
    hipLaunchKernelGGL(bq_compact_rows_kernel, dim3((unsigned)bc_wave_count(p.live * p.R)), dim3(64), 0, s, p);
    BC_LAUNCHED();
    return JV_OK;
}

// rows [0, p.live) of the destination BQ rows (W <= 256: the widest row the BQ builder takes)
BC_EXPORT int launch_bq_compact_bq_rows(hipStream_t s, const BcParams &p, size_t p_bytes)
{
    if (p_bytes != sizeof(BcParams)) return JV_ERR_INVALID;
    if (p.live == 0) return JV_OK;
    if (p.n < 1 || p.n > 0x7fffffffLL || p.live < 0 || p.live > p.n || p.W < 1 || p.W > 256 || !p.new_to_old || !p.src_rows || !p.dst_rows)
        return JV_ERR_INVALID;
    hipLaunchKernelGGL(bq_compact_bq_rows_kernel, dim3((unsigned)bc_wave_count(p.live * p.W)), dim3(64), 0, s, p);
    BC_LAUNCHED();
    return JV_OK;
}

BC_EXPORT int launch_bq_compact_fill_bits(hipStream_t s, uint64_t *d_bits, int64_t n, int64_t live)
{
    if (n < 1 || !d_bits) return JV_ERR_INVALID;
    const int64_t words = (n + 63) / 64;
    hipLaunchKernelGGL(bq_compact_fill_bits_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, d_bits, words, live);
    BC_LAUNCHED();
    return JV_OK;
}

}  // namespace jv
