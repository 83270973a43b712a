// k_flat_accept.hip — the kernels of the flat PQ search under an accept filter (fa_body.h), for gfx950: the accept masks compacted to
// ascending ordinal lists by an exclusive scan (per-block sums, one wavefront per mask over the sums, the write-out with a lane per
// bit), the multi-query ADC scan over such a list (four queries' tables interleaved in LDS, cycled in slices), and the map from list
// positions back to ordinals.  No atomics.
//
// This file is a library of its own, jvector_amd/libjvector_hip_fa.so, which libjvector_hip.so links: it uses nothing of the engine
// but the status codes, and its four launchers are its whole interface (fa_params.h holds their parameters, flat_accept.cpp declares
// them).  A launcher sets no error text — the caller does.  The kernels' resource baseline is
// tests/golden/kernel_resources_flat_accept.json.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"
#include "fa_params.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "fa_body.h"

#define FA_EXPORT __attribute__((visibility("default")))
#define FA_LAUNCHED()                                   \
    do {                                                \
        if (hipGetLastError() != hipSuccess) return JV_ERR_HIP; \
    } while (0)

namespace jv {

constexpr int FA_GRID_Y = 32768;   // masks / list rows per launch (grid.y holds 65535)

__global__ __launch_bounds__(64) void flat_accept_sums_kernel(FaScanParams p, int y0) { fa_sums(p, (int64_t)y0 + blockIdx.y, (int64_t)blockIdx.x); }

__global__ __launch_bounds__(64) void flat_accept_scan_kernel(FaScanParams p) { fa_scan(p, (int64_t)blockIdx.x); }

__global__ __launch_bounds__(64) void flat_accept_write_kernel(FaScanParams p, int y0) { fa_write(p, (int64_t)y0 + blockIdx.y, (int64_t)blockIdx.x); }

template <int VSF, int SLCH, int R>
__global__ __launch_bounds__(FA_THREADS) void adc_mq_list_kernel(FaAdcParams p)
{
    extern __shared__ __attribute__((aligned(16))) FaF4 fa_lds4[];   // [16 SLCH x 256]
    fa_adc_list<VSF, SLCH, R, FA_THREADS>(p, (int)blockIdx.y, (int64_t)blockIdx.x, fa_lds4);
}

__global__ __launch_bounds__(256) void flat_accept_map_kernel(FaMapParams p) { fa_map(p, (int64_t)blockIdx.x * 256 + threadIdx.x); }

// `masks` masks of p.bits: p.block_base ([masks][p.blocks]) and p.totals ([masks]) are written
FA_EXPORT int launch_flat_accept_count(hipStream_t s, const FaScanParams &p, size_t p_bytes, int masks)
{
    if (p_bytes != sizeof(FaScanParams) || masks < 1 || p.n < 1 || p.n > 0x7fffffffLL || p.blocks != fa_scan_blocks(p.n) || !p.bits || !p.block_base ||
        !p.totals || p.stride_words < 0 || (masks > 1 && p.stride_words < (p.n + 63) / 64))
        return JV_ERR_INVALID;
    for (int y0 = 0; y0 < masks; y0 += FA_GRID_Y) {
        const int ny = masks - y0 < FA_GRID_Y ? masks - y0 : FA_GRID_Y;
        hipLaunchKernelGGL(flat_accept_sums_kernel, dim3((unsigned)p.blocks, (unsigned)ny), dim3(64), 0, s, p, y0);
        FA_LAUNCHED();
    }
    hipLaunchKernelGGL(flat_accept_scan_kernel, dim3((unsigned)masks), dim3(64), 0, s, p);
    FA_LAUNCHED();
    return JV_OK;
}

// rows [0, rows) of p.lists, each p.L entries: row y from mask p.first_mask + y (from the one mask when p.stride_words == 0)
FA_EXPORT int launch_flat_accept_write(hipStream_t s, const FaScanParams &p, size_t p_bytes, int rows)
{
    if (p_bytes != sizeof(FaScanParams) || rows < 1 || p.n < 1 || p.n > 0x7fffffffLL || p.blocks != fa_scan_blocks(p.n) || !p.bits || !p.block_base ||
        !p.totals || !p.lists || p.L < 1 || p.L > fa_segments(p.n) * FA_SEG_ROWS || p.first_mask < 0 || p.stride_words < 0)
        return JV_ERR_INVALID;
    for (int y0 = 0; y0 < rows; y0 += FA_GRID_Y) {
        const int ny = rows - y0 < FA_GRID_Y ? rows - y0 : FA_GRID_Y;
        hipLaunchKernelGGL(flat_accept_write_kernel, dim3((unsigned)fa_segments(p.n), (unsigned)ny), dim3(64), 0, s, p, y0);
        FA_LAUNCHED();
    }
    return JV_OK;
}

template <int VSF, int SLCH>
static int launch_list_r(hipStream_t s, const FaAdcParams &p, int R)
{
    const size_t lds = fa_adc_lds_bytes(SLCH);
#define FA_MQ(RR)                                                                                                             \
    do {                                                                                                                      \
        auto kfn = adc_mq_list_kernel<VSF, SLCH, RR>;                                                                         \
        if (hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {     \
            (void)hipGetLastError();                                                                                          \
            return JV_ERR_HIP;                                                                                                \
        }                                                                                                                     \
        dim3 grid((unsigned)((p.count + FA_THREADS * RR - 1) / (FA_THREADS * RR)), (unsigned)((p.Q + FA_P - 1) / FA_P));      \
        hipLaunchKernelGGL(kfn, grid, dim3(FA_THREADS), lds, s, p);                                                           \
    } while (0)
    // (cosine keeps four entries per lane: with eight, the 32 sums, the 8 rows and the double-precision finish together pass the
    // 128 registers a 1024-thread workgroup allows and the kernel spills)
    if constexpr (VSF != 2) {
        if (R >= 8) {
            FA_MQ(8);
            FA_LAUNCHED();
            return JV_OK;
        }
    }
    FA_MQ(4);
#undef FA_MQ
    FA_LAUNCHED();
    return JV_OK;
}

template <int VSF>
static int launch_list_slch(hipStream_t s, const FaAdcParams &p, int R)
{
    if (p.M % 32 == 0) return launch_list_r<VSF, 2>(s, p, R);
    return launch_list_r<VSF, 1>(s, p, R);
}

// p.out[q][i] for i < p.count; vsf: the kernel numbering (0 EUCLIDEAN, 1 DOT_PRODUCT, 2 COSINE)
FA_EXPORT int launch_flat_accept_adc_list(hipStream_t s, const FaAdcParams &p, size_t p_bytes, int vsf, int num_cus)
{
    if (p_bytes != sizeof(FaAdcParams)) return JV_ERR_INVALID;
    if (p.Q == 0 || p.count == 0) return JV_OK;
    if (p.Q < 0 || p.Q > 4 * 65535 || p.count < 0 || p.count > p.L || p.n < 1 || p.M < 16 || p.M % 16 != 0 || !p.luts || !p.codes || !p.list || !p.out ||
        (reinterpret_cast<uintptr_t>(p.codes) & 15) != 0 || vsf < 0 || vsf > 2 || (vsf == 2 && (!p.bmag || !p.norms)))
        return JV_ERR_INVALID;
    // list entries per lane: amortise the per-slice table refill, but keep >= ~2 workgroups per CU in the grid
    const int64_t groups = (p.Q + FA_P - 1) / FA_P;
    const int R = groups * ((p.count + FA_THREADS * 8 - 1) / (FA_THREADS * 8)) >= 2 * (int64_t)num_cus ? 8 : 4;
    switch (vsf) {
    case 0: return launch_list_slch<0>(s, p, R);
    case 1: return launch_list_slch<1>(s, p, R);
    default: return launch_list_slch<2>(s, p, R);
    }
}

FA_EXPORT int launch_flat_accept_map(hipStream_t s, const FaMapParams &p, size_t p_bytes)
{
    if (p_bytes != sizeof(FaMapParams)) return JV_ERR_INVALID;
    if (p.cells == 0) return JV_OK;
    if (p.cells < 0 || p.count < 0 || !p.ids || (p.count > 0 && !p.list)) return JV_ERR_INVALID;
    hipLaunchKernelGGL(flat_accept_map_kernel, dim3((unsigned)((p.cells + 255) / 256)), dim3(256), 0, s, p);
    FA_LAUNCHED();
    return JV_OK;
}

}  // namespace jv
