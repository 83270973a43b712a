// k_exact_builder.hip — the exact-score builder's own kernels (xm_body.h), for gfx950: the gather of an upper level's float rows into a
// compacted set, and the entry point of a layered graph (mean row, nearest member, pick).  A library of its own
// (libjvector_hip_xm.so) that libjvector_hip.so links: nothing here calls back into the main library, the launchers report through
// their return codes.
//
// Gather: workgroups of 256 threads, 16 / 8 / 4 rows per pass.  Mean: one wavefront per 64 dimensions.  Nearest: one-wave workgroups
// (the row tile's sync points are wave-scope), each with the 17 KB tile of xg_body.h as static LDS and sixteen float4 staging registers
// per lane; launch-bounded to one wavefront, so the allocator has the whole register budget.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "xm_body.h"

#define XM_EXPORT __attribute__((visibility("default")))

namespace jv {

template <int LPR, bool AL>
__global__ __launch_bounds__(256) void exact_gather_rows_kernel(XmGatherParams p)
{
    xm_gather_rows<LPR, AL>(p, (int)threadIdx.x, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(64) void exact_entry_mean_kernel(XmEntryParams p) { xm_mean(p, (int)(blockIdx.x * 64 + threadIdx.x)); }

template <int VSF, bool TR>
__global__ __launch_bounds__(64) void exact_entry_nearest_kernel(XmEntryParams p)
{
    __shared__ __attribute__((aligned(16))) float xm_tile[XG_TILE_FLOATS];
    xm_nearest<VSF, TR>(p, (int)blockIdx.x, xm_tile);
}

__global__ __launch_bounds__(64) void exact_entry_pick_kernel(XmEntryParams p) { xm_pick(p); }

template <int LPR>
static void launch_gather(hipStream_t s, const XmGatherParams &p, bool al)
{
    const int64_t passes = (p.count + 256 / LPR - 1) / (256 / LPR);
    const dim3 grid((unsigned)(passes < 65536 ? passes : 65536)), block(256);
    if (al) hipLaunchKernelGGL((exact_gather_rows_kernel<LPR, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((exact_gather_rows_kernel<LPR, false>), grid, block, 0, s, p);
}

XM_EXPORT int launch_xm_gather_rows(hipStream_t s, const XmGatherParams &p, size_t p_bytes)
{
    if (p_bytes != sizeof(XmGatherParams)) return JV_ERR_INVALID;
    if (p.count == 0) return JV_OK;
    if (p.count < 0 || p.D < 1 || p.n < 1 || !p.rows || !p.ids || !p.out) return JV_ERR_INVALID;
    const bool al = p.D % 4 == 0 && ((reinterpret_cast<uintptr_t>(p.rows) | reinterpret_cast<uintptr_t>(p.out)) & 15) == 0;
    const int pieces = al ? p.D / 4 : p.D;   // what a group of lanes shares out: 16-byte pieces, or dwords
    if (pieces <= 16) launch_gather<16>(s, p, al);
    else if (pieces <= 32) launch_gather<32>(s, p, al);
    else launch_gather<64>(s, p, al);
    if (hipGetLastError() != hipSuccess) return JV_ERR_HIP;
    return JV_OK;
}

template <int VSF>
static void launch_nearest(hipStream_t s, const XmEntryParams &p, bool tr)
{
    const dim3 grid(p.waves), block(64);
    if (tr) hipLaunchKernelGGL((exact_entry_nearest_kernel<VSF, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((exact_entry_nearest_kernel<VSF, false>), grid, block, 0, s, p);
}

XM_EXPORT int launch_xm_entry(hipStream_t s, const XmEntryParams &p, size_t p_bytes, int vsf)
{
    if (p_bytes != sizeof(XmEntryParams) || vsf < VSF_L2 || vsf > VSF_COS) return JV_ERR_INVALID;
    if (p.count < 1 || p.D < 1 || p.n < 1 || !p.rows || !p.ids || !p.mean || !p.wave_best || !p.best || p.waves != xm_entry_waves(p.count))
        return JV_ERR_INVALID;
    const bool tr = p.D % 8 == 0 && ((reinterpret_cast<uintptr_t>(p.rows) | reinterpret_cast<uintptr_t>(p.mean)) & 15) == 0;
    if (vsf == VSF_COS && tr && !p.vnorm) return JV_ERR_INVALID;
    hipLaunchKernelGGL(exact_entry_mean_kernel, dim3((p.D + 63) / 64), dim3(64), 0, s, p);
    switch (vsf) {
    case VSF_L2: launch_nearest<VSF_L2>(s, p, tr); break;
    case VSF_DOT: launch_nearest<VSF_DOT>(s, p, tr); break;
    default: launch_nearest<VSF_COS>(s, p, tr); break;
    }
    hipLaunchKernelGGL(exact_entry_pick_kernel, dim3(1), dim3(64), 0, s, p);
    if (hipGetLastError() != hipSuccess) return JV_ERR_HIP;
    return JV_OK;
}

}  // namespace jv
