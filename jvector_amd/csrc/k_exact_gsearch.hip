// k_exact_gsearch.hip — the one-wave graph traversal with exact scores over float rows (xg_body.h), for gfx950.  One wavefront per
// query, persistent workers pulling queries off a counter.  A library of its own (libjvector_hip_xg.so) that libjvector_hip.so links:
// nothing here calls back into the main library, the launcher reports through its return code.
//
// Registers: the score phase stages a chunk of up to 64 rows in sixteen float4 registers per lane while the previous chunk is
// computed out of the LDS tile; the kernels are launch-bounded to one wavefront per workgroup, so the allocator has the whole 512-register
// budget and the LDS block of a worker (17 KB of tile + queues + visited table) sets the waves per CU, not the register file.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "xg_body.h"

#define XG_EXPORT __attribute__((visibility("default")))

namespace jv {

template <int VSF, bool TR, bool SAFE>
__global__ __launch_bounds__(64) void exact_graph_search_kernel(XgParams p)
{
    extern __shared__ __attribute__((aligned(16))) char xg_lds[];
    xg_worker<VSF, TR, SAFE>(p, (int)blockIdx.x, xg_lds);
}

template <int VSF>
static void launch_form(hipStream_t s, const XgParams &p, bool tr, bool safe, int workers, size_t lds)
{
    const dim3 grid(workers), block(64);
    if (tr && safe) hipLaunchKernelGGL((exact_graph_search_kernel<VSF, true, true>), grid, block, lds, s, p);
    else if (tr) hipLaunchKernelGGL((exact_graph_search_kernel<VSF, true, false>), grid, block, lds, s, p);
    else if (safe) hipLaunchKernelGGL((exact_graph_search_kernel<VSF, false, true>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((exact_graph_search_kernel<VSF, false, false>), grid, block, lds, s, p);
}

XG_EXPORT int launch_exact_graph_search(hipStream_t s, const XgParams &p, size_t p_bytes, int vsf, bool tr, int workers, bool safe)
{
    if (p_bytes != sizeof(XgParams) || vsf < VSF_L2 || vsf > VSF_COS) return JV_ERR_INVALID;
    if (p.Q == 0) return JV_OK;
    if (workers < 1 || p.D < 1 || p.rerankK < 1 || p.n_nodes < 1 || p.entry_node < 0 || p.entry_node >= p.n_nodes || p.entry_level < 0 ||
        p.entry_level >= GS_MAX_LEVELS || p.cand_cap < BG_MIN_CAND_CAP || p.spill_cap < 64 || !p.rows || !p.queries || !p.spill || !p.out_ids ||
        !p.out_scores || !p.out_stats || !p.out_status || !p.next_query)
        return JV_ERR_INVALID;
    if (safe ? (p.vcap_log2 != 0 || !p.bitmap || p.bitmap_words < ((long long)p.n_nodes + 31) / 32 || (p.bitmap_words & 3))
             : (p.vcap_log2 < BG_MIN_VCAP_LOG2 || p.vcap_log2 > BG_MAX_VCAP_LOG2 || (p.vcap_log2 > BG_VIS_LDS_MAX_LOG2 && !p.visited)))
        return JV_ERR_INVALID;
    if (vsf == VSF_COS && (!p.qnorm || (tr && !p.vnorm))) return JV_ERR_INVALID;
    if (tr && (p.D % 8 != 0 || (reinterpret_cast<uintptr_t>(p.rows) & 15) != 0)) return JV_ERR_INVALID;
    const size_t lds = xg_lds_bytes(p.rerankK, p.cand_cap, p.vcap_log2);
    if (lds > 65536) return JV_ERR_UNSUPPORTED;
    switch (vsf) {
    case VSF_L2: launch_form<VSF_L2>(s, p, tr, safe, workers, lds); break;
    case VSF_DOT: launch_form<VSF_DOT>(s, p, tr, safe, workers, lds); break;
    default: launch_form<VSF_COS>(s, p, tr, safe, workers, lds); break;
    }
    if (hipGetLastError() != hipSuccess) return JV_ERR_HIP;
    return JV_OK;
}

}  // namespace jv
