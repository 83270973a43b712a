// k_gsearch_ubr_plain.hip — the PLAIN-search instantiation of the register-table bound traversal (k_gsearch_ubr.hip; gs_body.h "PLAIN"):
// the kernel of a search that carries no acceptOrds mask, no excluded id, no query map and no speculative touch, and whose level 0 is
// found without a map look-up (gs_params_plain, gs_params.h) — the headline's.  What such a search never executes is not compiled in
// and holds no scalar registers across the expansion loop; the rare paths of the loop are laid out and spilled as rare.  Same
// results, counters, push log and status codes as the general kernel, which serves everything else (filtered searches, the retry
// pass, gs_prefetch = 1, gs_prof = 1, gs_plain = 0).
// A translation unit of its own: in one module with the general kernels this code changed their register allocation.
#include "jv_device.h"
#include "jv_internal.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "gs_body.h"

namespace jv {

template <int VSF, int CH16>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void graph_search_ubr_plain_kernel(GsParams p)
{
    extern __shared__ __attribute__((aligned(16))) char gs_lds[];
    gs_worker<VSF, CH16, true, false, false, false, true, true>(p, (int)blockIdx.x, gs_lds);
}

int launch_graph_search_ubr_plain(hipStream_t s, int vsf, const GsParams &p, int workers, size_t lds)
{
    if (p.Q == 0) return JV_OK;
    if (!gs_params_plain(p) || p.session || p.generic || p.M != 96 || !p.ubr_tab || !p.ubr_meta) {
        set_error("graph search kernel: the plain-search form serves unfiltered searches of the register-table bound form over the row");
        return JV_ERR_INVALID;
    }
    dim3 grid(workers), block(64);
    if (vsf == VSF_L2) hipLaunchKernelGGL((graph_search_ubr_plain_kernel<VSF_L2, 6>), grid, block, lds, s, p);
    else if (vsf == VSF_DOT) hipLaunchKernelGGL((graph_search_ubr_plain_kernel<VSF_DOT, 6>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((graph_search_ubr_plain_kernel<VSF_COS, 6>), grid, block, lds, s, p);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

}  // namespace jv
