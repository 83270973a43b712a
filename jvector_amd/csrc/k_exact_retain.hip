// k_exact_retain.hip — batched VamanaDiversityProvider.retainDiverse scored float row against float row (xb_body.h), for gfx950.
// One wavefront per node, persistent blocks striding over the nodes.  A library of its own (libjvector_hip_xb.so) that
// libjvector_hip.so links: nothing here calls back into the main library, the launcher reports through its return code.
//
// LDS: one 17 KB row tile, the pair-score matrix [min(maxDegree, C)][C rounded up to 64] and four words per candidate, as dynamic LDS
// sized by the launch (36 KB at maxDegree 32 x C 128: four nodes per CU; above 64 KB the kernel opts in to gfx950's 160 KB).
// Registers: the score phase stages a chunk of up to 64 rows in sixteen float4 registers per lane while the previous chunk is
// computed out of the tile; the kernels are launch-bounded to one wavefront per workgroup.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "xb_body.h"

#define XB_EXPORT __attribute__((visibility("default")))

namespace jv {

template <int VSF, bool AL>
__global__ __launch_bounds__(64) void exact_retain_kernel(XbParams p)
{
    extern __shared__ __attribute__((aligned(16))) char xb_lds[];
    xb_worker<VSF, AL>(p, (int)blockIdx.x, (int)gridDim.x, xb_lds);
}

template <int VSF, bool AL>
static int launch_one(hipStream_t s, const XbParams &p, int blocks, size_t lds)
{
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute((const void *)exact_retain_kernel<VSF, AL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return JV_ERR_HIP;
    hipLaunchKernelGGL((exact_retain_kernel<VSF, AL>), dim3(blocks), dim3(64), lds, s, p);
    return JV_OK;
}

XB_EXPORT int launch_exact_retain(hipStream_t s, const XbParams &p, size_t p_bytes, int vsf, size_t lds_limit, int blocks)
{
    if (p_bytes != sizeof(XbParams) || vsf < VSF_L2 || vsf > VSF_COS) return JV_ERR_INVALID;
    if (p.P == 0) return JV_OK;
    if (p.P < 0 || blocks < 1 || p.C < 1 || p.C > XB_MAX_CANDIDATES || p.D < 1 || p.n < 0 || p.maxDegree < 1 || p.maxDegree > 64 || !p.rows ||
        !p.cand_nodes || !p.cand_scores || !p.selected_out || !p.n_selected_out || (vsf == VSF_COS && !p.vnorm))
        return JV_ERR_INVALID;
    const size_t lds = xb_lds_bytes(p.C, p.maxDegree);
    if (lds > lds_limit) return JV_ERR_UNSUPPORTED;
    const bool al = p.D % 4 == 0 && (reinterpret_cast<uintptr_t>(p.rows) & 15) == 0;
    int rc;
    switch (vsf) {
    case VSF_L2: rc = al ? launch_one<VSF_L2, true>(s, p, blocks, lds) : launch_one<VSF_L2, false>(s, p, blocks, lds); break;
    case VSF_DOT: rc = al ? launch_one<VSF_DOT, true>(s, p, blocks, lds) : launch_one<VSF_DOT, false>(s, p, blocks, lds); break;
    default: rc = al ? launch_one<VSF_COS, true>(s, p, blocks, lds) : launch_one<VSF_COS, false>(s, p, blocks, lds); break;
    }
    if (rc != JV_OK) return rc;
    if (hipGetLastError() != hipSuccess) return JV_ERR_HIP;
    return JV_OK;
}

}  // namespace jv
