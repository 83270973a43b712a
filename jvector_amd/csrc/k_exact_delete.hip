// k_exact_delete.hip — deleting nodes from a graph built over float rows (xd_body.h), for gfx950: for each live node with a marked
// neighbour the two-hop ids gathered, de-duplicated, scored float row against float row, ordered and merged with the surviving
// neighbours into the list the robust prune reads.  One wavefront per node, persistent blocks striding over the list.  A library of its
// own (libjvector_hip_xd.so) that libjvector_hip.so links: nothing here calls back into the main library, the launcher reports through
// its return code.
//
// LDS: the 17 KB row tile of xg_body.h, the key array (the id array in its upper half) and 1 KB of survivor arrays, as dynamic LDS
// sized by the working row width (51 KB at 64: three nodes per CU; above 48 KB the kernel opts in).  Registers: the score phase stages
// up to 64 rows in sixteen float4 registers per lane while the chunk before is computed out of the tile; launch-bounded to one
// wavefront per workgroup.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "xd_body.h"

#define XD_EXPORT __attribute__((visibility("default")))

namespace jv {

template <int VSF, bool TR>
__global__ __launch_bounds__(64) void exact_delete_merge_kernel(XdParams p)
{
    extern __shared__ __attribute__((aligned(16))) char xd_lds[];
    xd_worker<VSF, TR>(p, (int)blockIdx.x, (int)gridDim.x, xd_lds);
}

template <int VSF, bool TR>
static int launch_one(hipStream_t s, const XdParams &p, int blocks, size_t lds)
{
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute((const void *)exact_delete_merge_kernel<VSF, TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return JV_ERR_HIP;
    hipLaunchKernelGGL((exact_delete_merge_kernel<VSF, TR>), dim3(blocks), dim3(64), lds, s, p);
    return JV_OK;
}

XD_EXPORT int launch_exact_delete_merge(hipStream_t s, const XdParams &p, size_t p_bytes, int vsf, size_t lds_limit, int blocks)
{
    if (p_bytes != sizeof(XdParams) || vsf < VSF_L2 || vsf > VSF_COS) return JV_ERR_INVALID;
    if (p.P == 0) return JV_OK;
    if (p.P < 0 || blocks < 1 || p.n < 1 || p.n > 0x7fffffffLL || p.D < 1 || p.R < 1 || p.R > 64 || !p.rows || !p.nbrs || !p.nsc || !p.marked || !p.tasks ||
        !p.ln || !p.cn || (p.given && (p.G < 1 || p.G > 64 || !p.given_n)) || (p.list && (p.L < 1 || !p.lsc)) || (vsf == VSF_COS && !p.vnorm))
        return JV_ERR_INVALID;
    const size_t lds = xd_lds_bytes(p.R);
    if (lds > lds_limit) return JV_ERR_UNSUPPORTED;
    const bool tr = p.D % 8 == 0 && (reinterpret_cast<uintptr_t>(p.rows) & 15) == 0;
    int rc;
    switch (vsf) {
    case VSF_L2: rc = tr ? launch_one<VSF_L2, true>(s, p, blocks, lds) : launch_one<VSF_L2, false>(s, p, blocks, lds); break;
    case VSF_DOT: rc = tr ? launch_one<VSF_DOT, true>(s, p, blocks, lds) : launch_one<VSF_DOT, false>(s, p, blocks, lds); break;
    default: rc = tr ? launch_one<VSF_COS, true>(s, p, blocks, lds) : launch_one<VSF_COS, false>(s, p, blocks, lds); break;
    }
    if (rc != JV_OK) return rc;
    if (hipGetLastError() != hipSuccess) return JV_ERR_HIP;
    return JV_OK;
}

}  // namespace jv
