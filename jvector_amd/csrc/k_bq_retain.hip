// k_bq_retain.hip — batched VamanaDiversityProvider.retainDiverse scored row against row over binary-quantized vectors
// (bd_body.h), for gfx950.  One wavefront per node, persistent blocks striding over the nodes; a test is xor + popcount over W words
// per lane and one f32 division.  No table, no codebook: what a block holds is its node's candidate rows in LDS, and that LDS block
// sets the waves per CU.  Row widths of 1, 2, 4, 8, 12, 16 and 24 words are compiled unrolled; every other width runs the generic loop.
#include <algorithm>

#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "bd_body.h"

namespace jv {

template <int WT>
__global__ __launch_bounds__(64) void bq_retain_kernel(BdParams p)
{
    extern __shared__ __attribute__((aligned(16))) char bd_lds[];
    bd_worker<WT>(p, (int)blockIdx.x, (int)gridDim.x, bd_lds);
}

int bq_retain_compiled_width(int W)
{
    switch (W) {
    case 1: case 2: case 4: case 8: case 12: case 16: case 24: return W;
    default: return 0;
    }
}

size_t bq_retain_lds_bytes(int C, int W) { return bd_lds_bytes(C, W); }

template <int WT>
static int launch_one(hipStream_t s, const BdParams &p, int blocks, size_t lds)
{
    if (lds > 48 * 1024)
        JV_HIP_CHECK(hipFuncSetAttribute((const void *)bq_retain_kernel<WT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((bq_retain_kernel<WT>), dim3(blocks), dim3(64), lds, s, p);
    return JV_OK;
}

int launch_bq_retain(hipStream_t s, const jv_ctx *ctx, const BdParams &p)
{
    if (p.P == 0) return JV_OK;
    const size_t lds = bd_lds_bytes(p.C, p.W);
    if (p.C < 1 || p.C > BD_MAX_CANDIDATES || p.W < 1 || p.maxDegree < 1 || p.maxDegree > 64 || lds > std::min<size_t>(65536, ctx->lds_per_block) ||
        (reinterpret_cast<uintptr_t>(p.rows) & 7) != 0) {
        set_error("bq retain kernel: bad launch parameters");
        return JV_ERR_INVALID;
    }
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / (lds + 256)));
    const int blocks = std::min(p.P, ctx->num_cus * per_cu);
    int rc;
    switch (bq_retain_compiled_width(p.W)) {
    case 1: rc = launch_one<1>(s, p, blocks, lds); break;
    case 2: rc = launch_one<2>(s, p, blocks, lds); break;
    case 4: rc = launch_one<4>(s, p, blocks, lds); break;
    case 8: rc = launch_one<8>(s, p, blocks, lds); break;
    case 12: rc = launch_one<12>(s, p, blocks, lds); break;
    case 16: rc = launch_one<16>(s, p, blocks, lds); break;
    case 24: rc = launch_one<24>(s, p, blocks, lds); break;
    default: rc = launch_one<0>(s, p, blocks, lds); break;
    }
    if (rc != JV_OK) return rc;
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

}  // namespace jv
