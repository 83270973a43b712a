// k_bq_gsearch.hip — the one-wave graph traversal over binary-quantized vectors (bg_body.h), for gfx950.  One wavefront per
// query, persistent workers pulling queries off a counter.  Scoring is xor + popcount on integer registers: no table, no codebook
// gathers, a few dozen VGPRs — the LDS block of a worker (results, candidate tier, visited table) sets the waves per CU, not the
// register file.  Row widths of 1, 2, 4, 8, 12, 16 and 24 words (D up to 64 ... 1536) are compiled with the query's words in
// scalar registers; every other width runs the generic form with the words in LDS.
#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "bg_body.h"

namespace jv {

template <int WT, bool SAFE>
__global__ __launch_bounds__(64) void bq_graph_search_kernel(BgParams p)
{
    extern __shared__ __attribute__((aligned(16))) char bg_lds[];
    bg_worker<WT, SAFE>(p, (int)blockIdx.x, bg_lds);
}

int bq_graph_compiled_width(int W)
{
    switch (W) {
    case 1: case 2: case 4: case 8: case 12: case 16: case 24: return W;
    default: return 0;
    }
}

size_t bq_graph_lds_bytes(int rerankK, int cand_cap, int W, int vcap_log2) { return bg_lds_bytes(rerankK, cand_cap, bq_graph_compiled_width(W) ? 0 : W, vcap_log2); }

template <bool SAFE>
static void launch_width(hipStream_t s, const BgParams &p, int workers, size_t lds)
{
    dim3 grid(workers), block(64);
    switch (bq_graph_compiled_width(p.W)) {
    case 1: hipLaunchKernelGGL((bq_graph_search_kernel<1, SAFE>), grid, block, lds, s, p); break;
    case 2: hipLaunchKernelGGL((bq_graph_search_kernel<2, SAFE>), grid, block, lds, s, p); break;
    case 4: hipLaunchKernelGGL((bq_graph_search_kernel<4, SAFE>), grid, block, lds, s, p); break;
    case 8: hipLaunchKernelGGL((bq_graph_search_kernel<8, SAFE>), grid, block, lds, s, p); break;
    case 12: hipLaunchKernelGGL((bq_graph_search_kernel<12, SAFE>), grid, block, lds, s, p); break;
    case 16: hipLaunchKernelGGL((bq_graph_search_kernel<16, SAFE>), grid, block, lds, s, p); break;
    case 24: hipLaunchKernelGGL((bq_graph_search_kernel<24, SAFE>), grid, block, lds, s, p); break;
    default: hipLaunchKernelGGL((bq_graph_search_kernel<0, SAFE>), grid, block, lds, s, p); break;
    }
}

int launch_bq_graph_search(hipStream_t s, const BgParams &p, int workers, bool safe)
{
    if (p.Q == 0) return JV_OK;
    if (workers < 1 || p.cand_cap < BG_MIN_CAND_CAP || (!safe && (p.vcap_log2 < BG_MIN_VCAP_LOG2 || p.vcap_log2 > BG_MAX_VCAP_LOG2)) ||
        (safe && p.vcap_log2 != 0) || (reinterpret_cast<uintptr_t>(p.rows) & 15) != 0) {
        set_error("bq graph search kernel: bad launch parameters");
        return JV_ERR_INVALID;
    }
    const size_t lds = bq_graph_lds_bytes(p.rerankK, p.cand_cap, p.W, p.vcap_log2);
    if (lds > 65536) {
        set_error("bq graph search kernel: %zu bytes of LDS per worker", lds);
        return JV_ERR_UNSUPPORTED;
    }
    if (safe) launch_width<true>(s, p, workers, lds);
    else launch_width<false>(s, p, workers, lds);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

}  // namespace jv
