// k_gsearch_ubr.hip — the one-wave traversal with a REGISTER-resident upper-bound table (gs_body.h "UBR"); the dense kernel that
// builds the tables of a whole batch is k_ubr_table.hip.  A translation unit of its own: the traversal's other instantiations compile
// in parallel.
//
// Why: round 4's UB8 form (gone from the source since round 6) proved that 60 % of the neighbours a search scores can soundly be dropped behind an 8-bit upper bound of
// their score, and lost 2.3x to three removable overheads — the table built inside the traversal wave, 24 KB of LDS per wave, and
// survivors scored in place.  Here the table is built by ubr_table_kernel for all queries at once (codebook rows reused across 8
// queries, ~25 GB of L2 reads and 3.2 GB of HBM writes per 131 072 queries instead of 355 k clocks per query), lives in 96 of the
// wave's registers (two ds_bpermute_b32 per look-up: the LDS crossbar, no LDS bytes, so 8 waves per CU and the visited set's LDS
// tier stay), and what the bound cannot drop is compacted through LDS and scored eight lanes per neighbour.
#include "jv_device.h"
#include "jv_internal.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "gs_body.h"

namespace jv {

static_assert(VSF_L2 == 0 && VSF_DOT == 1 && VSF_COS == 2, "gs_body.h hard-codes the kernel vsf numbering");

template <int VSF, int CH16, bool PROF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void graph_search_ubr_kernel(GsParams p)
{
    extern __shared__ __attribute__((aligned(16))) char gs_lds[];
    gs_worker<VSF, CH16, true, PROF, false, false, true>(p, (int)blockIdx.x, gs_lds);
}

// the same bound form over the COMPACTED fresh list of rows up to 64 wide, codes by ordinal (gs_body.h PAIRC + UBR): the builder's searches
template <int VSF, int CH16, bool PROF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void graph_search_ubrc_kernel(GsParams p)
{
    extern __shared__ __attribute__((aligned(16))) char gs_lds[];
    gs_worker<VSF, CH16, false, PROF, false, true, true>(p, (int)blockIdx.x, gs_lds);
}

// the plain-search instantiation of the kernel above lives in a translation unit of its own (k_gsearch_ubr_plain.hip): in one module
// with the general kernels its code moved THEIR register allocation (the phase-clock build and the compacted form spilled more)
int launch_graph_search_ubr_plain(hipStream_t s, int vsf, const GsParams &p, int workers, size_t lds);

bool graph_search_ubr_supported(int M, int /*vsf*/) { return M == 96; }   // (round 6: euclidean too — lower bucket edges, gs_host.h)

int launch_graph_search_ubr(hipStream_t s, int vsf, const GsParams &p, int workers, size_t lds)
{
    if (p.Q == 0) return JV_OK;
    if (!p.pair || p.session || p.generic || !graph_search_ubr_supported(p.M, vsf) || !p.ubr_tab || !p.ubr_meta) {
        set_error("graph search kernel: the register-table bound form serves the pair-lane kernels at M = 96");
        return JV_ERR_INVALID;
    }
    // a search without mask, excluded id, query map and speculative touch (and no phase clocks): the instantiation without them
    if (gs_params_plain(p)) return launch_graph_search_ubr_plain(s, vsf, p, workers, lds);
    dim3 grid(workers), block(64);
#define JV_UBR(VSFV)                                                                                             \
    do {                                                                                                         \
        if (p.pair == 2) {   /* over the compacted fresh list (no phase-clock build) */                           \
            hipLaunchKernelGGL((graph_search_ubrc_kernel<VSFV, 6, false>), grid, block, lds, s, p);               \
        } else if (p.prof) hipLaunchKernelGGL((graph_search_ubr_kernel<VSFV, 6, true>), grid, block, lds, s, p);  \
        else hipLaunchKernelGGL((graph_search_ubr_kernel<VSFV, 6, false>), grid, block, lds, s, p);              \
    } while (0)
    if (vsf == VSF_L2) JV_UBR(VSF_L2);
    else if (vsf == VSF_DOT) JV_UBR(VSF_DOT);
    else JV_UBR(VSF_COS);
#undef JV_UBR
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

}  // namespace jv
