// k_nvq_gsearch.hip — the one-wave graph traversal scored on NVQ rows alone (ng_body.h), for gfx950: NVQVectors.scoreFunctionFor as
// GraphSearcher's score function, no float rows and no rerank.  One wavefront per query, persistent workers pulling queries off a
// counter.  A library of its own (libjvector_hip_ng.so) that libjvector_hip.so links: nothing here calls back into the main library, the
// launcher reports through its return code.  Six kernels: three similarities x FAST / SAFE visited structures.
//
// Score phase (ng_body.h has the whole argument): the fresh neighbours of an expansion are de-quantised by ALL 64 lanes, sixteen bytes
// of some row per lane, into an LDS tile of floats [R][CH + 4] (R x CH = 64 x 64, 32 x 128 or 16 x 256: 17 KB, the exact walk's footprint),
// then lane j runs NVQScorer's sequential fma chain over row j.  Banks: the chain's ds_read_b128 (16 consecutive rows per phase, row
// stride 4 mod 64 dwords) are conflict-free in every shape; the decode's ds_write_b128 are conflict-free in the 64 x 64 shape, 2-way in
// 32 x 128 and 4-way in 16 x 256 — four writes per piece under ~420 VALU instructions of decode.
//
// Registers: two stages of a chunk's loads per lane (4 x 16 bytes of rows, 4 derived quadruples, 16 floats of the element-wise operand)
// so that chunk c + 1 is in flight while chunk c is decoded; the kernels are launch-bounded to one wavefront per workgroup, so the
// allocator has the whole 512-register budget and the worker's LDS block sets the waves per CU.
// All fused operations are explicit __builtin_fmaf (the reference writes Math.fma); the Makefile's -ffp-contract=off keeps the rest apart.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "ng_body.h"

#define NG_EXPORT __attribute__((visibility("default")))

namespace jv {

template <int VSF, bool SAFE>
__global__ __launch_bounds__(64) void nvq_graph_search_kernel(NgParams p)
{
    extern __shared__ __attribute__((aligned(16))) char ng_lds[];
    ng_worker<VSF, SAFE>(p, (int)blockIdx.x, ng_lds);
}

template <int VSF>
static void launch_form(hipStream_t s, const NgParams &p, bool safe, int workers, size_t lds)
{
    const dim3 grid(workers), block(64);
    if (safe) hipLaunchKernelGGL((nvq_graph_search_kernel<VSF, true>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((nvq_graph_search_kernel<VSF, false>), grid, block, lds, s, p);
}

NG_EXPORT int launch_nvq_graph_search(hipStream_t s, const NgParams &p, size_t p_bytes, int vsf, int workers, bool safe)
{
    if (p_bytes != sizeof(NgParams) || vsf < VSF_L2 || vsf > VSF_COS) return JV_ERR_INVALID;
    if (p.Q == 0) return JV_OK;
    if (workers < 1 || p.D < 1 || p.rerankK < 1 || p.n_nodes < 1 || p.entry_node < 0 || p.entry_node >= p.n_nodes || p.entry_level < 0 ||
        p.entry_level >= GS_MAX_LEVELS || p.cand_cap < BG_MIN_CAND_CAP || p.spill_cap < 64 || !p.bytes || !p.derived || !p.queries || !p.qaux ||
        !p.spill || !p.out_ids || !p.out_scores || !p.out_stats || !p.out_status || !p.next_query)
        return JV_ERR_INVALID;
    if (safe ? (p.vcap_log2 != 0 || !p.bitmap || p.bitmap_words < ((long long)p.n_nodes + 31) / 32 || (p.bitmap_words & 3))
             : (p.vcap_log2 < BG_MIN_VCAP_LOG2 || p.vcap_log2 > BG_MAX_VCAP_LOG2 || (p.vcap_log2 > BG_VIS_LDS_MAX_LOG2 && !p.visited)))
        return JV_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(p.bytes) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.derived) & 15) != 0 || p.ld % 16 != 0 || p.ld < p.D ||
        p.S < 1 || p.S > p.D)
        return JV_ERR_INVALID;
    if (vsf == VSF_COS && (!p.cosnorm || !p.mean)) return JV_ERR_INVALID;
    const size_t lds = ng_lds_bytes(p.rerankK, p.cand_cap, p.vcap_log2);
    if (lds > 65536) return JV_ERR_UNSUPPORTED;
    switch (vsf) {
    case VSF_L2: launch_form<VSF_L2>(s, p, safe, workers, lds); break;
    case VSF_DOT: launch_form<VSF_DOT>(s, p, safe, workers, lds); break;
    default: launch_form<VSF_COS>(s, p, safe, workers, lds); break;
    }
    if (hipGetLastError() != hipSuccess) return JV_ERR_HIP;
    return JV_OK;
}

}  // namespace jv
