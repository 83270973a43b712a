// k_bq_delete.hip — deleting nodes from a graph built over binary-quantized rows (bx_body.h), for gfx950: which live nodes have a marked
// neighbour (one wavefront per 64 nodes, then one wavefront that lists them in ascending order), and for each of them the two-hop
// candidates gathered, scored row against row, ordered and merged with the surviving neighbours into the list the robust prune reads
// (one wavefront per node, persistent blocks striding over the list; what a block holds is its node's keys in LDS).  Row widths of
// 1, 2, 4, 8, 12, 16 and 24 words are compiled unrolled; every other width runs the generic loop.  The bitmap helpers below them are
// one thread per word or per cell.
#include <algorithm>

#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"

#define GS_WAVE_SCOPE_BARRIER 1
#define GS_UNIFORM_SHFL 1
#include "gs_wave_hip.h"

#include "bx_body.h"

namespace jv {

__global__ __launch_bounds__(64) void bq_delete_affected_kernel(BxParams p) { bx_affected_word(p, (int64_t)blockIdx.x); }

__global__ __launch_bounds__(64) void bq_delete_compact_kernel(BxParams p) { bx_compact(p); }

template <int WT>
__global__ __launch_bounds__(64) void bq_delete_merge_kernel(BxParams p)
{
    extern __shared__ __attribute__((aligned(16))) char bx_lds[];
    bx_worker<WT>(p, (int)blockIdx.x, (int)gridDim.x, bx_lds);
}

// bits[id] |= 1 for the B ids (each inside the bitmap: the host has looked at them)
__global__ void bq_delete_set_bits_kernel(const int32_t *ids, int B, int64_t n, unsigned long long *bits)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= B) return;
    const int32_t id = ids[i];
    if (id >= 0 && id < n) atomicOr(bits + (id >> 6), 1ull << (id & 63));
}

// out = present & ~marked
__global__ void bq_delete_live_bits_kernel(const uint64_t *present, const uint64_t *marked, int64_t words, uint64_t *out)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < words) out[w] = present[w] & ~marked[w];
}

// the rows of the marked nodes: ids -1, scores 0, diverseBefore 0
__global__ void bq_delete_blank_rows_kernel(const uint64_t *marked, int64_t n, int R, int32_t *nbrs, float *nsc, int32_t *db)
{
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n * R) return;
    const int64_t node = cell / R;
    if (!((marked[node >> 6] >> (node & 63)) & 1ull)) return;
    nbrs[cell] = -1;
    nsc[cell] = 0.0f;
    if (cell == node * R) db[node] = 0;
}

// present &= ~marked; marked = 0
__global__ void bq_delete_retire_bits_kernel(uint64_t *present, uint64_t *marked, int64_t words)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    present[w] &= ~marked[w];
    marked[w] = 0;
}

int bq_delete_compiled_width(int W)
{
    switch (W) {
    case 1: case 2: case 4: case 8: case 12: case 16: case 24: return W;
    default: return 0;
    }
}

int launch_bq_delete_set_bits(hipStream_t s, const int32_t *d_ids, int B, int64_t n, uint64_t *d_bits)
{
    if (B <= 0) return JV_OK;
    hipLaunchKernelGGL(bq_delete_set_bits_kernel, dim3((B + 255) / 256), dim3(256), 0, s, d_ids, B, n, (unsigned long long *)d_bits);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

int launch_bq_delete_live_bits(hipStream_t s, const uint64_t *d_present, const uint64_t *d_marked, int64_t n, uint64_t *d_out)
{
    const int64_t words = (n + 63) / 64;
    hipLaunchKernelGGL(bq_delete_live_bits_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, d_present, d_marked, words, d_out);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

int launch_bq_delete_retire(hipStream_t s, uint64_t *d_present, uint64_t *d_marked, int64_t n, int R, int32_t *d_nbrs, float *d_nsc, int32_t *d_db)
{
    const int64_t words = (n + 63) / 64, cells = n * R;
    hipLaunchKernelGGL(bq_delete_blank_rows_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_marked, n, R, d_nbrs, d_nsc, d_db);
    JV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bq_delete_retire_bits_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, d_present, d_marked, words);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

// p.affected, p.tasks (room for n ids) and p.task_count are written
int launch_bq_delete_affected(hipStream_t s, const BxParams &p)
{
    if (p.n < 1 || p.n > 0x7fffffffLL || p.R < 1 || p.R > 64 || !p.affected || !p.tasks || !p.task_count) {
        set_error("bq delete kernels: bad launch parameters");
        return JV_ERR_INVALID;
    }
    const int64_t words = (p.n + 63) / 64;
    hipLaunchKernelGGL(bq_delete_affected_kernel, dim3((unsigned)words), dim3(64), 0, s, p);
    JV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bq_delete_compact_kernel, dim3(1), dim3(64), 0, s, p);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

template <int WT>
static int launch_merge(hipStream_t s, const BxParams &p, int blocks, size_t lds)
{
    if (lds > 48 * 1024)
        JV_HIP_CHECK(hipFuncSetAttribute((const void *)bq_delete_merge_kernel<WT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((bq_delete_merge_kernel<WT>), dim3(blocks), dim3(64), lds, s, p);
    return JV_OK;
}

int launch_bq_delete_merge(hipStream_t s, const jv_ctx *ctx, const BxParams &p)
{
    if (p.P == 0) return JV_OK;
    const int wt = bq_delete_compiled_width(p.W);
    const size_t lds = bx_lds_bytes(p.R, wt ? 0 : p.W);
    if (p.P < 0 || p.W < 1 || p.R < 1 || p.R > 64 || p.D < 1 || p.D > kBqMaxDim || lds > std::min<size_t>(65536, ctx->lds_per_block) ||
        (reinterpret_cast<uintptr_t>(p.rows) & 15) != 0 || (p.given && (p.G < 1 || p.G > 64 || !p.given_n)) || (p.list && (p.L < 1 || !p.lsc)) || !p.ln ||
        !p.cn || !p.tasks) {
        set_error("bq delete kernels: bad launch parameters");
        return JV_ERR_INVALID;
    }
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(16, ((size_t)160 << 10) / (lds + 256)));
    const int blocks = std::min(p.P, ctx->num_cus * per_cu);
    int rc;
    switch (wt) {
    case 1: rc = launch_merge<1>(s, p, blocks, lds); break;
    case 2: rc = launch_merge<2>(s, p, blocks, lds); break;
    case 4: rc = launch_merge<4>(s, p, blocks, lds); break;
    case 8: rc = launch_merge<8>(s, p, blocks, lds); break;
    case 12: rc = launch_merge<12>(s, p, blocks, lds); break;
    case 16: rc = launch_merge<16>(s, p, blocks, lds); break;
    case 24: rc = launch_merge<24>(s, p, blocks, lds); break;
    default: rc = launch_merge<0>(s, p, blocks, lds); break;
    }
    if (rc != JV_OK) return rc;
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

}  // namespace jv
