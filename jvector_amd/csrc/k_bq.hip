// k_bq.hip — binary quantization (include/jvector_bq.h): encode, the gather scorer and the flat scan with its exact selection.
//
// Encode: one wave per (row, word).  Lane j tests v[64 w + j] > 0 on the float's bits (positive, not NaN: the reference's `>`
// whatever the denormal mode) and one __ballot is exactly the reference's long (bit j = lane j; lanes at and beyond D read
// nothing and give 0).
//
// Flat scan (bq_scan_kernel): a lane per row, a tile of QT queries per block.  The tile's query words sit in device memory
// transposed ([w][t]) and are read at wave-uniform addresses, so one row load serves QT queries and the inner step per
// (query, 64-bit word) is two v_xor_b32 and two v_bcnt_u32_b32 (the count accumulates into the distance).  Blocks own
// CONTIGUOUS row ranges [xb R, (xb + 1) R): block order is id order, which the tie ranks below rely on.  Three modes over the
// same loop:
//   HIST  per-block LDS histogram of the accepted rows' distances (QT x (D + 1) counters), added to the global one at the end;
//   EMIT  with the threshold t_q of each query (bq_threshold_kernel: smallest t with #{h <= t} >= k1): rows with h < t_q are
//         appended to the query's list; rows with h == t_q too when all of them fit the list (the usual case — top-k then
//         keeps the smallest ids), otherwise only counted per block;
//   RANK  only for queries whose ties did not fit: blocks whose exclusive prefix of tie counts is below the number still needed
//         walk their rows again in order and append ties by rank (prefix + ballot / mbcnt inside the block).  Every other
//         block returns at once.
// No Q x N score matrix exists anywhere; the lists hold at most cap entries per query.
#include "jv_device.h"
#include "jv_internal.h"
#include "bq_internal.h"

namespace jv {

__device__ __forceinline__ bool bq_bit(float v)
{
    const int32_t b = __float_as_int(v);
    return b > 0 && b <= 0x7f800000;   // +denormal .. +inf; NaN, -x, +-0 give false (Java: v > 0)
}

// out word index of (row r, word w): plain rows (tq == 0) or the scan's tile layout [r / tq][w][r % tq]
__global__ __launch_bounds__(256) void bq_encode_kernel(const float *__restrict__ src, int64_t count, int D, int W, int tq,
                                                         uint64_t *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= count * W) return;
    const int lane = threadIdx.x & 63;
    const int64_t r = g / W;
    const int w = (int)(g - r * W);
    const int idx = 64 * w + lane;
    const bool bit = idx < D && bq_bit(src[r * (int64_t)D + idx]);
    const uint64_t word = __ballot(bit);
    if (lane == 0) {
        const int64_t o = tq ? ((r / tq) * W + w) * tq + (r % tq) : r * W + w;
        out[o] = word;
    }
}

int launch_bq_encode(hipStream_t s, const float *d_src, int64_t count, int D, int W, int tq, uint64_t *d_out)
{
    if (count == 0) return JV_OK;
    const int64_t waves = count * W;
    hipLaunchKernelGGL(bq_encode_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, d_src, count, D, W, tq, d_out);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

__device__ __forceinline__ float bq_similarity(uint32_t h, int D) { return 1.0f - (float)h / (float)D; }

// out[p * B + b]: query words = qwords row p (scores) or rows[node1[p]] (pair scores)
__global__ __launch_bounds__(256) void bq_gather_kernel(const uint64_t *__restrict__ rows, int64_t N, int W, int D,
                                                         const uint64_t *__restrict__ qwords, const int32_t *__restrict__ node1,
                                                         int P, const int32_t *__restrict__ ord, int B, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)P * B) return;
    const int64_t p = i / B;
    const int32_t o = ord[i];
    const uint64_t *a;
    if (node1) {
        const int32_t n1 = node1[p];
        if (n1 < 0 || n1 >= N) { out[i] = -INFINITY; return; }
        a = rows + (int64_t)n1 * W;
    } else {
        a = qwords + p * W;
    }
    if (o < 0 || o >= N) { out[i] = -INFINITY; return; }
    const uint64_t *b = rows + (int64_t)o * W;
    uint32_t h = 0;
    for (int w = 0; w < W; ++w) h += __popcll(a[w] ^ b[w]);
    out[i] = bq_similarity(h, D);
}

int launch_bq_gather(hipStream_t s, const uint64_t *d_rows, int64_t N, int W, int D, const uint64_t *d_qwords, const int32_t *d_node1,
                     int P, const int32_t *d_ord, int B, float *d_out)
{
    const int64_t n = (int64_t)P * B;
    if (n == 0) return JV_OK;
    hipLaunchKernelGGL(bq_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_rows, N, W, D, d_qwords, d_node1, P,
                       d_ord, B, d_out);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// flat scan
// ---------------------------------------------------------------------------------------------------------------------------
enum : int { BQ_HIST = 0, BQ_EMIT = 1, BQ_RANK = 2 };

__device__ __forceinline__ bool bq_accepted(const uint64_t *__restrict__ acc, int64_t stride, int q, int64_t r)
{
    return acc == nullptr || ((acc[(int64_t)q * stride + (r >> 6)] >> (r & 63)) & 1ull);
}

__device__ __forceinline__ void bq_append(const BqScanArgs &a, int q, int64_t r, uint32_t h)
{
    const unsigned int slot = atomicAdd(&a.cand_cnt[q], 1u);
    if (slot < (unsigned int)a.cap) {   // (never false: the host sized the lists for every count it can reach)
        a.cand_ids[(int64_t)q * a.cap + slot] = (int32_t)r;
        a.cand_sc[(int64_t)q * a.cap + slot] = bq_similarity(h, a.D);
    }
}

template <int QT, int MODE>
__global__ __launch_bounds__(256) void bq_scan_kernel(const uint64_t *__restrict__ rows, const uint64_t *__restrict__ qw, BqScanArgs a)
{
    extern __shared__ uint32_t bq_lds[];
    const int tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const int64_t xb = blockIdx.x / (unsigned)a.tiles;
    const int q0 = tile * QT;
    const int W = a.W;
    const uint64_t *__restrict__ qt = qw + (int64_t)tile * W * QT;
    const int64_t row0 = xb * a.R, row1 = min(a.N, row0 + a.R);
    const int nb = a.D + 1;

    // RANK: which queries of the tile still need ties from this block (block-uniform)
    uint32_t rank_mask = 0;
    if constexpr (MODE == BQ_RANK) {
        for (int t = 0; t < QT; ++t) {
            const int q = q0 + t;
            if (q < a.Q && !a.all_ties[q] && a.tie_prefix[(int64_t)q * a.X + xb] < (uint32_t)a.need[q]) rank_mask |= 1u << t;
        }
        if (rank_mask == 0) return;
    }
    if constexpr (MODE == BQ_HIST) {
        for (int i = threadIdx.x; i < QT * nb; i += blockDim.x) bq_lds[i] = 0;
        __syncthreads();
    }
    if constexpr (MODE == BQ_EMIT) {
        if (threadIdx.x < QT) bq_lds[threadIdx.x] = 0;
        __syncthreads();
    }
    int thr[QT];
    if constexpr (MODE != BQ_HIST) {
        for (int t = 0; t < QT; ++t) thr[t] = (q0 + t < a.Q) ? a.thr[q0 + t] : -1;
    }
    uint32_t running[QT];   // RANK: ties of the query met earlier in this block
    for (int t = 0; t < QT; ++t) running[t] = 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

    for (int64_t base = row0; base < row1; base += blockDim.x) {
        const int64_t r = base + threadIdx.x;
        const bool valid = r < row1;
        const uint64_t *__restrict__ row = rows + (valid ? r : row0) * W;
        uint32_t h[QT];
        for (int t = 0; t < QT; ++t) h[t] = 0;
        for (int w = 0; w < W; ++w) {
            const uint64_t x = row[w];
            const uint64_t *__restrict__ qv = qt + (int64_t)w * QT;
#pragma unroll
            for (int t = 0; t < QT; ++t) h[t] += __popcll(x ^ qv[t]);
        }
        if constexpr (MODE == BQ_HIST) {
            if (valid) {
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    if (q0 + t < a.Q && bq_accepted(a.accept, a.accept_stride, q0 + t, r)) atomicAdd(&bq_lds[t * nb + h[t]], 1u);
            }
        } else if constexpr (MODE == BQ_EMIT) {
            if (valid) {
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    const int q = q0 + t;
                    if ((int)h[t] > thr[t] || !bq_accepted(a.accept, a.accept_stride, q, r)) continue;   // (thr = -1: no query)
                    if ((int)h[t] < thr[t] || a.all_ties[q]) bq_append(a, q, r, h[t]);
                    else atomicAdd(&bq_lds[t], 1u);
                }
            }
        } else {
            __shared__ uint32_t wcnt[QT][4];
            for (int t = 0; t < QT; ++t) {
                if (!((rank_mask >> t) & 1u)) continue;   // block-uniform
                const int q = q0 + t;
                const bool tie = valid && (int)h[t] == thr[t] && bq_accepted(a.accept, a.accept_stride, q, r);
                const uint64_t m = __ballot(tie);
                if (lane == 0) wcnt[t][wave] = (uint32_t)__popcll(m);
                __syncthreads();
                uint32_t off = 0, total = 0;
                for (int v = 0; v < (int)(blockDim.x >> 6); ++v) {
                    off += v < wave ? wcnt[t][v] : 0u;
                    total += wcnt[t][v];
                }
                const uint32_t in_wave = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                const uint32_t rank = a.tie_prefix[(int64_t)q * a.X + xb] + running[t] + off + in_wave;
                if (tie && rank < (uint32_t)a.need[q]) bq_append(a, q, r, h[t]);
                running[t] += total;
                __syncthreads();
            }
        }
    }

    if constexpr (MODE == BQ_HIST) {
        __syncthreads();
        for (int i = threadIdx.x; i < QT * nb; i += blockDim.x) {
            const int t = i / nb;
            const uint32_t c = bq_lds[i];
            if (c && q0 + t < a.Q) atomicAdd(&a.hist[(int64_t)(q0 + t) * nb + (i - t * nb)], c);
        }
    }
    if constexpr (MODE == BQ_EMIT) {
        __syncthreads();
        if (threadIdx.x < QT && q0 + (int)threadIdx.x < a.Q) a.tiec[(int64_t)(q0 + threadIdx.x) * a.X + xb] = bq_lds[threadIdx.x];
    }
}

// one thread per query: t_q = smallest t with #{h <= t} >= k1 (D + 1 when fewer than k1 rows are accepted: all of them pass)
__global__ void bq_threshold_kernel(BqScanArgs a, int k1)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.Q) return;
    const uint32_t *hq = a.hist + (int64_t)q * (a.D + 1);
    int64_t below = 0;
    int t = 0;
    for (; t <= a.D; ++t) {
        if (below + hq[t] >= (int64_t)k1) break;
        below += hq[t];
    }
    const int64_t ties = t <= a.D ? (int64_t)hq[t] : 0;
    a.thr[q] = t;
    a.need[q] = (int)((int64_t)k1 - below);
    a.all_ties[q] = (below + ties <= (int64_t)a.cap) ? 1 : 0;
    a.cand_cnt[q] = 0;
}

// one thread per query whose ties did not fit: exclusive prefix of the per-block tie counts (block order = id order)
__global__ void bq_tie_prefix_kernel(BqScanArgs a)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.Q || a.all_ties[q]) return;
    uint32_t run = 0;
    for (int64_t xb = 0; xb < a.X; ++xb) {
        a.tie_prefix[(int64_t)q * a.X + xb] = run;
        run += a.tiec[(int64_t)q * a.X + xb];
    }
}

template <int QT>
static int launch_scan_qt(hipStream_t s, const uint64_t *rows, const uint64_t *qw, const BqScanArgs &a, int mode)
{
    const dim3 grid((unsigned)(a.tiles * a.X)), block(256);
    if (mode == BQ_HIST)
        hipLaunchKernelGGL((bq_scan_kernel<QT, BQ_HIST>), grid, block, sizeof(uint32_t) * QT * (a.D + 1), s, rows, qw, a);
    else if (mode == BQ_EMIT)
        hipLaunchKernelGGL((bq_scan_kernel<QT, BQ_EMIT>), grid, block, sizeof(uint32_t) * QT, s, rows, qw, a);
    else
        hipLaunchKernelGGL((bq_scan_kernel<QT, BQ_RANK>), grid, block, 0, s, rows, qw, a);
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

int launch_bq_scan(hipStream_t s, const uint64_t *d_rows, const uint64_t *d_qw, const BqScanArgs &a, int qt, int mode)
{
    switch (qt) {
    case 1: return launch_scan_qt<1>(s, d_rows, d_qw, a, mode);
    case 8: return launch_scan_qt<8>(s, d_rows, d_qw, a, mode);
    case 16: return launch_scan_qt<16>(s, d_rows, d_qw, a, mode);
    case 32: return launch_scan_qt<32>(s, d_rows, d_qw, a, mode);
    default: set_error("bq scan: no kernel for a tile of %d queries", qt); return JV_ERR_INVALID;
    }
}

int launch_bq_select(hipStream_t s, const uint64_t *d_rows, const uint64_t *d_qw, const BqScanArgs &a, int qt, int k1)
{
    JV_TRY(launch_bq_scan(s, d_rows, d_qw, a, qt, BQ_HIST));
    hipLaunchKernelGGL(bq_threshold_kernel, dim3((unsigned)((a.Q + 63) / 64)), dim3(64), 0, s, a, k1);
    JV_HIP_CHECK(hipGetLastError());
    JV_TRY(launch_bq_scan(s, d_rows, d_qw, a, qt, BQ_EMIT));
    hipLaunchKernelGGL(bq_tie_prefix_kernel, dim3((unsigned)((a.Q + 63) / 64)), dim3(64), 0, s, a);
    JV_HIP_CHECK(hipGetLastError());
    return launch_bq_scan(s, d_rows, d_qw, a, qt, BQ_RANK);
}

}  // namespace jv
