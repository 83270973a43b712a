// k_flat_mask.hip — the dense route of the flat PQ search under an accept filter (flat_accept.cpp), for gfx950: a threshold scan over
// ALL n rows that reads the accept bits itself, and the kernel that takes the rejected rows out of the threshold's sample.
//
// Why: the list route (k_flat_accept.hip) scores every accepted row into a Q x L matrix and runs a top-k over it — right for a
// selective predicate, 3 to 7 times the unfiltered search for a mask that accepts most rows.  The unfiltered search never writes
// scores: a strided sample gives each query a threshold, one scan appends the rows that reach it to a short list.  This is that scan
// (the FILTER form of adc_mq_kernel, k_adc_mq.hip) under a mask:
//   * a tile starts at a multiple of 64 rows and lane t of a wavefront owns row base + t, so the 64 rows a wavefront handles for one
//     r are exactly ONE 64-bit accept word.  The word's address is wave-uniform: it is fetched by a scalar load (one word per r for a
//     shared mask, the four queries' words for per-query masks), and a lane's bit for query j is (word_j >> lane) & 1.  The lane
//     keeps its R x 4 bits in one register.
//   * a wavefront whose words are all zero issues neither the code loads nor the LDS look-ups of that r (a scalar branch: clustered
//     predicates skip whole runs of rows); a lane whose row no query of the group accepts skips its own.
//   * the sums are one f32 chain per (query, row) in ascending m, as in adc_mq_kernel: bit-identical to it and to the scalar reference.
//   * in the epilogue a (query, row) pair is tested only if its own bit is set: the conservative sure-reject cut, the similarity
//     transform, score >= tau[q].  Survivors are staged per workgroup in the LDS the table slices no longer need and handed to the
//     query's global list with one reservation per (workgroup, query).  The list's order is immaterial: it feeds a top-k.
// Bits at and beyond n count as clear and no word past ceil(n / 64) of a mask is read.
//
// This file is a library of its own, jvector_amd/libjvector_hip_fm.so, which libjvector_hip.so links: it uses nothing of the engine
// but the status codes and jv_device.h, and its two launchers are its whole interface (fm_params.h holds their parameters,
// flat_accept.cpp declares them).  A launcher sets no error text — the caller does.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"
#include "fm_params.h"
#include "jv_device.h"

#define FM_EXPORT __attribute__((visibility("default")))
#define FM_LAUNCHED()                                           \
    do {                                                        \
        if (hipGetLastError() != hipSuccess) return JV_ERR_HIP; \
    } while (0)

namespace jv {

constexpr int FM_GRID_Y = 32768;   // tiles per launch (grid.y holds 65535)

// word w of mask m as the scan sees it: nothing at and beyond n, nothing past the last word
__device__ __forceinline__ uint64_t fm_word(const uint64_t *bits, int64_t stride_words, int64_t n, int64_t m, int64_t w)
{
    if (w * 64 >= n) return 0ull;
    uint64_t v = bits[m * stride_words + w];
    const int64_t left = n - w * 64;
    if (left < 64) v &= (1ull << left) - 1ull;
    return v;
}

template <int VSF, int SLCH, int R, bool PERQ>
__global__ __launch_bounds__(FM_THREADS) void adc_mq_mask_kernel(FmScanParams p, int tile0)
{
    constexpr int P = FM_P;
    constexpr int SL = 16 * SLCH;  // subspaces per LDS slice
    extern __shared__ __attribute__((aligned(16))) float4 fm_lds4[];  // [SL*256]

    const int q0 = blockIdx.x * P;
    const int64_t tile_base = ((int64_t)tile0 + blockIdx.y) * (FM_THREADS * R);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nslices = p.M / SL;

    // the accept bits: word (tile_base / 64 + 16 r + wave) of each query's mask covers this wavefront's rows of step r
    uint32_t abits = 0;  // nibble r: this lane's row of step r under the four queries
    uint32_t live = 0;   // wave-uniform, bit r: some query accepts some row of the wavefront's step r
#pragma unroll 1   // (unrolled, the 4 R words in flight at once push scalar registers out to vector lanes)
    for (int r = 0; r < R; ++r) {
        const int64_t w = (tile_base >> 6) + r * (FM_THREADS / 64) + wave;
        uint64_t wq[P];
        if (PERQ) {
#pragma unroll
            for (int j = 0; j < P; ++j) wq[j] = q0 + j < p.Q ? fm_word(p.bits, p.stride_words, p.n, q0 + j, w) : 0ull;
        } else {
            const uint64_t v = fm_word(p.bits, 0, p.n, 0, w);
#pragma unroll
            for (int j = 0; j < P; ++j) wq[j] = q0 + j < p.Q ? v : 0ull;
        }
        uint64_t any = 0ull;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            abits |= (uint32_t)((wq[j] >> lane) & 1ull) << (4 * r + j);
            any |= wq[j];
        }
        live |= (any != 0ull ? 1u : 0u) << r;
    }

    float acc[R][P];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < P; ++j) acc[r][j] = 0.0f;

    // per-query table bases (queries past Q read query Q-1's table; their results are discarded)
    const float *lq[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        int q = q0 + j < p.Q ? q0 + j : p.Q - 1;
        lq[j] = p.luts + (int64_t)q * p.M * FM_CLUSTERS;
    }

    for (int s = 0; s < nslices; ++s) {
        __syncthreads();  // readers of the previous slice are done
        const int mb = s * SL;
        for (int idx = tid; idx < SL * FM_CLUSTERS; idx += FM_THREADS) {
            const int off = mb * FM_CLUSTERS + idx;
            fm_lds4[idx] = make_float4(lq[0][off], lq[1][off], lq[2][off], lq[3][off]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (((live >> r) & 1u) == 0u) continue;          // the whole word is clear: a scalar branch
            if (((abits >> (4 * r)) & 15u) == 0u) continue;  // nobody wants this lane's row (rows at and beyond n among them)
            const int64_t row = tile_base + (int64_t)r * FM_THREADS + tid;
            const uint4 *rp = reinterpret_cast<const uint4 *>(p.codes + row * p.M + mb);
            uint4 w[SLCH];
#pragma unroll
            for (int c = 0; c < SLCH; ++c) w[c] = rp[c];
#pragma unroll
            for (int c = 0; c < SLCH; ++c) {
                const uint32_t d[4] = {w[c].x, w[c].y, w[c].z, w[c].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int m = c * 16 + e * 4 + b;
                        const uint32_t code = (d[e] >> (8 * b)) & 0xFFu;
                        const float4 t = fm_lds4[m * FM_CLUSTERS + code];
                        acc[r][0] += t.x;
                        acc[r][1] += t.y;
                        acc[r][2] += t.z;
                        acc[r][3] += t.w;
                    }
                }
            }
        }
    }

    // epilogue: adc_mq_kernel's, entered by the accepted (query, row) pairs only
    constexpr int STAGE = (SL * FM_CLUSTERS * (int)sizeof(float4)) / (P * 8);  // (id, score) pairs per query
    __shared__ unsigned int s_cnt[P], s_base[P];
    int32_t *st_ids = reinterpret_cast<int32_t *>(fm_lds4);
    float *st_sc = reinterpret_cast<float *>(fm_lds4) + (size_t)P * STAGE;
    const bool staged = p.staged != 0;
    if (staged) {
        __syncthreads();  // every lane is done with the last table slice
        if (tid < P) s_cnt[tid] = 0u;
        __syncthreads();
    }
    // the thresholds and the sure-reject bounds of the four queries, once per lane.  tau = -inf (an accepted sample below k_s rows)
    // leaves every cut at "never rejects": every accepted row passes.
    float tq[P], cut[P], bm[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        cut[j] = (VSF == VSF_L2) ? __builtin_inff() : -__builtin_inff();   // never rejects
        bm[j] = 0.0f;
        tq[j] = __builtin_inff();
        if (q0 + j < p.Q) {
            tq[j] = p.tau[(int64_t)(q0 + j) * p.tau_stride];
            if (VSF == VSF_L2) {
                if (tq[j] > 1e-6f) cut[j] = (1.0f / tq[j] - 1.0f) * 1.000002f + 4e-6f;
            } else if (VSF == VSF_DOT) {
                cut[j] = (2.0f * tq[j] - 1.0f) - 4e-6f * (fabsf(2.0f * tq[j] - 1.0f) + 1.0f);
            } else {
                cut[j] = 2.0f * tq[j] - 1.0f;
                bm[j] = p.bmag[q0 + j];
            }
            if (!(cut[j] == cut[j])) cut[j] = (VSF == VSF_L2) ? __builtin_inff() : -__builtin_inff();
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t nib = (abits >> (4 * r)) & 15u;
        if (nib == 0u) continue;
        const int64_t row = tile_base + (int64_t)r * FM_THREADS + tid;
        const float nrm = (VSF == VSF_COS) ? p.norms[row] : 0.0f;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            if (((nib >> j) & 1u) == 0u) continue;   // (a set bit: q0 + j < Q and row < n)
            const int q = q0 + j;
            // the cheap sure-reject before the similarity transform (adc_mq_kernel: conservative by a relative 2e-6 / absolute 4e-6,
            // orders of magnitude above the transform's rounding, so it only drops pairs the exact comparison below drops too)
            const float raw = acc[r][j];
            bool sure_fail;
            if (VSF == VSF_L2) sure_fail = raw > cut[j];                                          // 1 / (1 + raw) < tau
            else if (VSF == VSF_DOT) sure_fail = raw < cut[j];                                     // (1 + raw) / 2 < tau
            else {
                const float prod = nrm * bm[j];
                const float c = raw * __builtin_amdgcn_rsqf(prod);                                  // ~cosine, few ulps
                sure_fail = prod > 1e-30f && prod < 1e30f && c < cut[j] - 8e-6f * (fabsf(c) + 1.0f);
            }
            if (sure_fail) continue;
            float sc;
            if (VSF == VSF_COS) sc = score_from_raw(VSF_COS, cosine_finish(raw, nrm, bm[j]));
            else sc = score_from_raw(VSF, raw);
            if (sc >= tq[j]) {
                const unsigned int sp = staged ? atomicAdd(&s_cnt[j], 1u) : (unsigned int)STAGE;
                if (sp < (unsigned int)STAGE) {
                    st_ids[j * STAGE + sp] = (int32_t)row;
                    st_sc[j * STAGE + sp] = sc;
                } else {  // staging area full (or off): straight to the global list
                    const unsigned int pos = atomicAdd(&p.cand_count[q], 1u);
                    if (pos < (unsigned int)p.cap) {
                        p.cand_ids[(int64_t)q * p.cap + pos] = (int32_t)row;
                        p.cand_scores[(int64_t)q * p.cap + pos] = sc;
                    }
                }
            }
        }
    }
    if (staged) {
        __syncthreads();
        if (tid < P && q0 + tid < p.Q) {
            const unsigned int n = s_cnt[tid] < (unsigned int)STAGE ? s_cnt[tid] : (unsigned int)STAGE;
            s_base[tid] = n ? atomicAdd(&p.cand_count[q0 + tid], n) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int q = q0 + j;
            if (q >= p.Q) continue;
            const unsigned int n = s_cnt[j] < (unsigned int)STAGE ? s_cnt[j] : (unsigned int)STAGE, base = s_base[j];
            for (unsigned int t = tid; t < n; t += FM_THREADS) {
                const unsigned int pos = base + t;
                if (pos < (unsigned int)p.cap) {
                    p.cand_ids[(int64_t)q * p.cap + pos] = st_ids[j * STAGE + t];
                    p.cand_scores[(int64_t)q * p.cap + pos] = st_sc[j * STAGE + t];
                }
            }
        }
    }
}

// samp[q][i] = -INFINITY where bit i * stride of query q's mask is clear: what is left is a uniform 1 / stride sample of the accepted rows
__global__ __launch_bounds__(256) void flat_mask_sample_kernel(FmSampleParams p)
{
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= (int64_t)p.Q * p.S) return;
    const int64_t q = cell / p.S, i = cell - q * p.S;
    const int64_t row = i * p.stride;
    const uint64_t w = fm_word(p.bits, p.stride_words, p.n, p.stride_words ? q : 0, row >> 6);
    if (((w >> (row & 63)) & 1ull) == 0ull) p.samp[cell] = -__builtin_inff();
}

// the instantiations that are built: all but the cosine's R = 8 over two-chunk slices (SLCH = 2), where the 32 sums, two 16-byte code
// words and the double-precision finish together pass the 128 registers a 1024-thread workgroup allows (8 registers spilled, 36 bytes
// of scratch per lane): the launcher takes R = 4 there.  The list kernel leaves its cosine R = 8 out for the same reason.
template <int VSF, int SLCH, int R>
constexpr bool fm_built()
{
    return R == 4 || !(VSF == VSF_COS && SLCH == 2);
}

template <int VSF, int SLCH, int R, bool PERQ>
static int launch_scan_one(hipStream_t s, const FmScanParams &p0)
{
    if constexpr (!fm_built<VSF, SLCH, R>()) {
        return launch_scan_one<VSF, SLCH, 4, PERQ>(s, p0);
    } else {
        FmScanParams p = p0;
        const size_t lds = fm_scan_lds_bytes(SLCH);
        auto kfn = adc_mq_mask_kernel<VSF, SLCH, R, PERQ>;
        if (hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return JV_ERR_HIP;
        }
        // expected survivors per (workgroup, query): the threshold aims at cap / 4 per query over n rows (adc_mq_kernel's rule)
        p.staged = (double)p.cap / 4.0 * (double)(FM_THREADS * R) / (double)p.n >= 16.0 ? 1 : 0;
        const int64_t tiles = (p.n + FM_THREADS * R - 1) / (FM_THREADS * R);
        for (int64_t t0 = 0; t0 < tiles; t0 += FM_GRID_Y) {
            const int64_t ny = tiles - t0 < FM_GRID_Y ? tiles - t0 : FM_GRID_Y;
            hipLaunchKernelGGL(kfn, dim3((unsigned)((p.Q + FM_P - 1) / FM_P), (unsigned)ny), dim3(FM_THREADS), lds, s, p, (int)t0);
            FM_LAUNCHED();
        }
        return JV_OK;
    }
}

template <int VSF, int SLCH>
static int launch_scan_rp(hipStream_t s, const FmScanParams &p, int R)
{
    const bool perq = p.stride_words != 0;
    if (R >= 8) return perq ? launch_scan_one<VSF, SLCH, 8, true>(s, p) : launch_scan_one<VSF, SLCH, 8, false>(s, p);
    return perq ? launch_scan_one<VSF, SLCH, 4, true>(s, p) : launch_scan_one<VSF, SLCH, 4, false>(s, p);
}

template <int VSF>
static int launch_scan_slch(hipStream_t s, const FmScanParams &p, int R)
{
    if (p.M % 32 == 0) return launch_scan_rp<VSF, 2>(s, p, R);
    return launch_scan_rp<VSF, 1>(s, p, R);
}

// the threshold scan; vsf: the kernel numbering (0 EUCLIDEAN, 1 DOT_PRODUCT, 2 COSINE); rows_per_lane: 4, 8 or 0 (the launcher chooses)
FM_EXPORT int launch_flat_mask_scan(hipStream_t s, const FmScanParams &p, size_t p_bytes, int vsf, int rows_per_lane, int num_cus)
{
    if (p_bytes != sizeof(FmScanParams)) return JV_ERR_INVALID;
    if (p.Q == 0) return JV_OK;
    if (p.Q < 0 || p.Q > 4 * 65535 || p.n < 1 || p.n > 0x7fffffffLL || p.M < 16 || p.M % 16 != 0 || !p.luts || !p.codes || !p.bits || !p.tau ||
        !p.cand_ids || !p.cand_scores || !p.cand_count || p.cap < 1 || p.tau_stride < 1 || p.stride_words < 0 ||
        (p.stride_words != 0 && p.stride_words < (p.n + 63) / 64) || (reinterpret_cast<uintptr_t>(p.codes) & 15) != 0 || vsf < 0 || vsf > 2 ||
        (vsf == 2 && (!p.bmag || !p.norms)) || (rows_per_lane != 0 && rows_per_lane != 4 && rows_per_lane != 8))
        return JV_ERR_INVALID;
    // rows per lane: amortise the per-slice table refill, but keep >= ~2 workgroups per CU in the grid
    int R = rows_per_lane;
    if (R == 0) {
        const int64_t groups = (p.Q + FM_P - 1) / FM_P;
        R = groups * ((p.n + FM_THREADS * 8 - 1) / (FM_THREADS * 8)) >= 2 * (int64_t)num_cus ? 8 : 4;
    }
    switch (vsf) {
    case 0: return launch_scan_slch<VSF_L2>(s, p, R);
    case 1: return launch_scan_slch<VSF_DOT>(s, p, R);
    default: return launch_scan_slch<VSF_COS>(s, p, R);
    }
}

FM_EXPORT int launch_flat_mask_sample(hipStream_t s, const FmSampleParams &p, size_t p_bytes)
{
    if (p_bytes != sizeof(FmSampleParams)) return JV_ERR_INVALID;
    if (p.Q == 0 || p.S == 0) return JV_OK;
    const int64_t cells = (int64_t)p.Q * p.S;
    if (p.Q < 0 || p.S < 0 || p.stride < 1 || p.n < 1 || (p.S - 1) * p.stride >= p.n || !p.samp || !p.bits || p.stride_words < 0 ||
        (p.stride_words != 0 && p.stride_words < (p.n + 63) / 64) || (cells + 255) / 256 > 0x7fffffffLL)
        return JV_ERR_INVALID;
    hipLaunchKernelGGL(flat_mask_sample_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, p);
    FM_LAUNCHED();
    return JV_OK;
}

}  // namespace jv
