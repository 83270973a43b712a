// k_exact_flat.hip — the kernels of the exact flat search (include/jvector_exact_flat.h, host driver exact_flat.cpp), for gfx950:
// exact_dense_kernel's MFMA tile with an epilogue that SELECTS instead of storing.
//
// Why: brute force over float rows used to be exact_dense_kernel into a Q x chunk score matrix and a top-k that reads it back: every
// score crosses HBM twice, the matrix is gigabytes, and an accept filter has no place in it.  The tile kernel already holds each
// 128 x 128 block of finished scores in accumulator registers; what a top-k needs of them is the few that reach the query's
// kc-th best.  So, as in the flat PQ search: a SAMPLE pass scores every g-th row tile into a small Q x S matrix whose kc-th best
// per query is a threshold tau[q] that at least kc accepted rows reach by construction, and a SELECT pass scores every tile and
// keeps (id, score) only where !(score < tau[q]) on an accepted row.  Both are exact_select_kernel, one body, two epilogues.
//
//   * Tile and pipeline are ed_tile's (ed_body.h), restated here so that exact_dense_kernel's code object stays what it is: four
//     wavefronts, 128 queries x 128 rows, K staged K-major through LDS 32 columns at a time by ed_load_chunk, the next chunk's
//     global loads in flight under the 64 v_mfma_f32_32x32x2_f32 of the current one, the operands of step s + 1 read before the
//     MFMAs of step s, ed_block_to_tile's XCD-aware map.  The chains run in the same order, ed_finish is the same function: the
//     scores are exact_dense_kernel's bit for bit.
//   * Tile stride: block b works on row tile tile_offset + b * tile_stride.  The sample pass is the kernel at stride g; the
//     select pass is stride 1.
//   * A shared mask: the two 64-bit accept words of the block's 128 rows are block-uniform.  Both zero: the block returns before
//     any load (the sample epilogue first writes its -INFINITY cells).  Otherwise a lane keeps the bits of its four rows.
//     Per-query masks are read per (query, row), in the select epilogue only by the lanes that passed the threshold.
//   * Select epilogue.  In the C layout a half-wavefront at a fixed accumulator register holds 32 rows of ONE query, the two
//     halves two queries.  A lane tests !(score < tau) — equality passes, so every tie at the threshold is kept; a NaN on either
//     side passes and is left to the list's top-k, as in the composition — then the bounds, and only where that passed the accept
//     bit.  One ballot per register; zero (the common case behind a good threshold) costs nothing more.  Otherwise lane 0 of a
//     half reserves popcount positions in cand_count[q] with one atomic add and every surviving lane writes (id, score) at its
//     prefix position if that lies below the capacity.  The atomic decides a position in a list that feeds a top-k over unique
//     keys: never a result.  tau of the tile's 128 queries is read from LDS, loaded once per block.
// This file is a library of its own, jvector_amd/libjvector_hip_xf.so, which libjvector_hip.so links: it uses nothing of the engine
// but the status codes, and its launchers are its whole interface (xf_params.h holds their parameters, exact_flat.cpp declares them).
// A launcher sets no error text — the caller does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"
#include "gs_wave_hip.h"
#include "ed_body.h"
#include "xf_params.h"

#define XF_EXPORT __attribute__((visibility("default")))
#define XF_LAUNCHED()                                           \
    do {                                                        \
        if (hipGetLastError() != hipSuccess) return JV_ERR_HIP; \
    } while (0)

namespace jv {

static_assert(ED_TN == XF_TILE && ED_TQ == XF_TILE, "xf_params.h restates the tile of ed_body.h");
constexpr int XF_LDS_FLOATS = ED_LDS_FLOATS + ED_TQ;   // ed_tile's staging and norms, then tau of the tile's queries

// word w of a shared mask as the kernel sees it: nothing at and beyond n, nothing past the last word
GS_FN uint64_t xf_word(const uint64_t *bits, int64_t n, int64_t w)
{
    if (w * 64 >= n) return 0ull;
    uint64_t v = bits[w];
    const int64_t left = n - w * 64;
    if (left < 64) v &= (1ull << left) - 1ull;
    return v;
}

// row tile `tile` x queries q0 .. q0 + 128; sample column block b_tile.  lds: XF_LDS_FLOATS floats.  Runs on ED_THREADS threads.
template <int VSF, bool SELECT>
GS_FN void xf_tile(const XfParams &xp, int64_t b_tile, int q0, float *lds)
{
    const int tid = gs_tid();
    const int wave = tid >> 6, lane = tid & 63;
    const int lo = lane & 31, hi = lane >> 5;
    const int64_t n0 = (xp.tile_offset + b_tile * xp.tile_stride) * ED_TN;
    const bool shared = xp.bits != nullptr && xp.stride_words == 0, perq = xp.bits != nullptr && xp.stride_words != 0;

    // ---- a shared mask: the block's two accept words ----
    uint64_t w0 = ~0ull, w1 = ~0ull;
    if (shared) {
        w0 = xf_word(xp.bits, xp.n, n0 >> 6);
        w1 = xf_word(xp.bits, xp.n, (n0 >> 6) + 1);
        if ((w0 | w1) == 0ull) {   // block-uniform: nothing of these 128 rows can be returned
            if (!SELECT)
                for (int c = tid; c < ED_TQ * ED_TN; c += ED_THREADS) {
                    const int q = q0 + (c >> 7);
                    if (q < xp.Q) xp.samp[(int64_t)q * xp.S + b_tile * ED_TN + (c & 127)] = -INFINITY;
                }
            return;
        }
    }
    // bit t: this lane's row 32 t + lo of the tile under the shared mask (all set without one)
    const unsigned acc4 = (unsigned)((w0 >> lo) & 1ull) | (unsigned)((w0 >> (32 + lo)) & 1ull) << 1 | (unsigned)((w1 >> lo) & 1ull) << 2 |
                          (unsigned)((w1 >> (32 + lo)) & 1ull) << 3;

    const EdParams p{xp.vecs, xp.queries, nullptr, 0, xp.n, xp.D, xp.Q};
    float *As = lds, *Bs = As + ED_KB * ED_LDW, *qn = Bs + ED_KB * ED_LDW, *vn = qn + ED_TQ, *tau_s = lds + ED_LDS_FLOATS;
    const bool vec4 = (p.D & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.vecs) | reinterpret_cast<uintptr_t>(p.queries)) & 15) == 0;
    const bool wave_active = q0 + 32 * wave < p.Q;  // wave-uniform
    gs_f32x16 acc[4] = {};
    float nrm = 0.0f;  // threads 0..127: |v|^2 of tile row tid; threads 128..255: |q|^2 of tile row tid - 128
    ed_f4 ra[4], rb[4];
    ed_load_chunk(p, n0, q0, 0, tid, vec4, ra, rb);
    if (SELECT && tid < ED_TQ) tau_s[tid] = q0 + tid < xp.Q ? xp.tau[(int64_t)(q0 + tid) * xp.tau_stride] : INFINITY;

    // ---- the K loop of ed_tile, statement for statement: the same chains in the same order ----
    for (int kb = 0; kb < p.D; kb += ED_KB) {
        {
            const int r0 = tid >> 3, kq = 4 * (tid & 7);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = r0 + 32 * i;
                As[(kq + 0) * ED_LDW + row] = ra[i].x;
                As[(kq + 1) * ED_LDW + row] = ra[i].y;
                As[(kq + 2) * ED_LDW + row] = ra[i].z;
                As[(kq + 3) * ED_LDW + row] = ra[i].w;
                Bs[(kq + 0) * ED_LDW + row] = rb[i].x;
                Bs[(kq + 1) * ED_LDW + row] = rb[i].y;
                Bs[(kq + 2) * ED_LDW + row] = rb[i].z;
                Bs[(kq + 3) * ED_LDW + row] = rb[i].w;
            }
        }
        gs_block_barrier();
        if (kb + ED_KB < p.D) ed_load_chunk(p, n0, q0, kb + ED_KB, tid, vec4, ra, rb);  // prefetch: consumed after the MFMAs
        if (VSF != 1 /* not DOT: the norms, k ascending */) {
            const float *src = (tid < ED_TN) ? Bs + tid : As + (tid - ED_TN);
#pragma unroll 8
            for (int c = 0; c < ED_KB; ++c) {
                const float x = src[c * ED_LDW];
                nrm = gs_fmaf(x, x, nrm);
            }
        }
        const float *a_col = As + 32 * wave + lo + hi * ED_LDW;   // k = 2 s + hi
        const float *b_col = Bs + lo + hi * ED_LDW;
        if (wave_active) {
            float a_cur = a_col[0], b_cur[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) b_cur[t] = b_col[32 * t];
#pragma unroll
            for (int s = 0; s < ED_KB / 2; ++s) {
                float a_nxt = 0.0f, b_nxt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (s + 1 < ED_KB / 2) {
                    a_nxt = a_col[(2 * s + 2) * ED_LDW];
#pragma unroll
                    for (int t = 0; t < 4; ++t) b_nxt[t] = b_col[(2 * s + 2) * ED_LDW + 32 * t];
                }
                gs_sched_fence();
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = gs_mfma_32x32x2(a_cur, b_cur[t], acc[t]);
                gs_sched_fence();
                a_cur = a_nxt;
#pragma unroll
                for (int t = 0; t < 4; ++t) b_cur[t] = b_nxt[t];
            }
        }
        gs_block_barrier();
    }

    if (VSF != 1) {
        if (tid < ED_TN) vn[tid] = nrm;
        else qn[tid - ED_TN] = nrm;
    }
    gs_block_barrier();   // the norms and tau
    // ---- C/D layout: col = lane & 31 (a row of the tile), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (a query) ----
    if (!wave_active) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = 32 * t + lo;
        const int64_t n = n0 + j;
        const bool row_ok = n < xp.n && ((acc4 >> t) & 1u);   // in bounds and accepted by the shared mask
        const float vnj = VSF != 1 ? vn[j] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const int q = q0 + i;
            const float score = ed_finish<VSF>(acc[t][r], VSF != 1 ? qn[i] : 0.0f, vnj);
            if (!SELECT) {
                if (q < xp.Q) {
                    bool ok = row_ok;
                    if (ok && perq) ok = (xp.bits[(int64_t)q * xp.stride_words + (n >> 6)] >> (n & 63)) & 1ull;
                    xp.samp[(int64_t)q * xp.S + b_tile * ED_TN + j] = ok ? score : -INFINITY;
                }
            } else {
                bool pass = !(score < tau_s[i]);
                pass = pass && row_ok && q < xp.Q;
                if (pass && perq) pass = (xp.bits[(int64_t)q * xp.stride_words + (n >> 6)] >> (n & 63)) & 1ull;
                const unsigned long long b = __ballot(pass);
                if (b != 0ull) {   // wave-uniform
                    const unsigned half = (unsigned)(b >> (32 * hi));   // the survivors of this half's query
                    const unsigned cnt = (unsigned)__popc(half);
                    unsigned base = 0u;
                    if (lo == 0 && cnt != 0u) base = atomicAdd(xp.cand_count + q, cnt);   // cnt != 0 implies q < Q
                    base = (unsigned)__shfl((int)base, 32 * hi);
                    const unsigned pos = base + (unsigned)__popc(half & ((1u << lo) - 1u));
                    if (pass && pos < (unsigned)xp.cap) {
                        xp.cand_ids[(int64_t)q * xp.cap + pos] = (int32_t)n;
                        xp.cand_scores[(int64_t)q * xp.cap + pos] = score;
                    }
                }
            }
        }
    }
}

// Three waves per SIMD, as exact_dense_kernel's measured default: the staging registers are dead by the epilogue, which lives in the
// accumulators' shadow.
template <int VSF, bool SELECT>
__global__ __launch_bounds__(ED_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void exact_select_kernel(XfParams p, int64_t blocks_padded,
                                                                                                             int q_tiles)
{
    __shared__ float lds[XF_LDS_FLOATS];
    int64_t b_tile;
    int q_tile;
    if (!ed_block_to_tile((int64_t)blockIdx.x, blocks_padded, p.tiles, q_tiles, &b_tile, &q_tile)) return;
    xf_tile<VSF, SELECT>(p, b_tile, q_tile * ED_TQ, lds);
}

// select != 0: the select epilogue, else the sample epilogue.  The tiles must lie inside the rows: tile_offset + (tiles - 1) *
// tile_stride < ceil(n / 128).
XF_EXPORT int launch_exact_select(hipStream_t s, const XfParams &p, size_t p_bytes, int vsf, int select)
{
    if (p_bytes != sizeof(XfParams) || vsf < 0 || vsf > 2 || p.D < 1 || p.tile_stride < 1 || p.tile_offset < 0) return JV_ERR_INVALID;
    if (p.Q == 0 || p.tiles == 0) return JV_OK;
    if ((p.tile_offset + (p.tiles - 1) * p.tile_stride) * ED_TN >= p.n) return JV_ERR_INVALID;
    if (select ? (!p.tau || !p.cand_ids || !p.cand_scores || !p.cand_count || p.cap < 1) : (!p.samp || p.S != p.tiles * ED_TN)) return JV_ERR_INVALID;
    const int q_tiles = (p.Q + ED_TQ - 1) / ED_TQ;
    const int64_t blocks_padded = (p.tiles * q_tiles + 7) / 8 * 8;
    if (blocks_padded > 0x7fffffffLL) return JV_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)blocks_padded), block(ED_THREADS);
#define XF_LAUNCH(SEL)                                                                                                   \
    switch (vsf) {                                                                                                       \
    case 0: hipLaunchKernelGGL((exact_select_kernel<0, SEL>), grid, block, 0, s, p, blocks_padded, q_tiles); break;     \
    case 1: hipLaunchKernelGGL((exact_select_kernel<1, SEL>), grid, block, 0, s, p, blocks_padded, q_tiles); break;     \
    default: hipLaunchKernelGGL((exact_select_kernel<2, SEL>), grid, block, 0, s, p, blocks_padded, q_tiles); break;    \
    }
    if (select) { XF_LAUNCH(true) }
    else { XF_LAUNCH(false) }
#undef XF_LAUNCH
    XF_LAUNCHED();
    return JV_OK;
}

// ids[0 .. cells) = -1, scores[0 .. cells) = -INFINITY (nullable), counts[0 .. Q) = 0 (nullable), *chk = {0, 0} (nullable)
__global__ __launch_bounds__(256) void xf_init_kernel(int32_t *ids, float *scores, int64_t cells, unsigned int *counts, int Q, XfCheck *chk)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cells) {
        ids[i] = -1;
        if (scores) scores[i] = -INFINITY;
    }
    if (counts && i < Q) counts[i] = 0u;
    if (chk && i == 0) *chk = XfCheck{0ull, 0ull};
}

XF_EXPORT int launch_exact_flat_init(hipStream_t s, int32_t *ids, float *scores, int64_t cells, unsigned int *counts, int Q, XfCheck *chk)
{
    const int64_t work = cells > Q ? cells : (Q > 1 ? Q : 1);
    const int64_t blocks = (work + 255) / 256;
    if (blocks > 0x7fffffffLL) return JV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(xf_init_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ids, scores, cells, counts, Q, chk);
    XF_LAUNCHED();
    return JV_OK;
}

// the list-length check: over != 0 when some query's list holds more than cap entries; listed is the sum of the lengths.  Integer
// atomics: the sums do not depend on their order.
__global__ __launch_bounds__(256) void xf_check_kernel(const unsigned int *counts, int Q, int cap, XfCheck *chk)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const unsigned int c = counts[q];
    if (c > (unsigned int)cap) atomicOr(&chk->over, 1ull);
    atomicAdd(&chk->listed, (unsigned long long)c);
}

XF_EXPORT int launch_exact_flat_check(hipStream_t s, const unsigned int *counts, int Q, int cap, XfCheck *chk)
{
    if (Q == 0) return JV_OK;
    hipLaunchKernelGGL(xf_check_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, counts, Q, cap, chk);
    XF_LAUNCHED();
    return JV_OK;
}

// the chunked route under a mask: the ids of a chunk's score columns, -1 where the query rejects the row.  grid (blocks, Q)
__global__ __launch_bounds__(256) void xf_ids_kernel(XfIdsParams p)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= p.count) return;
    const int q = blockIdx.y;
    const int64_t n = p.first + j;
    const bool ok = (p.bits[(int64_t)q * p.stride_words + (n >> 6)] >> (n & 63)) & 1ull;
    p.ids[(int64_t)q * p.count + j] = ok ? (int32_t)n : -1;
}

XF_EXPORT int launch_exact_flat_ids(hipStream_t s, const XfIdsParams &p, size_t p_bytes)
{
    if (p_bytes != sizeof(XfIdsParams) || !p.bits || !p.ids || p.Q > 65535) return JV_ERR_INVALID;
    if (p.Q == 0 || p.count == 0) return JV_OK;
    hipLaunchKernelGGL(xf_ids_kernel, dim3((unsigned)((p.count + 255) / 256), (unsigned)p.Q), dim3(256), 0, s, p);
    XF_LAUNCHED();
    return JV_OK;
}

}  // namespace jv
