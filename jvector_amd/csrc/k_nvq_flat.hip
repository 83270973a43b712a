// k_nvq_flat.hip — the kernel of the NVQ flat search (include/jvector_nvq_flat.h, host driver nvq_flat.cpp), for gfx950: ed_tile's MFMA
// tile over NVQ rows that are de-quantised ONCE per tile, with exact_select_kernel's two epilogues.
//
// Why: the only way to score every NVQ row used to be the gather kernel (k_nvq.hip) over all ordinals, which de-quantises a byte once
// per (query, row, dimension) — ~26 VALU instructions each, the whole cost of that kernel.  The de-quantised value depends on the row,
// never on the query: a 128 x 128 tile decodes a row chunk once and uses it for 128 queries through MFMA, and the rows cross HBM at one
// byte per dimension.
//
//   * Tile, pipeline, block map: ed_tile's (ed_body.h).  Four wavefronts, 128 queries x 128 rows, wavefront w owns queries 32 w .. + 31
//     against all 128 rows (4 accumulators of 32x32), operands K-major in LDS at [k * 129 + row], the operands of step s + 1 read before
//     the MFMAs of step s, the next chunk's global loads in flight under the current chunk's MFMAs, ed_block_to_tile.
//   * Staging of the B tile.  A chunk is KB = ED_KB = 32 dimensions of 128 rows: 4 KB of bytes[row * ld + k], 16 bytes per thread.
//     Thread t owns row t >> 1 of the tile and the half h = t & 1 of the chunk: ONE 16-byte load (rows are 16-byte aligned, ld is a
//     multiple of 16, so a piece never leaves its row), held in four registers while the previous chunk's MFMAs run.  At the top of
//     the next step it decodes the sixteen bytes in registers (nq_scaled_logit's bits; the short division where the row's whole
//     sub-vector passes nq_fast_ok, chosen per lane — both divisions are correctly rounded, so the choice changes no bit) and stores
//     them with sixteen ds_write_b32 at [(16 h + c) * 129 + row].  Banks: 129 = 1 mod 32, so lane l of a 32-lane write group hits bank
//     (16 (l & 1) + c + (l >> 1) + const) mod 32 — l >> 1 runs over 0..15 and l & 1 adds 0 or 16: 32 distinct banks.
//     KB = 32 and not 64: the byte loads are already 16 bytes wide, the float tiles stay ed_tile's 33 KB (four blocks per CU where
//     64 columns would leave two), and the K loop is ed_tile's statement for statement.
//   * Sub-vector parameters.  The boundaries depend on D and S only (base = D / S, the first D % S sub-vectors one longer), so every
//     thread walks them with two integers; the `derived` float4 of (row, sub-vector) is fetched by the thread that decodes the row, and
//     again only when its k range enters the next sub-vector — also in the middle of its sixteen dimensions.
//   * Zeroing.  Dimensions at and beyond D and rows at and beyond n are staged as 0.0f, NOT as the decode of a zero byte (which is
//     not zero): a zero product leaves a chain as it is.
//   * The A tile holds the queries (EUCLIDEAN: query - globalMean, made by nvq_query_prep_kernel), staged as ed_load_chunk stages it.
//   * Scores: dot = one k-ascending fmaf chain from +0 over the whole row (the MFMA chain; NVQScorer restarts its chain at every
//     sub-vector — the one difference, of f32 round-off class).  DOT (1 + dot + qaux[q]) / 2.  EUCLIDEAN ed_finish: |q|^2 and |v|^2
//     are k-ascending fmaf chains over the staged tiles.  COSINE stages val[k] + mean[k] and finishes
//     (1 + (dot / qaux[q]) / (float)sqrt((double)cosnorm[row])) / 2.
//   * Epilogues, tile stride and offset, masks: exact_select_kernel's (k_exact_flat.hip) — the block-uniform skip of a tile whose two
//     accept words are zero before any load, the sample epilogue into a Q x S matrix, the select epilogue with !(score < tau[q]), one
//     ballot per accumulator register, one atomic per half-wavefront and the capacity check.
// This file is a library of its own, jvector_amd/libjvector_hip_nf.so, which libjvector_hip.so links; its launcher is its whole
// interface (nf_params.h holds the parameters, nvq_flat.cpp declares it).  A launcher sets no error text — the caller does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/jvector_hip.h"
#include "gs_wave_hip.h"
#include "ed_body.h"
#include "nq_decode.h"
#include "nf_params.h"

#define NF_EXPORT __attribute__((visibility("default")))

namespace jv {

static_assert(ED_TN == NF_TILE && ED_TQ == NF_TILE, "nf_params.h restates the tile of ed_body.h");
static_assert(ED_THREADS * 16 == ED_TN * ED_KB, "one 16-byte piece per thread covers a chunk of the B tile");
constexpr int NF_LDS_FLOATS = ED_LDS_FLOATS + ED_TQ;   // ed_tile's staging and per-query / per-row scalars, then tau of the tile's queries

// word w of a shared mask as the kernel sees it: nothing at and beyond n, nothing past the last word
GS_FN uint64_t nf_word(const uint64_t *bits, int64_t n, int64_t w)
{
    if (w * 64 >= n) return 0ull;
    uint64_t v = bits[w];
    const int64_t left = n - w * 64;
    if (left < 64) v &= (1ull << left) - 1ull;
    return v;
}

// the A half of ed_load_chunk: thread t fetches columns kb + 4 (t & 7) .. + 3 of query rows (t >> 3) + 32 i (zero beyond D / Q)
GS_FN void nf_load_a(const float *queries, int Q, int D, int q0, int kb, int tid, bool vec4, ed_f4 (&ra)[4])
{
    const int r0 = tid >> 3, k = kb + 4 * (tid & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = r0 + 32 * i;
        ed_f4 a = {0.f, 0.f, 0.f, 0.f};
        if (q0 + row < Q && k < D) {
            const float *src = queries + (int64_t)(q0 + row) * D + k;
            if (vec4) a = *reinterpret_cast<const ed_f4 *>(src);
            else {
                a.x = src[0];
                if (k + 1 < D) a.y = src[1];
                if (k + 2 < D) a.z = src[2];
                if (k + 3 < D) a.w = src[3];
            }
        }
        ra[i] = a;
    }
}

// the de-quantised value of one byte: nq_scaled_logit's bits on either path (nq_elem of k_nvq.hip)
GS_FN float nf_decode(uint32_t byte, const float4 prm, bool fast)
{
    if (fast) {
        const float sv = __builtin_fmaf((float)byte, prm.z, prm.w);
        const int zb = __float_as_int(nq_div_fast(sv, 1.0f - sv));
        const float p = (float)(((zb & 0x7f800000) >> 23) - 128);
        const float m = __int_as_float((zb & 0x007fffff) + 0x3f800000);
        return __builtin_fmaf(m + p, prm.x, prm.y);
    }
    return nq_scaled_logit((float)byte, prm.x, prm.y, prm.z, prm.w);
}

template <int VSF>
GS_FN float nf_finish(float dot, float qx, float vx)
{
    if (VSF == 0 /* L2: qx = |qwork|^2, vx = |val|^2 */) return ed_finish<0>(dot, qx, vx);
    if (VSF == 1 /* DOT: qx = qaux */) return (1.0f + dot + qx) / 2.0f;
    return (1.0f + (dot / qx) / vx) / 2.0f;   // COSINE: qx = qaux, vx = (float)sqrt((double)cosnorm[row])
}

// row tile `tile` x queries q0 .. q0 + 128; sample column block b_tile.  lds: NF_LDS_FLOATS floats.  Runs on ED_THREADS threads.
template <int VSF, bool SELECT>
GS_FN void nf_tile(const NfParams &xp, int64_t b_tile, int q0, float *lds)
{
    const int tid = gs_tid();
    const int wave = tid >> 6, lane = tid & 63;
    const int lo = lane & 31, hi = lane >> 5;
    const int64_t n0 = (xp.tile_offset + b_tile * xp.tile_stride) * ED_TN;
    const bool shared = xp.bits != nullptr && xp.stride_words == 0, perq = xp.bits != nullptr && xp.stride_words != 0;

    // ---- a shared mask: the block's two accept words ----
    uint64_t w0 = ~0ull, w1 = ~0ull;
    if (shared) {
        w0 = nf_word(xp.bits, xp.n, n0 >> 6);
        w1 = nf_word(xp.bits, xp.n, (n0 >> 6) + 1);
        if ((w0 | w1) == 0ull) {   // block-uniform: nothing of these 128 rows can be returned
            if (!SELECT)
                for (int c = tid; c < ED_TQ * ED_TN; c += ED_THREADS) {
                    const int q = q0 + (c >> 7);
                    const int64_t col = b_tile * ED_TN + (c & 127);
                    if (q < xp.Q && col < xp.S) xp.samp[(int64_t)q * xp.S + col] = -INFINITY;
                }
            return;
        }
    }
    // bit t: this lane's row 32 t + lo of the tile under the shared mask (all set without one)
    const unsigned acc4 = (unsigned)((w0 >> lo) & 1ull) | (unsigned)((w0 >> (32 + lo)) & 1ull) << 1 | (unsigned)((w1 >> lo) & 1ull) << 2 |
                          (unsigned)((w1 >> (32 + lo)) & 1ull) << 3;

    const int D = xp.D;
    float *As = lds, *Bs = As + ED_KB * ED_LDW, *qn = Bs + ED_KB * ED_LDW, *vn = qn + ED_TQ, *tau_s = lds + ED_LDS_FLOATS;
    const bool vec4 = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(xp.queries) & 15) == 0;
    const bool wave_active = q0 + 32 * wave < xp.Q;  // wave-uniform
    gs_f32x16 acc[4] = {};
    float nrm = 0.0f;  // EUCLIDEAN.  threads 0..127: |v|^2 of tile row tid; threads 128..255: |q|^2 of tile row tid - 128

    // ---- this thread's part of the B tile: row brow, dimensions kb + bh .. kb + bh + 15 of every chunk ----
    const int brow = tid >> 1, bh = 16 * (tid & 1);
    const bool b_ok = n0 + brow < xp.n;
    const uint8_t *bp = xp.bytes + (b_ok ? (n0 + brow) * xp.ld : 0) + bh;
    const float4 *dp = reinterpret_cast<const float4 *>(xp.derived) + (b_ok ? (n0 + brow) * xp.subs : 0);
    const int base = D / xp.subs, rem = D % xp.subs;
    int sub = 0, sub_end = base + (rem ? 1 : 0), sub_have = -1;   // the sub-vector of the next dimension, its end, the one prm holds
    float4 prm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool fast = false;
    const uint4 zero16 = make_uint4(0u, 0u, 0u, 0u);

    ed_f4 ra[4];
    uint4 rb;
    nf_load_a(xp.queries, xp.Q, D, q0, 0, tid, vec4, ra);
    rb = (b_ok && bh < xp.ld) ? *reinterpret_cast<const uint4 *>(bp) : zero16;
    if (SELECT && tid < ED_TQ) tau_s[tid] = q0 + tid < xp.Q ? xp.tau[(int64_t)(q0 + tid) * xp.tau_stride] : INFINITY;

    for (int kb = 0; kb < D; kb += ED_KB) {
        {
            const int r0 = tid >> 3, kq = 4 * (tid & 7);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = r0 + 32 * i;
                As[(kq + 0) * ED_LDW + row] = ra[i].x;
                As[(kq + 1) * ED_LDW + row] = ra[i].y;
                As[(kq + 2) * ED_LDW + row] = ra[i].z;
                As[(kq + 3) * ED_LDW + row] = ra[i].w;
            }
        }
        {   // decode the sixteen bytes in registers and store them K-major
            const int k0 = kb + bh;
            while (sub_end <= k0 && sub + 1 < xp.subs) {   // the sub-vectors that ended inside the other half's dimensions
                ++sub;
                sub_end += base + (sub < rem ? 1 : 0);
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int k = k0 + t;
                if (k == sub_end && sub + 1 < xp.subs) {   // a boundary inside the piece
                    ++sub;
                    sub_end += base + (sub < rem ? 1 : 0);
                }
                float val = 0.0f;   // at and beyond D, at and beyond n: zero, not the decode of a zero byte
                if (b_ok && k < D) {
                    if (sub != sub_have) {
                        prm = dp[sub];
                        fast = nq_fast_ok(prm);
                        sub_have = sub;
                    }
                    const uint32_t w = t < 4 ? rb.x : (t < 8 ? rb.y : (t < 12 ? rb.z : rb.w));   // t is a constant here
                    val = nf_decode((w >> (8 * (t & 3))) & 0xffu, prm, fast);
                    if (VSF == 2) val += xp.mean[k];
                }
                Bs[(bh + t) * ED_LDW + brow] = val;
            }
        }
        gs_block_barrier();
        if (kb + ED_KB < D) {  // prefetch: consumed after the MFMAs
            nf_load_a(xp.queries, xp.Q, D, q0, kb + ED_KB, tid, vec4, ra);
            rb = (b_ok && kb + ED_KB + bh < xp.ld) ? *reinterpret_cast<const uint4 *>(bp + kb + ED_KB) : zero16;
        }
        if (VSF == 0 /* EUCLIDEAN: the norms, k ascending */) {
            const float *src = (tid < ED_TN) ? Bs + tid : As + (tid - ED_TN);
#pragma unroll 8
            for (int c = 0; c < ED_KB; ++c) {
                const float x = src[c * ED_LDW];
                nrm = gs_fmaf(x, x, nrm);
            }
        }
        // ---- the K steps of ed_tile, statement for statement ----
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

    // ---- the scalars of the finish: qn[i] of query i, vn[j] of row j of the tile ----
    if (VSF == 0) {
        if (tid < ED_TN) vn[tid] = nrm;
        else qn[tid - ED_TN] = nrm;
    } else if (tid < ED_TQ) {
        qn[tid] = q0 + tid < xp.Q ? xp.qaux[q0 + tid] : 0.0f;
    } else if (VSF == 2) {
        const int64_t n = n0 + (tid - ED_TQ);
        vn[tid - ED_TQ] = n < xp.n ? (float)sqrt((double)xp.cosnorm[n]) : 1.0f;
    }
    gs_block_barrier();   // the scalars and tau
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
            const float score = nf_finish<VSF>(acc[t][r], qn[i], vnj);
            if (!SELECT) {
                const int64_t col = b_tile * ED_TN + j;
                if (q < xp.Q && col < xp.S) {
                    bool ok = row_ok;
                    if (ok && perq) ok = (xp.bits[(int64_t)q * xp.stride_words + (n >> 6)] >> (n & 63)) & 1ull;
                    xp.samp[(int64_t)q * xp.S + col] = ok ? score : -INFINITY;
                }
            } else {
                bool pass = !(score < tau_s[i]);
                pass = pass && row_ok && q < xp.Q;
                if (pass && perq) pass = (xp.bits[(int64_t)q * xp.stride_words + (n >> 6)] >> (n & 63)) & 1ull;
                const unsigned long long b = __ballot(pass);
                if (b != 0ull) {   // wave-uniform
                    const unsigned half = (unsigned)(b >> (32 * hi));   // the survivors of this half's query
                    const unsigned cnt = (unsigned)__popc(half);
                    unsigned pbase = 0u;
                    if (lo == 0 && cnt != 0u) pbase = atomicAdd(xp.cand_count + q, cnt);   // cnt != 0 implies q < Q
                    pbase = (unsigned)__shfl((int)pbase, 32 * hi);
                    const unsigned pos = pbase + (unsigned)__popc(half & ((1u << lo) - 1u));
                    if (pass && pos < (unsigned)xp.cap) {
                        xp.cand_ids[(int64_t)q * xp.cap + pos] = (int32_t)n;
                        xp.cand_scores[(int64_t)q * xp.cap + pos] = score;
                    }
                }
            }
        }
    }
}

// Three waves per SIMD, as exact_select_kernel: the staging and decode registers are dead by the epilogue.
template <int VSF, bool SELECT>
__global__ __launch_bounds__(ED_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void nvq_select_kernel(NfParams p, int64_t blocks_padded,
                                                                                                           int q_tiles)
{
    __shared__ float lds[NF_LDS_FLOATS];
    int64_t b_tile;
    int q_tile;
    if (!ed_block_to_tile((int64_t)blockIdx.x, blocks_padded, p.tiles, q_tiles, &b_tile, &q_tile)) return;
    nf_tile<VSF, SELECT>(p, b_tile, q_tile * ED_TQ, lds);
}

// select != 0: the select epilogue, else the sample epilogue.  The tiles must lie inside the rows: tile_offset + (tiles - 1) *
// tile_stride < ceil(n / 128).  vsf: the kernels' numbering (0 L2, 1 DOT, 2 COSINE).
NF_EXPORT int launch_nvq_select(hipStream_t s, const NfParams &p, size_t p_bytes, int vsf, int select)
{
    if (p_bytes != sizeof(NfParams) || vsf < 0 || vsf > 2 || p.D < 1 || p.subs < 1 || p.subs > p.D || p.ld < p.D || (p.ld & 15) ||
        p.tile_stride < 1 || p.tile_offset < 0)
        return JV_ERR_INVALID;
    if (p.Q == 0 || p.tiles == 0) return JV_OK;
    if (!p.bytes || !p.derived || !p.queries || (vsf != 0 && !p.qaux) || (vsf == 2 && (!p.cosnorm || !p.mean))) return JV_ERR_INVALID;
    if ((p.tile_offset + (p.tiles - 1) * p.tile_stride) * ED_TN >= p.n) return JV_ERR_INVALID;
    if (select ? (!p.tau || !p.cand_ids || !p.cand_scores || !p.cand_count || p.cap < 1)
               : (!p.samp || p.S > p.tiles * ED_TN || p.S <= (p.tiles - 1) * ED_TN))
        return JV_ERR_INVALID;
    const int q_tiles = (p.Q + ED_TQ - 1) / ED_TQ;
    const int64_t blocks_padded = (p.tiles * q_tiles + 7) / 8 * 8;
    if (blocks_padded > 0x7fffffffLL) return JV_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)blocks_padded), block(ED_THREADS);
#define NF_LAUNCH(SEL)                                                                                               \
    switch (vsf) {                                                                                                   \
    case 0: hipLaunchKernelGGL((nvq_select_kernel<0, SEL>), grid, block, 0, s, p, blocks_padded, q_tiles); break;   \
    case 1: hipLaunchKernelGGL((nvq_select_kernel<1, SEL>), grid, block, 0, s, p, blocks_padded, q_tiles); break;   \
    default: hipLaunchKernelGGL((nvq_select_kernel<2, SEL>), grid, block, 0, s, p, blocks_padded, q_tiles); break;  \
    }
    if (select) { NF_LAUNCH(true) }
    else { NF_LAUNCH(false) }
#undef NF_LAUNCH
    if (hipGetLastError() != hipSuccess) return JV_ERR_HIP;
    return JV_OK;
}

}  // namespace jv
