// k_ubr_table.hip — the dense kernel that builds the 8-bit bound tables of a whole batch for the register-table traversal (gs_body.h
// "UBR", k_gsearch_ubr.hip): [Q][M / 4][64] x 16 bytes in the traversal's register-pair layout plus four meta floats per query.
// Arithmetic and layout = gs_ubr_build_ref (gs_host.h), bit for bit (tests/test_zz_ubr_gpu.py, tests/test_zz_ubr_table_shapes_gpu.py).
// A translation unit of its own: none of the traversal's code-generation flags (-mllvm -enable-ipra=0) apply to it.
//
// One block = UBR_QB queries x all M subspaces, 4 waves; lane s takes the codes s, s + 64, s + 128, s + 192 of a subspace, so a
// codebook row is loaded once per pass and used for every query of the block.  The queries sit in LDS as PAIRS, {q_2p[d], q_2p+1[d]}
// per dimension: one v_pk_mul_f32 / v_pk_add_f32 then runs the entry chains of two queries at once (the codebook value is the
// operand both halves share, op_sel), the same IEEE operations in the same order as the scalar chain — 4 + 4 packed instructions per
// dot-product entry.
//   pass 1: every entry once, for its subspace's extremes — per lane v_min3 / v_max3 over the lane's four codes, then the 16 partial
//           extremes of the 8 queries folded across the wave TOGETHER (permlane32_swap, permlane16_swap, 4 DPP row steps: 2.5
//           instructions per value instead of a 6-step DPP chain each); non-finite entries are caught by one v_pk_fma_f32 per two
//           entries (e * 0 + acc is NaN from the first non-finite e on, exactly the entries the old |bits| >= 0x7f800000 test found);
//   the scale of each query (one thread per query, the reference's sequential loops);
//   pass 2: every entry again, its bucket in packed arithmetic ((e - lo) * inv +- 2^-10 for two queries per instruction), and the
//           register pair (2r, 2r + 1) of every lane as one 8-byte store.
#include "jv_device.h"
#include "jv_internal.h"

namespace jv {

namespace {

constexpr int UBR_QB = 8;            // queries per block
constexpr int UBR_QP = UBR_QB / 2;   // query pairs per block
constexpr int UBR_WAVES = 4;
constexpr int UBR_MAX_M = 256;       // the largest M the kernel is built and tested for

typedef float ubr_f2 __attribute__((ext_vector_type(2)));
typedef float ubr_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t ubr_u2 __attribute__((ext_vector_type(2)));

// the entries of one codebook row (c0, c1) for a query pair q[8] = {qa[d], qb[d]}: calculatePartialSums' chain in each half (gs_host.h;
// euclidean: squareDistance's t = c - q, ent += t * t), the codebook value broadcast to both halves by op_sel; `0 + first product`
// as in the reference (x - y is x + (-y) in IEEE arithmetic).  One asm block per chain: the compiler assembles the broadcast of an
// odd register with a v_mov one time in four, and puts an s_nop behind every single-instruction asm whose result is read next.
template <int VSF>
__device__ __forceinline__ ubr_f2 ubr_entry2(const ubr_f4 c0, const ubr_f4 c1, const ubr_f2 *q)
{
    const ubr_f2 a = {c0.x, c0.y}, b = {c0.z, c0.w}, c = {c1.x, c1.y}, d = {c1.z, c1.w};
    ubr_f2 ent, t;
    if (VSF == VSF_L2) {
#define JV_UBR_STEP(SEL, C, Q) "v_pk_add_f32 %1, " C ", " Q " " SEL " neg_lo:[0,1] neg_hi:[0,1]\n" "v_pk_mul_f32 %1, %1, %1\n" "v_pk_add_f32 %0, %0, %1\n"
        asm("v_pk_add_f32 %1, %2, %6 op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]\n"
            "v_pk_mul_f32 %1, %1, %1\n"
            "v_pk_add_f32 %0, %1, 0 op_sel_hi:[1,0]\n"
            JV_UBR_STEP("op_sel:[1,0]", "%2", "%7") JV_UBR_STEP("op_sel_hi:[0,1]", "%3", "%8") JV_UBR_STEP("op_sel:[1,0]", "%3", "%9")
            JV_UBR_STEP("op_sel_hi:[0,1]", "%4", "%10") JV_UBR_STEP("op_sel:[1,0]", "%4", "%11")
            JV_UBR_STEP("op_sel_hi:[0,1]", "%5", "%12") JV_UBR_STEP("op_sel:[1,0]", "%5", "%13")
            : "=&v"(ent), "=&v"(t)
            : "v"(a), "v"(b), "v"(c), "v"(d), "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]), "v"(q[7]));
#undef JV_UBR_STEP
    } else {
#define JV_UBR_STEP(SEL, C, Q) "v_pk_mul_f32 %1, " C ", " Q " " SEL "\n" "v_pk_add_f32 %0, %0, %1\n"
        asm("v_pk_mul_f32 %1, %2, %6 op_sel_hi:[0,1]\n"
            "v_pk_add_f32 %0, %1, 0 op_sel_hi:[1,0]\n"
            JV_UBR_STEP("op_sel:[1,0]", "%2", "%7") JV_UBR_STEP("op_sel_hi:[0,1]", "%3", "%8") JV_UBR_STEP("op_sel:[1,0]", "%3", "%9")
            JV_UBR_STEP("op_sel_hi:[0,1]", "%4", "%10") JV_UBR_STEP("op_sel:[1,0]", "%4", "%11")
            JV_UBR_STEP("op_sel_hi:[0,1]", "%5", "%12") JV_UBR_STEP("op_sel:[1,0]", "%5", "%13")
            : "=&v"(ent), "=&v"(t)
            : "v"(a), "v"(b), "v"(c), "v"(d), "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]), "v"(q[7]));
#undef JV_UBR_STEP
    }
    return ent;
}

// v_min_f32 / v_max_f32 written out: the operands are products of the packed chains or moved copies of them, never signalling NaNs,
// and __builtin_fminf would canonicalise every operand that comes out of an asm block or a permlane first (one v_max_f32 x, x each)
__device__ __forceinline__ float ubr_min(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float ubr_max(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// the extremes of four entries: v_min_f32 + v_min3_f32, v_max_f32 + v_max3_f32
__device__ __forceinline__ void ubr_minmax4(float e0, float e1, float e2, float e3, float &mn, float &mx)
{
    asm("v_min_f32 %0, %2, %3\n"
        "v_max_f32 %1, %2, %3\n"
        "v_min3_f32 %0, %0, %4, %5\n"
        "v_max3_f32 %1, %1, %4, %5"
        : "=&v"(mn), "=&v"(mx) : "v"(e0), "v"(e1), "v"(e2), "v"(e3));
}

__device__ __forceinline__ float ubr_swap_fold(float a, float b, bool lanes32, bool is_min)
{
    const uint32_t ua = __builtin_bit_cast(uint32_t, a), ub = __builtin_bit_cast(uint32_t, b);
    float x, y;
    if (lanes32) {
        const auto r = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);
        x = __builtin_bit_cast(float, (uint32_t)r[0]);
        y = __builtin_bit_cast(float, (uint32_t)r[1]);
    } else {
        const auto r = __builtin_amdgcn_permlane16_swap(ua, ub, false, false);
        x = __builtin_bit_cast(float, (uint32_t)r[0]);
        y = __builtin_bit_cast(float, (uint32_t)r[1]);
    }
    return is_min ? ubr_min(x, y) : ubr_max(x, y);
}

// mn[j] / mx[j]: this lane's partial extremes of query j.  Folds all 16 across the wave; afterwards lane 16 rho + 15 of mn[k] / mx[k]
// (k = 0, 1) holds the wave's minimum / maximum of query 4 k + ubr_fold_query(rho).
//   permlane32_swap(a = v[2i], b = v[2i + 1]) leaves {a[0:32], b[0:32]} and {a[32:64], b[32:64]}: their min has query 2i in lanes 0-31
//   and 2i + 1 in lanes 32-63; permlane16_swap of two such registers (rows of 16 lanes r0..r3) leaves {a.r0, b.r0, a.r2, b.r2} and
//   {a.r1, b.r1, a.r3, b.r3}: rows 0..3 of their min hold queries 4k, 4k + 2, 4k + 1, 4k + 3; row_shr 1, 2, 4, 8 finish each row in
//   its lane 15.  min / max skip NaN in every order (no entry is a signalling NaN), so the result is the old chain's.
__device__ __forceinline__ int ubr_fold_query(int rho) { return ((rho & 1) << 1) | (rho >> 1); }
__device__ __forceinline__ void ubr_fold_extremes(float (&mn)[UBR_QB], float (&mx)[UBR_QB])
{
    float a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[i] = ubr_swap_fold(mn[2 * i], mn[2 * i + 1], true, true);
        b[i] = ubr_swap_fold(mx[2 * i], mx[2 * i + 1], true, false);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        mn[k] = ubr_swap_fold(a[2 * k], a[2 * k + 1], false, true);
        mx[k] = ubr_swap_fold(b[2 * k], b[2 * k + 1], false, false);
    }
    // four independent chains: each DPP read comes three instructions after the write of its operand (two wait states needed); the
    // s_nop covers the compiler's last writes before the block.  All 64 lanes must be active.
#define JV_UBR_ROW_STEP(CTRL)                                      \
    "v_min_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n" \
    "v_min_f32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n" \
    "v_max_f32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n" \
    "v_max_f32_dpp %3, %3, %3 " CTRL " row_mask:0xf bank_mask:0xf\n"
    asm volatile("s_nop 1\n" JV_UBR_ROW_STEP("row_shr:1") JV_UBR_ROW_STEP("row_shr:2") JV_UBR_ROW_STEP("row_shr:4") JV_UBR_ROW_STEP("row_shr:8")
                 : "+v"(mn[0]), "+v"(mn[1]), "+v"(mx[0]), "+v"(mx[1]));
#undef JV_UBR_ROW_STEP
}

template <int VSF>
__global__ __launch_bounds__(64 * UBR_WAVES) __attribute__((amdgpu_waves_per_eu(4))) void ubr_table_kernel(const float *__restrict__ codebooks, const float *__restrict__ cq, int Q,
                                                                    int M, uint32_t *__restrict__ tab, float *__restrict__ meta)
{
    extern __shared__ __attribute__((aligned(16))) char ubr_lds[];
    const int D = 8 * M, H = M / 2;
    ubr_f2 *qp = reinterpret_cast<ubr_f2 *>(ubr_lds);                // [UBR_QP][D] {query 2p, query 2p + 1}
    float *lo = reinterpret_cast<float *>(qp + UBR_QP * D);          // [M][UBR_QB]
    float *hi = lo + M * UBR_QB;                                     // [M][UBR_QB]
    float *qinv = hi + M * UBR_QB;                                   // [UBR_QB] 1 / scale
    int *qbad = reinterpret_cast<int *>(qinv + UBR_QB);              // [UBR_QB] no usable table
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = (int)blockIdx.x * UBR_QB;
    const int nq = min(UBR_QB, Q - q0);
    // the queries, interleaved in pairs (a ragged block's missing queries are zero: their entries are finite, their rows not stored)
    for (int i = tid; i < UBR_QP * D / 2; i += 64 * UBR_WAVES) {
        const int p = i / (D / 2), d2 = i - p * (D / 2);
        ubr_f2 a = {0.0f, 0.0f}, b = {0.0f, 0.0f};
        if (2 * p < nq) a = reinterpret_cast<const ubr_f2 *>(cq + (int64_t)(q0 + 2 * p) * D)[d2];
        if (2 * p + 1 < nq) b = reinterpret_cast<const ubr_f2 *>(cq + (int64_t)(q0 + 2 * p + 1) * D)[d2];
        reinterpret_cast<ubr_f4 *>(qp)[i] = ubr_f4{a.x, b.x, a.y, b.y};
    }
    if (tid < UBR_QB) qbad[tid] = 0;
    __syncthreads();

    // ---- pass 1: lo / hi of every (query, subspace) ----
    ubr_f2 nonfinite[UBR_QP];
#pragma unroll
    for (int p = 0; p < UBR_QP; ++p) nonfinite[p] = ubr_f2{0.0f, 0.0f};
    for (int m = wave; m < M; m += UBR_WAVES) {
        ubr_f4 c0[4], c1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const ubr_f4 *cp = reinterpret_cast<const ubr_f4 *>(codebooks + ((int64_t)m * 256 + lane + 64 * k) * 8);
            c0[k] = cp[0];
            c1[k] = cp[1];
        }
        float mn[UBR_QB], mx[UBR_QB];
#pragma unroll
        for (int p = 0; p < UBR_QP; ++p) {
            ubr_f2 q[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) q[t] = qp[p * D + m * 8 + t];
            ubr_f2 e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                e[k] = ubr_entry2<VSF>(c0[k], c1[k], q);
                nonfinite[p] = __builtin_elementwise_fma(e[k], ubr_f2{0.0f, 0.0f}, nonfinite[p]);
            }
            ubr_minmax4(e[0].x, e[1].x, e[2].x, e[3].x, mn[2 * p], mx[2 * p]);
            ubr_minmax4(e[0].y, e[1].y, e[2].y, e[3].y, mn[2 * p + 1], mx[2 * p + 1]);
        }
        ubr_fold_extremes(mn, mx);
        if ((lane & 15) == 15) {
            const int j = ubr_fold_query(lane >> 4);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                lo[m * UBR_QB + 4 * k + j] = mn[k];
                hi[m * UBR_QB + 4 * k + j] = mx[k];
            }
        }
    }
#pragma unroll
    for (int p = 0; p < UBR_QP; ++p) {
        const bool ba = __ballot(nonfinite[p].x != nonfinite[p].x ? 1 : 0) != 0;
        const bool bb = __ballot(nonfinite[p].y != nonfinite[p].y ? 1 : 0) != 0;
        if (lane == 0 && ba) qbad[2 * p] = 1;   // (benign race: every writer stores 1)
        if (lane == 0 && bb) qbad[2 * p + 1] = 1;
    }
    __syncthreads();

    // ---- one scale per query; base = sum of the low edges + slack ----
    if (tid < UBR_QB) {
        const int j = tid;
        float range = 0.0f;
        for (int m = 0; m < M; ++m) {
            const float r = hi[m * UBR_QB + j] - lo[m * UBR_QB + j];
            if (r > range) range = r;
        }
        float S = range / 255.0f;
        if (!(S > 1e-30f)) S = 1e-30f;
        float sum_lo = 0.0f, sum_abs = 0.0f, max_abs = 0.0f;
        for (int m = 0; m < M; ++m) {
            const float l = lo[m * UBR_QB + j], h = hi[m * UBR_QB + j];
            sum_lo += l;
            const float amn = l < 0.0f ? -l : l, amx = h < 0.0f ? -h : h;
            const float a = amn > amx ? amn : amx;
            sum_abs += a + 256.0f * S;
            if (a > max_abs) max_abs = a;
        }
        // (usable only if a bucket is not lost in the rounding of an edge: lo + 256 S then bounds every entry of a subspace in f32 too)
        const bool ok = qbad[j] == 0 && (sum_abs - sum_abs == 0.0f) && S * 1e6f >= max_abs;
        qinv[j] = 1.0f / S;
        if (!ok) qbad[j] = 1;
        if (j < nq) {
            float *mq = meta + (int64_t)(q0 + j) * 4;
            mq[0] = (VSF == VSF_L2) ? sum_lo - 4e-5f * sum_abs : sum_lo + 4e-5f * sum_abs;   // (euclidean: a LOWER bound of the distance)
            mq[1] = S;
            mq[2] = ok ? 1.0f : 0.0f;
            mq[3] = 0.0f;
        }
    }
    __syncthreads();

    // ---- pass 2: buckets, packed into the register pairs ----
    // (gs_host.h gs_ubr_build_ref: floor of the f32 quotient plus 2^-10 — its upper edge bounds the entry; euclidean: minus 2^-10,
    // lower bucket edges)
    const ubr_f2 edge = (VSF == VSF_L2) ? ubr_f2{-0x1p-10f, -0x1p-10f} : ubr_f2{0x1p-10f, 0x1p-10f};
    for (int r = wave; r < H; r += UBR_WAVES) {
        // the pair (2r, 2r + 1) of every query, filled half by half: subspace r gives bytes 0 / 1, subspace r + M/2 bytes 2 / 3
        uint32_t w[UBR_QB][2];
#pragma unroll
        for (int j = 0; j < UBR_QB; ++j) w[j][0] = w[j][1] = 0u;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int m = r + half * H;
            ubr_f4 c0[4], c1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const ubr_f4 *cp = reinterpret_cast<const ubr_f4 *>(codebooks + ((int64_t)m * 256 + lane + 64 * k) * 8);
                c0[k] = cp[0];
                c1[k] = cp[1];
            }
#pragma unroll
            for (int p = 0; p < UBR_QP; ++p) {
                if (2 * p >= nq) continue;
                const ubr_f2 inv = *reinterpret_cast<const ubr_f2 *>(qinv + 2 * p);
                const ubr_f2 l = *reinterpret_cast<const ubr_f2 *>(lo + m * UBR_QB + 2 * p);
                ubr_f2 q[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) q[t] = qp[p * D + m * 8 + t];
#pragma unroll
                for (int k = 0; k < 4; ++k) {   // codes s, s + 64 -> register 2r; s + 128, s + 192 -> register 2r + 1
                    const ubr_f2 x = (ubr_entry2<VSF>(c0[k], c1[k], q) - l) * inv + edge;
                    int ba = (int)x.x, bb = (int)x.y;
                    ba = ba < 0 ? 0 : (ba > 255 ? 255 : ba);
                    bb = bb < 0 ? 0 : (bb > 255 ? 255 : bb);
                    w[2 * p][k >> 1] |= (uint32_t)ba << (8 * (k & 1) + 16 * half);
                    w[2 * p + 1][k >> 1] |= (uint32_t)bb << (8 * (k & 1) + 16 * half);
                }
            }
        }
        const int k0 = 2 * r;   // even: the pair (k0, k0 + 1) is the lower or the upper half of one 16-byte group
        const int64_t off = ((int64_t)(k0 / 4) * 64 + lane) * 4 + (k0 % 4);
#pragma unroll
        for (int j = 0; j < UBR_QB; ++j) {
            if (j >= nq) continue;
            ubr_u2 out = {w[j][0], w[j][1]};
            if (qbad[j]) out = ubr_u2{0u, 0u};
            *reinterpret_cast<ubr_u2 *>(tab + (int64_t)(q0 + j) * M * 64 + off) = out;
        }
    }
}

size_t ubr_table_lds_bytes(int M)
{
    return sizeof(float) * ((size_t)UBR_QB * 8 * M + 2 * (size_t)UBR_QB * M + UBR_QB) + sizeof(int) * UBR_QB;
}

}  // namespace

// tables + meta of queries [0, Q): tab = Q x gs_ubr_tab_bytes(M), meta = Q x 4 floats
int launch_ubr_tables(hipStream_t s, int vsf, const float *codebooks, const float *cq, int Q, int M, uint32_t *tab, float *meta)
{
    if (Q == 0) return JV_OK;
    if (M <= 0 || M % 8 != 0) {
        set_error("ubr tables: M a multiple of 8 (M = %d)", M);
        return JV_ERR_INVALID;
    }
    if (M > UBR_MAX_M) {
        set_error("ubr tables: M = %d (at most %d subspaces)", M, UBR_MAX_M);
        return JV_ERR_UNSUPPORTED;
    }
    const size_t lds = ubr_table_lds_bytes(M);
    dim3 grid((unsigned)((Q + UBR_QB - 1) / UBR_QB)), block(64 * UBR_WAVES);
#define JV_UBR_TABLES(VSFV)                                                                                                             \
    do {                                                                                                                                \
        JV_HIP_CHECK(hipFuncSetAttribute((const void *)ubr_table_kernel<VSFV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(ubr_table_kernel<VSFV>, grid, block, lds, s, codebooks, cq, Q, M, tab, meta);                                \
    } while (0)
    if (vsf == VSF_L2) JV_UBR_TABLES(VSF_L2);
    else if (vsf == VSF_DOT) JV_UBR_TABLES(VSF_DOT);
    else JV_UBR_TABLES(VSF_COS);
#undef JV_UBR_TABLES
    JV_HIP_CHECK(hipGetLastError());
    return JV_OK;
}

}  // namespace jv
