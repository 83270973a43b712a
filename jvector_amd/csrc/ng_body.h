// ng_body.h — device-resident graph traversal scored on NVQ rows alone: the walk of gw_body.h with
// NVQScorer.scoreFunctionFor(query, vsf).similarityTo(compressedVectors[node]) (B/quantization/NVQScorer.java:33-137,
// NVQVectors.scoreFunctionFor :100-109) as the score function.  The body of nvq_graph_search_kernel (k_nvq_gsearch.hip).  The beamK kept
// results leave with those scores — the bits of nvq_gather_kernel (k_nvq.hip) — and the host's top-k puts the first topK in NodeQueue
// order.  Keys, rank, keepable and out_score are xg_body.h's: NodeQueue's signed keys, float comparisons, `score >= 0` is kept.
//
// Score phase.  An expansion drops the visited neighbours of 64 adjacency slots and compacts the fresh ones with a ballot (lane j then
// holds the j-th fresh node).  The de-quantisation of a byte costs ~26 VALU instructions and an expansion seldom has many fresh rows, so
// the gather form's "a lane decodes its own row" would leave most of the wave idle behind cnt sequential decodes of D bytes.  Here the
// group is scored chunk by chunk in two phases:
//   decode   all 64 lanes.  A chunk of CH dimensions of each of R rows is cut into 16-byte pieces; CH / 16 lanes cover a row's chunk with
//            one uint4 load each and 1024 / CH rows travel per load instruction: R x CH = 64 x 64, 32 x 128 or 16 x 256 by the fresh count
//            and D, four load instructions for a full chunk, and only those that carry a fresh row are issued and decoded (wave-uniform).
//            A lane de-quantises its sixteen bytes in registers (nq_decode.h's arithmetic; the short division where the piece's (row,
//            sub-vector) allows it — both divisions are correctly rounded), walking the sub-vector boundaries inside the piece with
//            integers and fetching the derived quadruple of every sub-vector it enters; it applies the element-wise part of the similarity
//            (COSINE: + globalMean[k], EUCLIDEAN: - (query - globalMean)[k]) and parks the sixteen floats in the LDS tile [R][CH + 4].
//            Dimensions at and beyond D are stored as 0.0f.  A group of one (the entry node, the upper levels) spreads over up to 16 lanes.
//   chain    lane j owns row j: NVQScorer's sequential fma chain over the tile (acc = fma(q[k], t[k], acc); EUCLIDEAN fma(t[k], t[k], acc)),
//            `total += acc; acc = 0` at every sub-vector boundary (wave-uniform), ds_read_b128 for the row, scalar loads for the query.
//   overlap  the loads of chunk c + 1 (bytes, the pieces' first quadruples, the element-wise operand) are issued before chunk c is decoded.
// Banks.  The tile's row stride is CH + 4 dwords = 4 mod 64.  Chain reads: the 16 lanes of a b128 phase hold 16 consecutive rows and the
// same column, so they start at 16 distinct multiples of 4 banks: conflict-free in every shape.  Decode writes: a lane writes four b128 at
// row * (CH + 4) + 16 l + 4 j (l: its piece of the row).  In the 64 x 64 shape a phase of 16 lanes is 4 rows x 4 pieces, 4 row + 16 l:
// conflict-free.  In 32 x 128 it is 2 rows x 8 pieces and pieces l and l + 4 of a row meet (2-way); in 16 x 256 it is one row's 16 pieces,
// four distinct starts (4-way).  Those are 4 write instructions against ~420 VALU instructions of decode per piece and the LDS queue
// drains under them; a rotated write order would cost 48 selects per piece to remove them.
#pragma once

#include <cstdint>

#include "jv_device.h"
#include "ng_params.h"
#include "gw_body.h"
#include "nq_decode.h"

namespace jv {

typedef const __attribute__((address_space(4))) float ng_cfloat;   // wave-uniform, never written while the kernel runs: s_load

// what one chunk needs from memory, per lane: the pieces of up to four load instructions, each piece's first derived quadruple, the
// element-wise operand of the lane's sixteen dimensions (the same for every piece: they share the columns) and where the columns start
// in the sub-vector split
struct NgStage {
    uint4 r[4];
    float4 prm[4];
    float e[16];
    int s, sub_end;
};

template <class T>
GS_FN T ng_pick(const T v0, const T v1, const T v2, const T v3, int k)   // k is wave-uniform; by value: selects, not an indexed array in scratch
{
    return k == 0 ? v0 : (k == 1 ? v1 : (k == 2 ? v2 : v3));
}

// scaledLogitFunctionNQT of one byte: nq_elem's two forms (k_nvq.hip), same bits
GS_FN float ng_value(float byte, const float4 prm, bool fast)
{
    if (fast) {
        const float sv = __builtin_fmaf(byte, prm.z, prm.w);
        const int zb = __float_as_int(nq_div_fast(sv, 1.0f - sv));
        const float p = (float)(((zb & 0x7f800000) >> 23) - 128);
        const float m = __int_as_float((zb & 0x007fffff) + 0x3f800000);
        return __builtin_fmaf(m + p, prm.x, prm.y);
    }
    return nq_scaled_logit(byte, prm.x, prm.y, prm.z, prm.w);
}

// the lane's piece: bytes w = dimensions d0 .. d0 + 15 of a row whose quadruples are dp[0 .. S); (s, sub_end, prm) describe dimension d0
template <int VSF>
GS_FN void ng_decode_piece(const uint4 w, float4 prm, const float (&e)[16], int d0, int s, int sub_end, const float4 *__restrict__ dp, int D,
                           int base, int rem, float *dst)
{
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    bool fast = nq_fast_ok(prm);
    float v[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int d = d0 + t;
        if (d == sub_end && d < D) {   // the piece straddles a boundary: the next sub-vector's numbers (s + 1 < S, for d < D)
            ++s;
            sub_end += base + (s < rem ? 1 : 0);
            prm = dp[s];
            fast = nq_fast_ok(prm);
        }
        float val = ng_value((float)((ws[t >> 2] >> (8 * (t & 3))) & 0xffu), prm, fast);
        if (VSF == VSF_COS) val = val + e[t];
        else if (VSF == VSF_L2) val = val - e[t];
        v[t] = d < D ? val : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(dst + 4 * j) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
}

// one step of NVQScorer's chain (nvqDotProduct8bit / nvqSquareL2Distance8bit / nvqCosine8bit) on a decoded element
template <int VSF>
GS_FN void ng_step(float t, float a, float &acc)
{
    acc = VSF == VSF_L2 ? __builtin_fmaf(t, t, acc) : __builtin_fmaf(a, t, acc);
}

// The chain total of row `mine` (lane j < cnt holds the j-th row of the group, every other lane -1) for query q.  The shape is
// R x CH = (4096 >> ch_log2) x (1 << ch_log2), ch_log2 6 .. 8, cnt <= R.  Wave-uniform control flow outside the pieces.
template <int VSF>
GS_FN float ng_rows(const NgParams &p, int q, int32_t mine, int cnt, int ch_log2, float *tile)
{
    const int lane = gs_lane();
    const int D = p.D, S = p.S;
    const int CH = 1 << ch_log2, LS = CH + 4;   // tile row stride
    const int lpr_log2 = ch_log2 - 4;           // lanes per row piece: 4, 8, 16
    const int RPI = 64 >> lpr_log2;             // rows per load instruction: 16, 8, 4
    const int seg = (lane & ((1 << lpr_log2) - 1)) * 16;   // this lane's 16 bytes inside a row's chunk
    const int sub = lane >> lpr_log2;                      // load instruction k fetches rows RPI k + sub
    int32_t rn[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rn[k] = gs_shfl32(mine, RPI * k + sub);
    const int base = D / S, rem = D % S, lim = rem * (base + 1);   // sub-vector s covers base dimensions, the first rem one more
    const float4 *dv = reinterpret_cast<const float4 *>(p.derived);
    const float *ev = VSF == VSF_COS ? p.mean : p.queries + (int64_t)q * D;
    ng_cfloat *a = (ng_cfloat *)(p.queries + (int64_t)q * D);
    const int nc = (D + CH - 1) >> ch_log2;

    auto issue = [&](int c, NgStage &st) {
        const int d0 = c * CH + seg;
        const bool in = d0 < D;   // (ld is D rounded up to 16 and d0 a multiple of 16: d0 < D is d0 + 16 <= ld)
        int s = 0, sub_end = 0;
        if (in) {
            int start;
            if (d0 < lim) {
                s = d0 / (base + 1);
                start = s * (base + 1);
            } else {
                s = rem + (d0 - lim) / base;
                start = lim + (s - rem) * base;
            }
            sub_end = start + base + (s < rem ? 1 : 0);
        }
        st.s = s;
        st.sub_end = sub_end;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (RPI * k < cnt) {   // (wave-uniform: instructions whose rows are all beyond the group are not issued)
                const bool on = in && rn[k] >= 0;
                st.r[k] = on ? *reinterpret_cast<const uint4 *>(p.bytes + (int64_t)rn[k] * p.ld + d0) : make_uint4(0u, 0u, 0u, 0u);
                st.prm[k] = on ? dv[(int64_t)rn[k] * S + s] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        if (VSF != VSF_DOT) {
#pragma unroll
            for (int t = 0; t < 16; ++t) st.e[t] = d0 + t < D ? ev[d0 + t] : 0.0f;
        }
    };

    NgStage cur, nxt;
    issue(0, cur);
    int cs = 0, csub_end = base + (rem ? 1 : 0);   // the chain's place in the sub-vector split (wave-uniform)
    float total = 0.0f, acc = 0.0f;
    for (int c = 0; c < nc; ++c) {
        if (c + 1 < nc) issue(c + 1, nxt);
        // ---- decode: every lane its pieces of chunk c ----
        const int d0 = c * CH + seg;
#pragma nounroll
        for (int k = 0; k < 4 && RPI * k < cnt; ++k) {
            const int32_t node = ng_pick(rn[0], rn[1], rn[2], rn[3], k);
            const uint4 w = ng_pick(cur.r[0], cur.r[1], cur.r[2], cur.r[3], k);
            const float4 prm = ng_pick(cur.prm[0], cur.prm[1], cur.prm[2], cur.prm[3], k);
            float *dst = tile + (RPI * k + sub) * LS + seg;
            if (node >= 0 && d0 < D) {
                ng_decode_piece<VSF>(w, prm, cur.e, d0, cur.s, cur.sub_end, dv + (int64_t)node * S, D, base, rem, dst);
            } else {
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(dst + 4 * j) = zero;
            }
        }
        gs_barrier();
        // ---- chain: lane j over row j of the tile ----
        const int c0 = c * CH;
        const int dend = D - c0 < CH ? D : c0 + CH;
        {   // (a lane without a row walks row 0 along: uniform control flow, scalar loads for the query, and no use for what it computes)
            const float *row = tile + (lane < cnt ? lane : 0) * LS;
            int d = c0;
            while (d < dend) {
                const int seg_end = csub_end < dend ? csub_end : dend;
                int i = d - c0;
                const int iend = seg_end - c0;
                for (; i < iend && (i & 3); ++i) ng_step<VSF>(row[i], VSF == VSF_L2 ? 0.0f : a[c0 + i], acc);
                for (; i + 16 <= iend; i += 16) {   // four reads and the query's sixteen floats in flight before the sixteen steps
                    float4 t4[4];
                    float aa[16];
#pragma unroll
                    for (int u = 0; u < 4; ++u) t4[u] = *reinterpret_cast<const float4 *>(row + i + 4 * u);
#pragma unroll
                    for (int u = 0; u < 16; ++u) aa[u] = VSF == VSF_L2 ? 0.0f : a[c0 + i + u];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        ng_step<VSF>(t4[u].x, aa[4 * u], acc);
                        ng_step<VSF>(t4[u].y, aa[4 * u + 1], acc);
                        ng_step<VSF>(t4[u].z, aa[4 * u + 2], acc);
                        ng_step<VSF>(t4[u].w, aa[4 * u + 3], acc);
                    }
                }
                for (; i + 4 <= iend; i += 4) {
                    const float4 t4 = *reinterpret_cast<const float4 *>(row + i);
                    ng_step<VSF>(t4.x, VSF == VSF_L2 ? 0.0f : a[c0 + i], acc);
                    ng_step<VSF>(t4.y, VSF == VSF_L2 ? 0.0f : a[c0 + i + 1], acc);
                    ng_step<VSF>(t4.z, VSF == VSF_L2 ? 0.0f : a[c0 + i + 2], acc);
                    ng_step<VSF>(t4.w, VSF == VSF_L2 ? 0.0f : a[c0 + i + 3], acc);
                }
                for (; i < iend; ++i) ng_step<VSF>(row[i], VSF == VSF_L2 ? 0.0f : a[c0 + i], acc);
                d = seg_end;
                if (d == csub_end) {   // `nvqDot += ...` per sub-vector (NVQScorer :66)
                    total += acc;
                    acc = 0.0f;
                    ++cs;
                    if (cs < S) csub_end += base + (cs < rem ? 1 : 0);
                }
            }
        }
        gs_barrier();
        if (c + 1 < nc) cur = nxt;
    }
    return total;
}

// NVQScorer...similarityTo(row mine) for a group of cnt rows, lane j < cnt holding the j-th (others -1): nvq_gather_kernel's finish
template <int VSF>
GS_FN float ng_score_group(const NgParams &p, int q, int32_t mine, int cnt, float *tile)
{
    const int ch_log2 = (cnt <= 16 && p.D > 128) ? 8 : ((cnt <= 32 && p.D > 64) ? 7 : 6);
    const float total = ng_rows<VSF>(p, q, mine, cnt, ch_log2, tile);
    if (mine < 0) return 0.0f;
    if (VSF == VSF_DOT) return (1.0f + total + p.qaux[q]) / 2.0f;   // :71
    if (VSF == VSF_L2) return 1.0f / (1.0f + total);                // :101
    const float cosine = (total / p.qaux[q]) / (float)sqrt((double)p.cosnorm[mine]);   // :129
    return (1.0f + cosine) / 2.0f;
}

// The walk's Scorer over NVQ rows: XgScorer's keys and tests around the score phase above
template <int VSF>
struct NgScorer {
    const NgParams &p;
    int q;
    float *tile;
    int32_t *fr;   // NG_GROUP ids: the compaction of the fresh neighbours

    GS_FN long long entry_key(int32_t e) const   // a group of one row
    {
        const int32_t mine = gs_lane() == 0 ? e : -1;
        return gs_key(mine, ng_score_group<VSF>(p, q, mine, 1, tile));
    }
    static GS_FN float rank(long long k) { return gs_key_score(k); }
    static GS_FN bool keepable(float score) { return score >= 0.0f; }
    GS_FN bool score(int32_t nb, bool fresh, uint64_t fm, long long &key) const
    {
        const int lane = gs_lane();
        const int cnt = gs_popc(fm);
        if (fresh) fr[gs_popc(fm & ((1ull << lane) - 1ull))] = nb;
        gs_barrier();
        const int32_t mine = lane < cnt ? fr[lane] : -1;
        gs_barrier();
        key = gs_key(mine, ng_score_group<VSF>(p, q, mine, cnt, tile));
        return mine >= 0;
    }
    GS_FN float out_score(long long k) const { return gs_key_score(k); }
};

// One query.  LDS: [float tile][64 fresh ids][results][candidate tier][64 samples][visited table] (the tile first: its b128 accesses
// want 16 bytes)
template <int VSF, bool SAFE>
GS_FN void ng_search_one(const NgParams &p, int q, int worker, char *lds)
{
    float *tile = reinterpret_cast<float *>(lds);
    int32_t *fr = reinterpret_cast<int32_t *>(tile + NG_TILE_FLOATS);
    long long *res = reinterpret_cast<long long *>(fr + NG_GROUP);
    NgScorer<VSF> scorer{p, q, tile, fr};
    gw_search_one<SAFE>(p, q, worker, res, reinterpret_cast<uint32_t *>(res + p.rerankK + p.cand_cap + 64), scorer);
}

template <int VSF, bool SAFE>
GS_FN void ng_worker(const NgParams &p, int worker, char *lds)
{
    gw_worker(p, [&](int q) { ng_search_one<VSF, SAFE>(p, q, worker, lds); });
}

}  // namespace jv
