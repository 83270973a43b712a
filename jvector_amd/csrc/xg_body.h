// xg_body.h — device-resident graph traversal with EXACT scores: the walk of gw_body.h with VectorSimilarityFunction.compare on the
// float rows as the score function.  The body of exact_graph_search_kernel (k_exact_gsearch.hip).  The beamK kept results leave with
// their exact scores; the host's top-k puts the first topK in NodeQueue order.
//
// Keys.  The queues hold NodeQueue's own keys, gs_key = sortableInt(score) << 32 | ~node as a SIGNED 64-bit integer: a negative score
// has a negative sortable int and a negative key, and signed comparison orders them as NodeQueue.encode does (-0.0 below +0.0).  The
// walk's own tests — stopSearch's `<`, addTopCandidate's `>` — are the reference's FLOAT comparisons on the decoded scores (-0.0 equals
// +0.0 there, a NaN compares false), never comparisons of key halves.
//
// Score phase.  An expansion drops the visited neighbours of 64 adjacency slots, compacts the fresh ones with a ballot (lane j then
// holds the j-th fresh node) and scores them together, one lane per row:
//   load     the rows travel as in k_exact.hip's tr_rows: a chunk of CH floats of each of R rows, 16 bytes per lane and CH / 4 lanes per
//            row (whole 128-byte lines), parked in an LDS tile [R][CH + 4].  Only the load instructions that carry a fresh row are issued:
//            a group of 9 rows in the 16 x 256 shape costs 9 of the 16, not 16.
//   compute  lane j runs the reference's chain (xc_chain.h: dot8 / l28 per 8-block, non-fused) over row j of the tile with
//            ds_read_b128 (row stride CH + 4 dwords: conflict-free); the query slice is wave-uniform and read through the constant address
//            space, i.e. scalar loads into SGPR operands — no LDS for the query.
//   overlap  the loads of chunk c + 1 are issued into registers before chunk c is computed.  ONE tile, not two: the wavefront is alone in
//            its workgroup, its LDS operations complete in order, so a second tile would buy no overlap and cost 17 KB of occupancy.
//   shape    R x CH = 64 x 64, 32 x 128 or 16 x 256 by the fresh count and D (a longer contiguous piece per row when few rows are fresh
//            and the row is long enough to fill it).  The chain order inside a row does not depend on the shape: same bits.
//   cosine   norm2 comes from the per-row table (launch_row_sqnorms), the query's norm from launch_query_sqnorms: cosine_finish.
//   fallback rows that are not 16-byte aligned or D % 8 != 0 (TR = false): a lane walks its own row with exact_row / cosine_row, as
//            exact_gather_kernel does.
// The entry node and the levels above 0 go through the same phase as groups of one or a few rows.
#pragma once

#include <cstdint>

#include "xg_params.h"
#include "gw_body.h"
#include "xc_chain.h"

namespace jv {

typedef const __attribute__((address_space(4))) float xg_cfloat;   // wave-uniform, never written while the kernel runs: s_load

// the chain over one chunk of `len` floats (a multiple of 8) of the lane's row in the tile against the uniform query slice a[]
template <int VSF, int CH>
GS_FN void xg_chunk(const float *row, xg_cfloat *a, int len, float &acc)
{
    auto block = [&](int i) {
        float aa[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) aa[u] = a[i + u];
        const float4 v0 = *reinterpret_cast<const float4 *>(row + i);
        const float4 v1 = *reinterpret_cast<const float4 *>(row + i + 4);
        if (VSF == VSF_DOT) acc += dot8(aa, v0, v1);
        else if (VSF == VSF_L2) acc += l28(aa, v0, v1);
        else {   // DefaultVectorUtilSupport.cosine's `sum`: one running accumulator
            float s = acc;
            s += aa[0] * v0.x; s += aa[1] * v0.y; s += aa[2] * v0.z; s += aa[3] * v0.w;
            s += aa[4] * v1.x; s += aa[5] * v1.y; s += aa[6] * v1.z; s += aa[7] * v1.w;
            acc = s;
        }
    };
    if (len == CH) {
#pragma unroll 8
        for (int i = 0; i < CH; i += 8) block(i);
    } else {
        for (int i = 0; i < len; i += 8) block(i);
    }
}

// Raw chain value of row my_node (lane j < cnt holds the j-th row of the group, every other lane -1) against the query a[0 .. D).
// D % 8 == 0, rows 16-byte aligned, cnt <= R.  Wave-uniform control flow: every lane takes part in the loads.
template <int VSF, int R, int CH>
GS_FN float xg_tr_rows(const float *rows, int D, int32_t my_node, int cnt, xg_cfloat *a, float *tile)
{
    constexpr int LS = CH + 4, LPR = CH / 4, RPI = 64 / LPR;   // tile row stride, lanes per row piece, rows per load instruction
    static_assert(R * CH == 4096 && R == 16 * RPI && R * LS <= XG_TILE_FLOATS, "sixteen 1 KB load instructions per full chunk");
    const int lane = gs_lane();
    const int seg = (lane % LPR) * 4;   // this lane's 16 bytes inside a row's chunk
    const int sub = lane / LPR;         // load instruction k fetches rows RPI k + sub
    int32_t rn[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) rn[k] = gs_shfl32(my_node, RPI * k + sub);
    const int nc = (D + CH - 1) / CH;
    float4 r[16];
    auto issue = [&](int c) {
        const bool in = c * CH + seg < D;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (RPI * k < cnt)   // (wave-uniform: instructions whose rows are all beyond the group are not issued)
                r[k] = (rn[k] >= 0 && in) ? *reinterpret_cast<const float4 *>(rows + (int64_t)rn[k] * D + c * CH + seg) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    issue(0);
    float acc = 0.0f;
    for (int c = 0; c < nc; ++c) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (RPI * k < cnt) *reinterpret_cast<float4 *>(tile + (RPI * k + sub) * LS + seg) = r[k];
        gs_barrier();
        if (c + 1 < nc) issue(c + 1);
        const int len = (D - c * CH < CH) ? (D - c * CH) : CH;
        if (lane < cnt) xg_chunk<VSF, CH>(tile + lane * LS, a + c * CH, len, acc);
        gs_barrier();
    }
    return acc;
}

// VectorSimilarityFunction.compare(query q, row my_node) for a group of cnt rows, lane j < cnt holding the j-th (others -1)
template <int VSF, bool TR>
GS_FN float xg_score_group(const XgParams &p, int q, int32_t my_node, int cnt, float *tile)
{
    const int D = p.D;
    float raw = 0.0f;
    if (TR) {
        xg_cfloat *a = (xg_cfloat *)(p.queries + (int64_t)q * D);
        if (cnt <= 16 && D > 128) raw = xg_tr_rows<VSF, 16, 256>(p.rows, D, my_node, cnt, a, tile);
        else if (cnt <= 32 && D > 64) raw = xg_tr_rows<VSF, 32, 128>(p.rows, D, my_node, cnt, a, tile);
        else raw = xg_tr_rows<VSF, 64, 64>(p.rows, D, my_node, cnt, a, tile);
        if (VSF == VSF_COS && my_node >= 0) raw = cosine_finish(raw, p.qnorm[q], p.vnorm[my_node]);
    } else if (my_node >= 0) {
        const float *a = p.queries + (int64_t)q * D;
        const float *b = p.rows + (int64_t)my_node * D;
        if (VSF == VSF_COS) {
            float sum, norm2;
            cosine_row(a, b, D, sum, norm2);
            raw = cosine_finish(sum, p.qnorm[q], norm2);
        } else {
            raw = exact_row<VSF>(a, b, D);
        }
    }
    return score_from_raw(VSF, raw);
}

// The walk's Scorer over float rows: keys compare as their decoded scores, a negative or NaN score is expanded but never kept.
template <int VSF, bool TR>
struct XgScorer {
    const XgParams &p;
    int q;
    float *tile;
    int32_t *fr;   // XG_GROUP ids: the compaction of the fresh neighbours

    GS_FN long long entry_key(int32_t e) const   // a group of one row
    {
        const int32_t mine = gs_lane() == 0 ? e : -1;
        return gs_key(mine, xg_score_group<VSF, TR>(p, q, mine, 1, tile));
    }
    static GS_FN float rank(long long k) { return gs_key_score(k); }
    static GS_FN bool keepable(float score) { return score >= 0.0f; }
    // compaction: lane j takes the j-th fresh neighbour, then the group is scored one lane per row
    GS_FN bool score(int32_t nb, bool fresh, uint64_t fm, long long &key) const
    {
        const int lane = gs_lane();
        const int cnt = gs_popc(fm);
        if (fresh) fr[gs_popc(fm & ((1ull << lane) - 1ull))] = nb;
        gs_barrier();
        const int32_t mine = lane < cnt ? fr[lane] : -1;
        gs_barrier();
        key = gs_key(mine, xg_score_group<VSF, TR>(p, q, mine, cnt, tile));
        return mine >= 0;
    }
    GS_FN float out_score(long long k) const { return gs_key_score(k); }
};

// One query.  LDS: [score tile][64 fresh ids][results][candidate tier][64 samples][visited table] (the tile first: its b128 accesses
// want 16 bytes)
template <int VSF, bool TR, bool SAFE>
GS_FN void xg_search_one(const XgParams &p, int q, int worker, char *lds)
{
    float *tile = reinterpret_cast<float *>(lds);
    int32_t *fr = reinterpret_cast<int32_t *>(tile + XG_TILE_FLOATS);
    long long *res = reinterpret_cast<long long *>(fr + XG_GROUP);
    XgScorer<VSF, TR> scorer{p, q, tile, fr};
    gw_search_one<SAFE>(p, q, worker, res, reinterpret_cast<uint32_t *>(res + p.rerankK + p.cand_cap + 64), scorer);
}

template <int VSF, bool TR, bool SAFE>
GS_FN void xg_worker(const XgParams &p, int worker, char *lds)
{
    gw_worker(p, [&](int q) { xg_search_one<VSF, TR, SAFE>(p, q, worker, lds); });
}

}  // namespace jv
