// bg_body.h — device-resident graph traversal over binary-quantized vectors: the walk of gw_body.h with
// BQVectors.scoreFunctionFor as the approximate score.  The body of bq_graph_search_kernel (k_bq_gsearch.hip), written against the
// wave API of gs_body.h so that the same source compiles for the lane emulator of the CPU tests (tests/emu/bg_emu.cpp).  It hands
// the rerank stage the kept approximate results with their BQ similarities.
//
// Scores.  BQVectors.similarityBetween = 1 - (float) hamming / D is strictly decreasing in the Hamming distance for every D the
// library takes (<= 16383), so the queues hold INTEGER keys: (D - hamming) << 32 | ~node — NodeQueue's order (higher score first,
// the smaller node id on equal score) without a float in the loop.  The f32 formula is applied once, when the results leave.
// A lane scores one neighbour: W 64-bit words of its row (16-byte loads when W is even: rows are then 16-byte aligned, else
// 8-byte loads) against the query's words, v_xor_b32 + v_bcnt_u32_b32 into one integer.  The query's words are wave-uniform: for the
// compiled row widths (WT > 0) they are read through a uniform address into scalar registers, else they sit in LDS.
#pragma once

#include <cstdint>

#include "bg_params.h"
#include "gw_body.h"

namespace jv {

struct alignas(16) bg_w2 { uint64_t x, y; };

GS_FN long long bg_key(int32_t node, int32_t closeness) { return (long long)(((unsigned long long)(uint32_t)closeness << 32) | (unsigned long long)(uint32_t)(~node)); }
GS_FN int32_t bg_key_hi(long long k) { return (int32_t)(k >> 32); }

// The walk's Scorer over BQ rows.  WT > 0: rows of exactly WT words, the query's words in (scalar) registers; WT == 0: any width, the
// words in LDS.  The walk compares the integer high halves of the keys; a BQ similarity is never negative or NaN: every key is keepable.
template <int WT>
struct BgScorer {
    const BgParams &p;
    const uint64_t *qw_lds;
    uint64_t qw[WT > 0 ? WT : 1];

    // hammingDistance(query words, row nb): DefaultVectorUtilSupport.hammingDistance, every word's loads issued before the counts
    GS_FN int32_t hamming(int32_t nb) const
    {
        int32_t h = 0;
        const int W = WT > 0 ? WT : p.W;
        const uint64_t *r = p.rows + (int64_t)nb * W;
        if constexpr (WT > 0 && WT % 2 == 0) {
            const bg_w2 *r2 = reinterpret_cast<const bg_w2 *>(r);
            bg_w2 v[WT / 2];
#pragma unroll
            for (int i = 0; i < WT / 2; ++i) v[i] = r2[i];
#pragma unroll
            for (int i = 0; i < WT / 2; ++i) h += gs_popc(v[i].x ^ qw[2 * i]) + gs_popc(v[i].y ^ qw[2 * i + 1]);
        } else if constexpr (WT > 0) {
            uint64_t v[WT];
#pragma unroll
            for (int i = 0; i < WT; ++i) v[i] = r[i];
#pragma unroll
            for (int i = 0; i < WT; ++i) h += gs_popc(v[i] ^ qw[i]);
        } else if ((W & 1) == 0) {
            const bg_w2 *r2 = reinterpret_cast<const bg_w2 *>(r);
            for (int i = 0; i < W; i += 2) {
                const bg_w2 v = r2[i >> 1];
                h += gs_popc(v.x ^ qw_lds[i]) + gs_popc(v.y ^ qw_lds[i + 1]);
            }
        } else {
            for (int i = 0; i < W; ++i) h += gs_popc(r[i] ^ qw_lds[i]);
        }
        return h;
    }
    GS_FN long long entry_key(int32_t e) const { return bg_key(e, p.D - hamming(e)); }
    static GS_FN int32_t rank(long long k) { return bg_key_hi(k); }
    static GS_FN bool keepable(int32_t) { return true; }
    // in place, one lane per neighbour
    GS_FN bool score(int32_t nb, bool fresh, uint64_t, long long &key) const
    {
        int32_t c = 0;
        if (fresh) c = p.D - hamming(nb);
        key = bg_key(nb, c);
        return fresh;
    }
    // BQVectors.similarityBetween in f32
    GS_FN float out_score(long long k) const { return 1.0f - (float)(p.D - bg_key_hi(k)) / (float)p.D; }
};

// One query.  LDS: [results][candidate tier][64 samples][query words (WT == 0 only)][visited table]
template <int WT, bool SAFE>
GS_FN void bg_search_one(const BgParams &p, int q, int worker, char *lds)
{
    const int W = WT > 0 ? WT : p.W;
    long long *res = reinterpret_cast<long long *>(lds);
    uint64_t *qw_lds = reinterpret_cast<uint64_t *>(res + p.rerankK + p.cand_cap + 64);
    uint32_t *vis_lds = reinterpret_cast<uint32_t *>(qw_lds + (WT > 0 ? 0 : p.W));
    BgScorer<WT> scorer{p, qw_lds, {}};
    // fetch the query's words
    if constexpr (WT > 0) {
        const uint64_t *src = p.qwords + (int64_t)q * WT;   // q is wave-uniform: scalar loads
#pragma unroll
        for (int i = 0; i < WT; ++i) scorer.qw[i] = src[i];
    } else {
        scorer.qw[0] = 0;
        const uint64_t *src = p.qwords + (int64_t)q * W;
        for (int i = gs_lane(); i < W; i += 64) qw_lds[i] = src[i];
    }
    gw_search_one<SAFE>(p, q, worker, res, vis_lds, scorer);
}

template <int WT, bool SAFE>
GS_FN void bg_worker(const BgParams &p, int worker, char *lds)
{
    gw_worker(p, [&](int q) { bg_search_one<WT, SAFE>(p, q, worker, lds); });
}

}  // namespace jv
