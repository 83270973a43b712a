// bd_body.h — batched robust prune over binary-quantized rows: VamanaDiversityProvider.retainDiverse
// (B/graph/diversity/VamanaDiversityProvider.java:45-96) for P nodes at once with the diversity score of
// BuildScoreProvider.bqBuildScoreProvider (B/graph/similarity/BuildScoreProvider.java:214-258): BQVectors.similarityBetween of two
// stored rows, 1 - (float) hamming / D.  The body of bq_retain_kernel (k_bq_retain.hip), written against the wave API of gs_body.h so
// that the same source compiles for the lane emulator of the CPU tests (tests/emu/bd_emu.cpp).  rd_body.h is its PQ twin.
//
// One 64-lane wavefront per node.  The node's candidate rows (C x W words) are staged into LDS once, every load independent of
// every other.  The walk over the candidates — once per alpha step 1.0, 1.2, ... <= alpha + 1e-6 — is sequential by definition;
// what runs in parallel is isDiverse (:83-96): lane j owns selected slot j (maxDegree <= 64), xors the candidate's W words (one
// LDS address for the whole wave) with its slot's (kept word-major: 64 consecutive words per read), counts the bits and makes the
// reference's own f32 comparison, 1 - (float) h / D > score * alpha: one division per lane and test, no integer stand-in to derive.
// isDiverse walks the selected set in ascending POSITION and stops at the first event — the candidate's own node id (diverse) or a
// violation (not diverse).  A lane whose slot holds the candidate's id never reports a violation; if no slot holds it (one ballot
// says so) any violation decides, else only a violation at a position below the first such slot does.
// A selected slot keeps its position, node id and "ordinal inside the rows" in registers of its lane; LDS holds rows, ids and scores.
#pragma once

#include <cstdint>

#include "bd_params.h"
#include "gs_body.h"

namespace jv {

// WT > 0: rows of exactly WT words (unrolled, every LDS read issued before the counts); WT == 0: any width
template <int WT>
GS_FN void bd_node(const BdParams &p, int node_idx, char *lds)
{
    const int lane = gs_lane();
    const int W = WT > 0 ? WT : p.W;
    const int C = p.C;
    const float fD = (float)p.D;
    uint64_t *cc = reinterpret_cast<uint64_t *>(lds);           // [C][W] candidate rows
    uint64_t *ss = cc + (size_t)C * W;                           // [W][64] selected slots' rows, word-major
    int32_t *cid = reinterpret_cast<int32_t *>(ss + (size_t)W * 64);   // [C] candidate ordinals
    float *csc = reinterpret_cast<float *>(cid + C);             // [C] candidate scores
    const int32_t *nodes = p.cand_nodes + (int64_t)node_idx * C;
    const float *scores = p.cand_scores + (int64_t)node_idx * C;
    int n = p.cand_count ? p.cand_count[node_idx] : C;
    if (n > C) n = C;
    if (n < 0) n = 0;
    const int maxDegree = p.maxDegree;
    int diverseBefore = p.diverse_before ? p.diverse_before[node_idx] : 0;
    if (diverseBefore < 0) diverseBefore = 0;

    // ---- stage the candidates' ordinals, scores and rows ----
    for (int i = lane; i < n; i += 64) {
        cid[i] = nodes[i];
        csc[i] = scores[i];
    }
    gs_barrier();
    {
        const int items = n * W;   // (candidate, word) over the lanes; C x W words fit LDS: far below 2^31
        for (int t = lane; t < items; t += 64) {
            const int i = t / W, w = t - i * W;
            const int32_t nd = cid[i];
            uint64_t v = 0;   // an ordinal outside the rows: never read, never scored
            if (nd >= 0 && nd < p.n) v = p.rows[(int64_t)nd * W + w];
            cc[t] = v;
        }
    }
    gs_barrier();

    unsigned long long mine = 0;   // bit t: candidate t * 64 + lane is selected
    int nSlots = 0;                // selected candidates held in the slots (== number of selected bits)
    int32_t s_pos = 0x7fffffff, s_node = -1;   // this lane's slot: candidate position, ordinal ...
    bool s_ok = false;                          // ... and whether the ordinal names a row
    auto take = [&](int i) {       // wave-uniform i
        if (lane == (i & 63)) mine |= 1ull << (i >> 6);
        const int32_t nd = cid[i];
        if (lane == nSlots) {
            s_pos = i;
            s_node = nd;
            s_ok = nd >= 0 && nd < p.n;
        }
        for (int w = lane; w < W; w += 64) ss[(size_t)w * 64 + nSlots] = cc[(size_t)i * W + w];
        nSlots++;
        gs_barrier();
    };
    // hammingDistance(candidate i's row, this lane's slot's row)
    auto hamming = [&](int i) -> int32_t {
        const uint64_t *cr = cc + (size_t)i * W;
        int32_t h = 0;
        if constexpr (WT > 0) {
            uint64_t a[WT], b[WT];
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                a[w] = ss[w * 64 + lane];
                b[w] = cr[w];
            }
#pragma unroll
            for (int w = 0; w < WT; ++w) h += gs_popc(a[w] ^ b[w]);
        } else {
            for (int w = 0; w < W; ++w) h += gs_popc(ss[(size_t)w * 64 + lane] ^ cr[w]);
        }
        return h;
    };
    {
        const int pre = diverseBefore < maxDegree ? diverseBefore : maxDegree;
        for (int i = 0; i < pre && i < n; ++i) take(i);
    }
    int nSelected = diverseBefore;
    float shortEdges = __builtin_nanf("");
    float currentAlpha = 1.0f;
    // (the host refuses alpha > BD_MAX_ALPHA; the clamp is what ends the rounds whatever the parameter block holds; NaN: no round)
    const double alphaEnd = (double)(p.alpha > BD_MAX_ALPHA ? BD_MAX_ALPHA : p.alpha) + 1E-6;
    while ((double)currentAlpha <= alphaEnd && nSelected < maxDegree) {
        for (int i = diverseBefore; i < n && nSelected < maxDegree; ++i) {
            const unsigned long long owner_bits = (unsigned long long)gs_shfl((long long)mine, i & 63);
            if ((owner_bits >> (i >> 6)) & 1ull) continue;
            const int32_t cNode = cid[i];
            const float thr = csc[i] * currentAlpha;
            const bool c_ok = cNode >= 0 && cNode < p.n;
            // ---- isDiverse ----
            const bool held = lane < nSlots;
            const bool same = held && s_node == cNode;   // node == otherNode -> break
            bool viol = false;
            if (held && !same) {
                float sim = -__builtin_inff();
                if (c_ok && s_ok) sim = 1.0f - (float)hamming(i) / fD;
                viol = sim > thr;
            }
            const uint64_t vm = gs_ballot(viol), dm = gs_ballot(same);
            bool not_diverse = vm != 0;
            if (vm != 0 && dm != 0) {   // an id listed twice: only what the walk meets before the first slot that holds it counts
                const int32_t first_same = (int32_t)gs_wave_min(same ? (long long)s_pos : (long long)0x7fffffff);
                not_diverse = gs_ballot(viol && s_pos < first_same) != 0;
            }
            if (!not_diverse) {
                if (nSlots < 64) take(i);
                nSelected++;
            }
        }
        if (currentAlpha == 1.0f) shortEdges = nSelected / (float)maxDegree;
        currentAlpha += 0.2f;
    }

    // ---- results: the selected positions in ascending order (what selected.nextSetBit iterates) ----
    gs_barrier();
    {
        int out_n = 0;
        for (int base = 0; base < n; base += 64) {
            const bool sel = ((mine >> (base >> 6)) & 1ull) != 0 && base + lane < n;
            const uint64_t m = gs_ballot(sel);
            const int pos = out_n + gs_popc(m & ((1ull << lane) - 1ull));
            if (sel && pos < maxDegree) p.selected_out[(int64_t)node_idx * maxDegree + pos] = base + lane;
            out_n += gs_popc(m);
        }
        for (int j = (out_n < maxDegree ? out_n : maxDegree) + lane; j < maxDegree; j += 64) p.selected_out[(int64_t)node_idx * maxDegree + j] = -1;
    }
    if (lane == 0) {
        p.n_selected_out[node_idx] = nSelected;
        if (p.short_edges_out) p.short_edges_out[node_idx] = shortEdges;
    }
    gs_barrier();   // the next node's staging overwrites the rows
}

// Persistent block: nodes first, first + stride, ...
template <int WT>
GS_FN void bd_worker(const BdParams &p, int first, int stride, char *lds)
{
    for (int node = first; node < p.P; node += stride) bd_node<WT>(p, node, lds);
}

}  // namespace jv
