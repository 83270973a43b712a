// xb_body.h — batched robust prune with EXACT scores: VamanaDiversityProvider.retainDiverse
// (B/graph/diversity/VamanaDiversityProvider.java:45-96) for P nodes at once with the diversity score of
// BuildScoreProvider.randomAccessScoreProvider (B/graph/similarity/BuildScoreProvider.java:106-160): VectorSimilarityFunction.compare
// on two float rows.  The body of exact_retain_kernel (k_exact_retain.hip).  bd_body.h is its BQ twin, and NOT its template: float rows
// do not fit LDS (64 selected rows at D = 768 are 192 KB) and the chain over D is serial per pair.
//
// One 64-lane wavefront per node.  Lanes own CANDIDATES (lane l owns positions l, l + 64, ...), not selected slots.
//
// Score when selected, not when tested.  When position j is selected its row becomes the wave-uniform operand, read through the
// constant address space (scalar loads into SGPR operands, as xg_body.h reads the query), and every still-unselected candidate is
// scored against it, one lane per candidate row: each (candidate, selected) pair is computed once over all alpha rounds with all
// lanes busy, where a lane per slot runs at nSlots / 64.  The scores go to an LDS matrix pm[slot][Cp] (Cp = C rounded up to 64:
// lane-consecutive candidates read consecutive words — conflict-free).
//
// Operand roles.  The reference scores diversityScoreFunctionFor(cand).similarityTo(other): cand is compare's first operand.  Here the
// roles are SWAPPED — `other` (the selected row) is the uniform operand a[], cand the lane's row — and the bits are the same:
//   dot     dot8 / the front remainder add the products a[i] * b[i] in ascending i; a product commutes.
//   L2      l28 / the tail square d = a[i] - b[i]; b[i] - a[i] is -d exactly and (-d) * (-d) = d * d.
//   cosine  `sum` adds a[i] * b[i] in ascending i; the two norms are sequential sums of e * e over one row each, whichever side the
//           row stands on (query_sqnorm_kernel, row_sqnorm_kernel, cosine_row and tr_rows add in the same order), and cosine_finish
//           multiplies them in f32 first: that product commutes.
// So pair(cand, other) carries the bits of jv_hip_exact_pair_scores(node1 = cand, node2 = other).
//
// Row movement (xb_score_rows).  As xg_body.h's rows: a chunk of 64 floats of each of up to 64 rows, 16 bytes per lane and 16 lanes
// per row (whole 128-byte lines), parked in one LDS tile [64][64 + 4]; only the load instructions that carry a live candidate are
// issued; the loads of chunk c + 1 wait in registers while lane j walks row j of chunk c with ds_read_b128.  The chains' structure
// survives the chunking: dot's front remainder (D % 8 elements, one by one) is added first, straight from the lane's own row, and the
// chunks start BEHIND it, so every chunk is a whole number of dot8 blocks; L2's chunks start at 0 and its tail (D % 8) falls at the
// end of the last chunk; cosine is one running sum.  Rows that are not 16-byte aligned (D % 4 != 0) fill the tile with dword loads,
// a row per instruction.
//
// Selection.  Each candidate keeps, per lane and group, a "selected" bit and a "violated at this alpha" bit, and in LDS its own-id stop:
// the lowest selected position that holds its own node id (isDiverse walks the selected positions in ascending order and breaks
// there).  Violated(i) = some slot s with pos(s) < stop(i) and pm[s][i] > score(i) * currentAlpha.  The bit is updated from the
// new slot alone, and rebuilt from the matrix at the start of a round (the threshold moved) and when a selection at a lower position
// with the candidate's own id moves the stop.  A round is then "ballot, first diverse unselected position at or after the cursor,
// select, score": as many steps as selections.  Between two selections the selected set does not change, so the candidates the ballot
// skips are exactly the ones the sequential loop would have tested and rejected.
#pragma once

#include <cstdint>

#include "xb_params.h"
#include "gs_body.h"
#include "xc_chain.h"

namespace jv {

typedef const __attribute__((address_space(4))) float xb_cfloat;   // wave-uniform, never written while the kernel runs: s_load

// the chain over `len` floats of the lane's row in the tile against the uniform slice a[]: 8-blocks, then single elements
template <int VSF>
GS_FN void xb_chunk(const float *row, xb_cfloat *a, int len, float &acc)
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
    if (len == 64) {
#pragma unroll 8
        for (int i = 0; i < 64; i += 8) block(i);
        return;
    }
    int i = 0;
    for (; i + 8 <= len; i += 8) block(i);
    for (; i < len; ++i) {   // L2's tail, cosine's last elements (dot: every chunk is whole blocks)
        if (VSF == VSF_L2) {
            const float d = a[i] - row[i];
            acc += d * d;
        } else {
            acc += a[i] * row[i];
        }
    }
}

// Raw chain value of the uniform row a[0 .. D) against row my_node of every lane (-1: no row).  Wave-uniform control flow: every
// lane takes part in the loads.  AL: rows 16-byte aligned (D % 4 == 0).
template <int VSF, bool AL>
GS_FN float xb_score_rows(const float *rows, int D, int32_t my_node, xb_cfloat *a, float *tile)
{
    constexpr int LS = 68;
    const int lane = gs_lane();
    const uint64_t live = gs_ballot(my_node >= 0);
    const int org = VSF == VSF_DOT ? D % 8 : 0;   // dot: the front remainder first, the 8-blocks behind it
    float acc = 0.0f;
    if (VSF == VSF_DOT && org > 0 && my_node >= 0) {
        const float *b = rows + (int64_t)my_node * D;
        for (int i = 0; i < org; ++i) acc += b[i] * a[i];
    }
    const int L = D - org;
    const int nc = (L + 63) / 64;
    if (nc == 0) return acc;
    if (AL) {
        const int seg = (lane & 15) * 4;   // this lane's 16 bytes inside a row's chunk
        const int sub = lane >> 4;         // load instruction k fetches rows 4 k + sub
        int32_t rn[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) rn[k] = gs_shfl32(my_node, 4 * k + sub);
        float4 r[16];
        auto issue = [&](int c) {
            const bool in = c * 64 + seg < L;   // (L % 4 == 0: a lane's 16 bytes lie wholly inside the row or wholly outside)
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if ((live >> (4 * k)) & 0xFull)   // (wave-uniform: instructions whose four rows are all dead are not issued)
                    r[k] = (rn[k] >= 0 && in) ? *reinterpret_cast<const float4 *>(rows + (int64_t)rn[k] * D + org + c * 64 + seg) : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        issue(0);
        for (int c = 0; c < nc; ++c) {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if ((live >> (4 * k)) & 0xFull) *reinterpret_cast<float4 *>(tile + (4 * k + sub) * LS + seg) = r[k];
            gs_barrier();
            if (c + 1 < nc) issue(c + 1);
            const int len = (L - c * 64 < 64) ? (L - c * 64) : 64;
            if (my_node >= 0) xb_chunk<VSF>(tile + lane * LS, a + org + c * 64, len, acc);
            gs_barrier();
        }
    } else {
        for (int c = 0; c < nc; ++c) {
            const int col = c * 64 + lane;
            for (int rr = 0; rr < 64; ++rr) {
                if (!((live >> rr) & 1ull)) continue;   // (wave-uniform)
                const int32_t nd = __builtin_amdgcn_readlane(my_node, rr);
                tile[rr * LS + lane] = col < L ? rows[(int64_t)nd * D + org + col] : 0.0f;
            }
            gs_barrier();
            const int len = (L - c * 64 < 64) ? (L - c * 64) : 64;
            if (my_node >= 0) xb_chunk<VSF>(tile + lane * LS, a + org + c * 64, len, acc);
            gs_barrier();
        }
    }
    return acc;
}

// One node.
template <int VSF, bool AL>
GS_FN void xb_node(const XbParams &p, int node_idx, char *lds)
{
    const int lane = gs_lane();
    const int C = p.C, Cp = xb_padded(C);
    // LDS: [score tile][pair matrix slots x Cp][ids Cp][scores Cp][squared norms Cp][own-id stops Cp][slot positions 64]
    float *tile = reinterpret_cast<float *>(lds);
    float *pm = tile + XB_TILE_FLOATS;
    int32_t *cid = reinterpret_cast<int32_t *>(pm + (size_t)xb_slots(C, p.maxDegree) * Cp);
    float *csc = reinterpret_cast<float *>(cid + Cp);
    float *cnm = csc + Cp;
    int32_t *stop = reinterpret_cast<int32_t *>(cnm + Cp);
    int32_t *spos = stop + Cp;
    const int32_t *nodes = p.cand_nodes + (int64_t)node_idx * C;
    const float *scores = p.cand_scores + (int64_t)node_idx * C;
    int n = p.cand_count ? p.cand_count[node_idx] : C;
    if (n > C) n = C;
    if (n < 0) n = 0;
    n = gs_uniform(n);
    const int maxDegree = p.maxDegree;
    int diverseBefore = p.diverse_before ? p.diverse_before[node_idx] : 0;
    if (diverseBefore < 0) diverseBefore = 0;
    diverseBefore = gs_uniform(diverseBefore);
    const int G = (n + 63) >> 6;   // groups of 64 candidates; bit g of a lane's masks is candidate g * 64 + lane

    // ---- stage the candidates' ordinals, scores and (cosine) squared norms: computed once per row by launch_row_sqnorms ----
    for (int i = lane; i < n; i += 64) {
        const int32_t nd = nodes[i];
        cid[i] = nd;
        csc[i] = scores[i];
        cnm[i] = (VSF == VSF_COS && nd >= 0 && nd < p.n) ? p.vnorm[nd] : 0.0f;
        stop[i] = 0x7fffffff;
    }
    gs_barrier();

    uint32_t selb = 0, violb = 0;
    int nSlots = 0;
    float currentAlpha = 1.0f;
    // (the host refuses alpha > XB_MAX_ALPHA; the clamp is what ends the rounds whatever the parameter block holds; NaN: no round)
    const double alphaEnd = (double)(p.alpha > XB_MAX_ALPHA ? XB_MAX_ALPHA : p.alpha) + 1E-6;
    const bool runs = 1.0 <= alphaEnd && diverseBefore < maxDegree;   // will isDiverse ever be asked?

    // the violated bit of candidate c (group g) from the matrix: slots below its own-id stop against its threshold (lane-local)
    auto rebuild = [&](int c, int g) {
        const int32_t st = stop[c];
        const float thr = csc[c] * currentAlpha;
        bool v = false;
        for (int s = 0; s < nSlots; ++s) v |= spos[s] < st && pm[(size_t)s * Cp + c] > thr;
        violb = (violb & ~(1u << g)) | (v ? (1u << g) : 0u);
    };
    // position i (wave-uniform) joins the selected set; score: every unselected candidate against its row
    auto take = [&](int i, bool score) {
        if (lane == (i & 63)) selb |= 1u << (i >> 6);
        const int s = nSlots;
        if (lane == 0) spos[s] = i;
        nSlots++;
        gs_barrier();
        if (!score) return;
        const int32_t snode = gs_uniform(cid[i]);
        const bool s_ok = snode >= 0 && snode < p.n;
        const float snorm = cnm[i];
        xb_cfloat *a = (xb_cfloat *)(p.rows + (int64_t)(s_ok ? snode : 0) * p.D);
        for (int g = 0; g < G; ++g) {
            const int c = g * 64 + lane;
            const bool act = c < n && !((selb >> g) & 1u);
            if (gs_ballot(act) == 0) continue;
            const int32_t cn = act ? cid[c] : -1;
            const bool c_ok = act && cn >= 0 && cn < p.n;
            float sim = -__builtin_inff();   // an ordinal outside the rows on either side
            if (s_ok) {
                const float raw0 = xb_score_rows<VSF, AL>(p.rows, p.D, c_ok ? cn : -1, a, tile);
                if (c_ok) sim = score_from_raw(VSF, VSF == VSF_COS ? cosine_finish(raw0, cnm[c], snorm) : raw0);
            }
            if (act) {
                pm[(size_t)s * Cp + c] = sim;
                const int32_t st = stop[c];
                if (cn == snode) {   // node == otherNode -> break: the walk of this candidate now ends at position i, if that is lower
                    if (i < st) {
                        stop[c] = i;
                        rebuild(c, g);
                    }
                } else if (i < st && sim > csc[c] * currentAlpha) {
                    violb |= 1u << g;
                }
            }
        }
        gs_barrier();
    };

    {
        const int pre = diverseBefore < maxDegree ? diverseBefore : maxDegree;
        for (int i = 0; i < pre && i < n; ++i)   // all of them first: a position that is about to be set is not scored as a candidate
            if (lane == (i & 63)) selb |= 1u << (i >> 6);
        for (int i = 0; i < pre && i < n; ++i) take(i, runs);
    }
    int nSelected = diverseBefore;
    float shortEdges = __builtin_nanf("");
    while ((double)currentAlpha <= alphaEnd && nSelected < maxDegree) {
        for (int g = 0; g < G; ++g) {   // the thresholds moved: every live candidate's bit from the matrix
            const int c = g * 64 + lane;
            if (c < n && !((selb >> g) & 1u)) rebuild(c, g);
        }
        int cursor = diverseBefore;
        while (nSelected < maxDegree && cursor < n) {
            int found = -1;   // the first unselected, diverse position at or after the cursor
            for (int g = cursor >> 6; g < G; ++g) {
                const int c = g * 64 + lane;
                const uint64_t m = gs_ballot(c >= cursor && c < n && !((selb >> g) & 1u) && !((violb >> g) & 1u));
                if (m) {
                    found = g * 64 + gs_first(m);
                    break;
                }
            }
            if (found < 0) break;
            nSelected++;
            take(found, nSelected < maxDegree);   // (after the last selection nothing is tested again)
            cursor = found + 1;
        }
        if (currentAlpha == 1.0f) shortEdges = nSelected / (float)maxDegree;
        currentAlpha += 0.2f;
    }

    // ---- results: the selected positions in ascending order (what selected.nextSetBit iterates) ----
    gs_barrier();
    {
        int out_n = 0;
        for (int g = 0; g < G; ++g) {
            const bool sel = ((selb >> g) & 1u) != 0;
            const uint64_t m = gs_ballot(sel);
            const int pos = out_n + gs_popc(m & ((1ull << lane) - 1ull));
            if (sel && pos < maxDegree) p.selected_out[(int64_t)node_idx * maxDegree + pos] = g * 64 + lane;
            out_n += gs_popc(m);
        }
        for (int j = (out_n < maxDegree ? out_n : maxDegree) + lane; j < maxDegree; j += 64) p.selected_out[(int64_t)node_idx * maxDegree + j] = -1;
    }
    if (lane == 0) {
        p.n_selected_out[node_idx] = nSelected;
        if (p.short_edges_out) p.short_edges_out[node_idx] = shortEdges;
    }
    gs_barrier();   // the next node's staging overwrites the lists
}

// Persistent block: nodes first, first + stride, ...
template <int VSF, bool AL>
GS_FN void xb_worker(const XbParams &p, int first, int stride, char *lds)
{
    for (int node = first; node < p.P; node += stride) xb_node<VSF, AL>(p, node, lds);
}

}  // namespace jv
