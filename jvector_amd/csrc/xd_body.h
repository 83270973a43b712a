// xd_body.h — deleting nodes from a graph built over float rows (exact_builder.cpp): GraphIndexBuilder.removeDeletedNodes
// (B/graph/GraphIndexBuilder.java:678-799) with Neighbors.replaceDeletedNeighbors (B/graph/ConcurrentNeighborMap.java:225-239) up to the
// prune, for every affected node at once.  The body of exact_delete_merge_kernel (k_exact_delete.hip).  The affected-node list, the
// bitmaps and the retire step are bx_body.h's: they never look at a score.
//
// xd_node: one wavefront per affected node i.
//   survivors   i's unmarked entries in stored order, with their stored scores (a lane per entry, one ballot, compacted into LDS)
//   gather      for every marked entry j of i's row (a loop over the R slots) the lanes read row j of the adjacency, one lane per entry,
//               and append the ids that are not -1, not i and not marked to a 32-bit id array in LDS: at most R x R ids.  IDS ONLY: no
//               float row is touched yet.
//   distinct    the ids are sorted (bitonic, ascending, 32-bit keys), the head of each run of equal ids is flagged and the heads are
//               prefix-compacted in place.  This is bx_body.h's order of work turned round: there a score is a few popcounts, so the
//               duplicates are scored and the score sort drops them; here a duplicate would cost 4 D bytes of HBM and a D-long dependent
//               add chain, so it is dropped before anything is scored.
//   scores      64 distinct candidates per pass, one lane per row, through xg_body.h's LDS row tile (xg_tr_rows; 32 x 128 or 16 x 256
//               for a short last group, chosen as xg_score_group chooses) with the node's OWN row as the wave-uniform operand, read
//               through scalar loads; rows that are not 16-byte aligned or D % 8 != 0: a lane walks its own candidate row (exact_row /
//               cosine_row).  COSINE takes both norms from the per-row table, which adds in query_sqnorm_kernel's order.  So a score has
//               the bits of jv_hip_exact_pair_scores(node1 = i, node2 = k).  It goes into NodeQueue's key sortableInt(score) << 32 | ~id.
//               The key array is the id array's own LDS: key x overwrites ids 2 x - capacity and 2 x + 1 - capacity, both at or below
//               x, and a pass has its 64 ids in registers before it writes a key.
//   order       ONE bitonic sort of the keys, descending (higher score first, the smaller id on equal score), over the next power of
//               two at or above the DISTINCT count.
//   merge       NodeArray.merge(survivors, candidates) in closed form, as bx_body.h documents it: in a run of equal scores with p
//               survivors and q candidates survivor r lands at offset r + min(r, q), candidate r at r + min(r + 1, p); of a survivor
//               and a candidate with one id and one score the later one is dropped, positions move up by the drops before them.
//               Scores are compared as f32.  (No similarity function gives -0.0 — 1 + x is +0.0 when it is zero, 1 / (1 + d) is
//               positive — so a run of equal f32 scores is a run of equal upper key halves.)
// Every loop is bounded by R, R x R or log2(R x R); nothing depends on the order in which waves or lanes run.
#pragma once

#include <cstdint>

#include "xd_params.h"
#include "xg_body.h"

namespace jv {

GS_FN bool xd_bit(const uint64_t *bits, int64_t i) { return ((bits[i >> 6] >> (i & 63)) & 1ull) != 0; }

// VectorSimilarityFunction.compare(row `node`, row my_node) for a group of cnt rows, lane j < cnt holding the j-th (others -1); `node` is
// wave-uniform, nnorm its sum of squares (COSINE)
template <int VSF, bool TR>
GS_FN float xd_score_group(const XdParams &p, int32_t node, float nnorm, int32_t my_node, int cnt, float *tile)
{
    const int D = p.D;
    float raw = 0.0f;
    if (TR) {
        xg_cfloat *a = (xg_cfloat *)(p.rows + (int64_t)node * D);
        if (cnt <= 16 && D > 128) raw = xg_tr_rows<VSF, 16, 256>(p.rows, D, my_node, cnt, a, tile);
        else if (cnt <= 32 && D > 64) raw = xg_tr_rows<VSF, 32, 128>(p.rows, D, my_node, cnt, a, tile);
        else raw = xg_tr_rows<VSF, 64, 64>(p.rows, D, my_node, cnt, a, tile);
        if (VSF == VSF_COS && my_node >= 0) raw = cosine_finish(raw, nnorm, p.vnorm[my_node]);
    } else if (my_node >= 0) {
        const float *a = p.rows + (int64_t)node * D;
        const float *b = p.rows + (int64_t)my_node * D;
        if (VSF == VSF_COS) {
            float sum, norm2;
            cosine_row(a, b, D, sum, norm2);
            raw = cosine_finish(sum, nnorm, norm2);
        } else {
            raw = exact_row<VSF>(a, b, D);
        }
    }
    return score_from_raw(VSF, raw);
}

// bitonic sort of a[0 .. n2), n2 a power of two; DESC: descending
template <bool DESC, class T>
GS_FN void xd_sort(T *a, int n2)
{
    const int lane = gs_lane();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = lane; x < (n2 >> 1); x += 64) {
                const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
                const T va = a[lo], vb = a[hi];
                if ((DESC ? va < vb : va > vb) == ((lo & k) == 0)) {
                    a[lo] = vb;
                    a[hi] = va;
                }
            }
            gs_barrier();
        }
    }
}

template <int VSF, bool TR>
GS_FN void xd_node(const XdParams &p, int t, char *lds)
{
    const int lane = gs_lane();
    const int R = p.R;
    const int cap = xd_capacity(R);
    float *tile = reinterpret_cast<float *>(lds);                           // [XG_TILE_FLOATS] (first: its b128 accesses want 16 bytes)
    long long *keys = reinterpret_cast<long long *>(tile + XG_TILE_FLOATS);   // [cap]
    uint32_t *ids = reinterpret_cast<uint32_t *>(keys) + cap;               // [cap] the upper half of the key array
    int32_t *sid = reinterpret_cast<int32_t *>(keys + cap);                 // [64] survivors: ids ...
    float *ssc = reinterpret_cast<float *>(sid + 64);                       // [64] ... and stored scores
    int32_t *dpos = reinterpret_cast<int32_t *>(ssc + 64);                  // [64] position (before the drops) of the entry dropped for survivor u's pair
    int32_t *dcand = dpos + 64;                                             // [64] the candidate dropped for survivor u's pair, or -1
    const int32_t node = gs_uniform(p.tasks[t]);
    const uint64_t below = (1ull << lane) - 1ull;
    if (node < 0 || node >= p.n) {   // (the host's list holds affected nodes only; nothing outside the rows is ever read)
        if (lane == 0) {
            p.ln[t] = p.cn[t] = 0;
            if (p.rn) p.rn[t] = 0;
        }
        return;
    }

    // ---- the node's row: survivors in stored order, marked entries as a mask ----
    const int32_t e = lane < R ? p.nbrs[(int64_t)node * R + lane] : -1;
    const float es = lane < R ? p.nsc[(int64_t)node * R + lane] : 0.0f;
    const bool e_ok = e >= 0 && e < p.n;
    const bool e_marked = e_ok && xd_bit(p.marked, e);
    const uint64_t sm = gs_ballot(e_ok && !e_marked), mm = gs_ballot(e_marked);
    const int S = gs_popc(sm);
    if (e_ok && !e_marked) {
        const int at = gs_popc(sm & below);
        sid[at] = e;
        ssc[at] = es;
    }

    // ---- the two-hop ids, duplicates and all ----
    int E = 0;
    if (p.given) {
        const int gn = p.given_n[t] < p.G ? p.given_n[t] : p.G;
        const int32_t k = lane < gn ? p.given[(int64_t)t * p.G + lane] : -1;
        const bool ok = k >= 0 && k < p.n && k != node && !xd_bit(p.marked, k);
        const uint64_t m = gs_ballot(ok);
        if (ok) ids[gs_popc(m & below)] = (uint32_t)k;
        E = gs_popc(m);
    } else {
        for (int j = 0; j < R; ++j) {
            if (!((mm >> j) & 1ull)) continue;   // wave-uniform
            const int32_t mj = (int32_t)gs_bcast32((uint32_t)e, j);
            const int32_t k = lane < R ? p.nbrs[(int64_t)mj * R + lane] : -1;
            const bool ok = k >= 0 && k < p.n && k != node && !xd_bit(p.marked, k);
            const uint64_t m = gs_ballot(ok);
            if (ok) ids[E + gs_popc(m & below)] = (uint32_t)k;   // E + R <= R x R <= cap: at most R marked rows of R entries
            E += gs_popc(m);
        }
    }
    int n2 = 1;
    while (n2 < E) n2 <<= 1;   // <= cap
    for (int idx = E + lane; idx < n2; idx += 64) ids[idx] = 0xFFFFFFFFu;   // padding: above every id
    gs_barrier();

    // ---- distinct ids, ascending: sort, flag the head of each run, compact the heads in place (a chunk of 64 read before it is written) ----
    xd_sort<false>(ids, n2);
    int Cn = 0;
    {
        uint32_t carry = 0xFFFFFFFFu;   // no id
        for (int base = 0; base < E; base += 64) {
            const int idx = base + lane;
            const uint32_t x = idx < E ? ids[idx] : 0u;
            const uint32_t prev = lane == 0 ? carry : (idx < E ? ids[idx - 1] : 0u);
            const bool first = idx < E && x != prev;
            const uint64_t m = gs_ballot(first);
            carry = gs_bcast32(x, 63);
            gs_barrier();
            if (first) ids[Cn + gs_popc(m & below)] = x;
            Cn += gs_popc(m);
            gs_barrier();
        }
    }

    // ---- 64 distinct candidates per pass, a lane per row: the score, the key ----
    float nnorm = 0.0f;
    if (VSF == VSF_COS) nnorm = p.vnorm[node];
    int n2k = 1;
    while (n2k < Cn) n2k <<= 1;   // <= cap
    for (int base = 0; base < Cn; base += 64) {
        const int idx = base + lane;
        const int cnt = Cn - base < 64 ? Cn - base : 64;
        const int32_t mine = idx < Cn ? (int32_t)ids[idx] : -1;
        gs_barrier();   // the pass's ids are in registers: its keys may overwrite them
        const float sc = xd_score_group<VSF, TR>(p, node, nnorm, mine, cnt, tile);
        if (mine >= 0) keys[idx] = gs_key(mine, sc);
    }
    for (int idx = Cn + lane; idx < n2k; idx += 64) keys[idx] = GS_KEY_MIN;   // padding: below every key
    gs_barrier();

    // ---- NodeQueue order ----
    xd_sort<true>(keys, n2k);

    // ---- survivors: run, twin, the dropped half of the pair ----
    const bool is_s = lane < S;
    const float su = is_s ? ssc[lane] : 0.0f;
    const int32_t my_id = is_s ? sid[lane] : -1;
    int gt = 0, r1 = 0, pp = 0;   // survivors above / equal before this one / equal
    for (int v = 0; v < S; ++v) {
        const float sv = ssc[v];
        gt += sv > su ? 1 : 0;
        r1 += (sv == su && v < lane) ? 1 : 0;
        pp += sv == su ? 1 : 0;
    }
    int cgt = 0, cge = 0;   // candidates above / not below
    {
        int lo = 0, hi = Cn, lo2 = 0, hi2 = Cn;
        for (int span = cap; span > 0; span >>= 1) {
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (gs_key_score(keys[mid]) > su) lo = mid + 1;
                else hi = mid;
            }
            if (lo2 < hi2) {
                const int mid = (lo2 + hi2) >> 1;
                if (gs_key_score(keys[mid]) >= su) lo2 = mid + 1;
                else hi2 = mid;
            }
        }
        cgt = lo;
        cge = lo2;
    }
    const int q = cge - cgt;
    int twin = -1;
    {
        const uint32_t want = (uint32_t)(~my_id);   // inside a run the lower halves descend
        int lo = cgt, hi = cge;
        for (int span = cap; span > 0; span >>= 1) {
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((uint32_t)(unsigned long long)keys[mid] > want) lo = mid + 1;
                else hi = mid;
            }
        }
        if (is_s && lo < cge && (uint32_t)(unsigned long long)keys[lo] == want) twin = lo;
    }
    const int pos_s = lane + cgt + (r1 < q ? r1 : q);
    bool s_dropped = false;
    {
        int32_t dp = 0x7fffffff, dc = -1;
        if (twin >= 0) {
            const int r2 = twin - cgt;
            const int off_s = r1 + (r1 < q ? r1 : q), off_c = r2 + (r2 + 1 < pp ? r2 + 1 : pp);
            const int pos_c = twin + gt + (r2 + 1 < pp ? r2 + 1 : pp);
            if (off_s < off_c) {
                dp = pos_c;
                dc = twin;
            } else {
                dp = pos_s;
                s_dropped = true;
            }
        }
        dpos[lane] = dp;
        dcand[lane] = dc;
    }
    const int drops = gs_popc(gs_ballot(twin >= 0));
    const int M = S + Cn - drops;
    gs_barrier();
    if (lane == 0) {
        p.ln[t] = M;
        p.cn[t] = Cn;
        if (p.rn) p.rn[t] = E;
    }
    if (!p.list) {
        gs_barrier();   // the next node's staging overwrites the block
        return;
    }

    // ---- the merged list ----
    int32_t *out = p.list + (int64_t)t * p.L;
    float *osc = p.lsc + (int64_t)t * p.L;
    if (is_s && !s_dropped) {
        int at = pos_s;
        for (int v = 0; v < S; ++v) at -= dpos[v] < pos_s ? 1 : 0;
        if (at >= 0 && at < p.L) {
            out[at] = my_id;
            osc[at] = su;
        }
    }
    for (int c = lane; c < Cn; c += 64) {
        const long long key = keys[c];
        const float sc = gs_key_score(key);
        int lo = 0, hi = c;   // the first candidate of this one's run
        for (int span = cap; span > 0; span >>= 1) {
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (gs_key_score(keys[mid]) > sc) lo = mid + 1;
                else hi = mid;
            }
        }
        const int r2 = c - lo;
        int gts = 0, eqs = 0;
        bool dropped = false;
        for (int v = 0; v < S; ++v) {
            const float sv = ssc[v];
            gts += sv > sc ? 1 : 0;
            eqs += sv == sc ? 1 : 0;
            dropped = dropped || dcand[v] == c;
        }
        const int pos_c = c + gts + (r2 + 1 < eqs ? r2 + 1 : eqs);
        if (!dropped) {
            int at = pos_c;
            for (int v = 0; v < S; ++v) at -= dpos[v] < pos_c ? 1 : 0;
            if (at >= 0 && at < p.L) {
                out[at] = gs_key_node(key);
                osc[at] = sc;
            }
        }
    }
    for (int x = (M > 0 ? M : 0) + lane; x < p.L; x += 64) {
        out[x] = -1;
        osc[x] = 0.0f;
    }
    gs_barrier();   // the next node's staging overwrites the block
}

// Persistent block: tasks first, first + stride, ...
template <int VSF, bool TR>
GS_FN void xd_worker(const XdParams &p, int first, int stride, char *lds)
{
    for (int t = first; t < p.P; t += stride) xd_node<VSF, TR>(p, t, lds);
}

}  // namespace jv
