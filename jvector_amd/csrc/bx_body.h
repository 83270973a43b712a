// bx_body.h — deleting nodes from a graph built over binary-quantized rows (bq_builder.cpp): GraphIndexBuilder.removeDeletedNodes
// (B/graph/GraphIndexBuilder.java:678-799, FreshDiskANN's consolidation) with Neighbors.replaceDeletedNeighbors
// (B/graph/ConcurrentNeighborMap.java:225-239) up to the prune, for every affected node at once.  The bodies of the kernels of
// k_bq_delete.hip, written against the wave API of gs_body.h so that the same source compiles for the lane emulator of the CPU tests
// (tests/emu/bx_emu.cpp).
//
// Affected nodes.  bx_affected_word: one wavefront per 64 nodes; for each live node (in the graph, not marked) the lanes read its
// row, one lane per entry, and one ballot says whether any entry is marked.  bx_compact: one wavefront turns that bitmap into the
// ascending list of affected nodes (popcount per word, prefix over the lanes, each lane writes its word's ids).  No atomics: the
// list is the same on every run.
//
// bx_node: one wavefront per affected node i.
//   survivors   i's unmarked entries in stored order, with their stored scores (a lane per entry, one ballot, compacted into LDS)
//   candidates  for every marked entry j of i's row (a loop over the R slots) the lanes read row j, one lane per entry, and keep the
//               ids that are not -1, not i and not marked, appended to the key array in LDS: at most R x R entries
//   scores      a lane per ENTRY: xor + popcount over the W words of its row against the node's own words (wave-uniform: scalar
//               registers for the compiled widths, LDS otherwise), into the integer key (D - h) << 32 | ~id.  Entries are scored before
//               duplicates are dropped: two entries with one id have one key, so the ONE sort that orders the candidates — bitonic, in
//               LDS, descending: higher score first, the smaller id on equal score — also brings duplicates together, and a pass over
//               neighbouring keys drops them.  That costs the row reads of the duplicates and saves a sort of its own.
//   merge       NodeArray.merge(survivors, candidates) (B/graph/NodeArray.java:63-143) without walking it: inside a run of equal
//               scores the walk emits survivor 0, candidate 0, survivor 1, candidate 1, ... and then what is left of the longer side, so
//               with p survivors and q candidates in the run, survivor r lands at offset r + min(r, q) and candidate r at r + min(r + 1, p).
//               A node is added once per run: a survivor and a candidate with one id and one score are a pair, the later of the two is
//               dropped, and every position moves up by the dropped positions before it.  Survivors find their run and their twin by
//               binary search in the sorted keys; candidates loop over the (at most R) survivors.  The f32 score 1 - (float) h / D is
//               formed once per comparison side, never inside the sort.
// Every loop is bounded by R, R x R or log2(R x R); nothing depends on the order in which waves or lanes run.
#pragma once

#include <cstdint>

#include "bx_params.h"
#include "gs_body.h"

namespace jv {

struct alignas(16) bx_w2 { uint64_t x, y; };

GS_FN bool bx_bit(const uint64_t *bits, int64_t i) { return ((bits[i >> 6] >> (i & 63)) & 1ull) != 0; }
GS_FN float bx_key_score(uint64_t key, int32_t D, float fD) { return 1.0f - (float)(D - (int32_t)(key >> 32)) / fD; }

// word w of the affected bitmap; every lane of the wave takes part
GS_FN void bx_affected_word(const BxParams &p, int64_t w)
{
    const int lane = gs_lane();
    uint64_t live = p.present[w] & ~p.marked[w];
    if ((w + 1) * 64 > p.n) live &= (p.n - w * 64 >= 64) ? ~0ull : ((1ull << (p.n - w * 64)) - 1ull);
    uint64_t word = 0;
    for (int b = 0; b < 64; ++b) {
        if (!((live >> b) & 1ull)) continue;   // wave-uniform
        const int64_t node = w * 64 + b;
        const int32_t e = lane < p.R ? p.nbrs[node * p.R + lane] : -1;
        const bool hit = e >= 0 && e < p.n && bx_bit(p.marked, e);
        if (gs_ballot(hit) != 0) word |= 1ull << b;
    }
    if (lane == 0) p.affected[w] = word;
}

// one wave: the set bits of the affected bitmap, ascending, into p.tasks; their number into p.task_count
GS_FN void bx_compact(const BxParams &p)
{
    const int lane = gs_lane();
    const int64_t words = (p.n + 63) >> 6;
    uint32_t running = 0;
    for (int64_t base = 0; base < words; base += 64) {
        const int64_t w = base + lane;
        uint64_t m = w < words ? p.affected[w] : 0ull;
        const uint32_t c = (uint32_t)gs_popc(m);
        uint32_t before = 0, total = 0;
        for (int s = 0; s < 64; ++s) {
            const uint32_t cs = gs_bcast32(c, s);
            before += s < lane ? cs : 0u;
            total += cs;
        }
        uint32_t off = running + before;
        for (int b = 0; b < 64; ++b)
            if ((m >> b) & 1ull) p.tasks[off++] = (int32_t)(w * 64 + b);
        running += total;
    }
    if (lane == 0) p.task_count[0] = running;
}

// WT > 0: rows of exactly WT words, the node's own words in registers; WT == 0: any width, the node's own words in LDS
template <int WT>
GS_FN void bx_node(const BxParams &p, int t, char *lds)
{
    const int lane = gs_lane();
    const int W = WT > 0 ? WT : p.W;
    const int R = p.R, D = p.D;
    const float fD = (float)D;
    const int cap = bx_key_capacity(R);
    uint64_t *keys = reinterpret_cast<uint64_t *>(lds);            // [cap]
    int32_t *sid = reinterpret_cast<int32_t *>(keys + cap);        // [64] survivors: ids ...
    float *ssc = reinterpret_cast<float *>(sid + 64);              // [64] ... and stored scores
    int32_t *dpos = reinterpret_cast<int32_t *>(ssc + 64);         // [64] position (before the drops) of the entry dropped for survivor u's pair
    int32_t *dcand = dpos + 64;                                    // [64] the candidate dropped for survivor u's pair, or -1
    uint64_t *qw_lds = reinterpret_cast<uint64_t *>(dcand + 64);   // [W] generic widths only
    const int32_t node = p.tasks[t];
    const uint64_t below = (1ull << lane) - 1ull;

    // ---- the node's own words ----
    const uint64_t *own = p.rows + (int64_t)node * W;
    uint64_t qw[WT > 0 ? WT : 1];
    if constexpr (WT > 0) {
#pragma unroll
        for (int w = 0; w < WT; ++w) qw[w] = own[w];
    } else {
        qw[0] = 0;
        for (int w = lane; w < W; w += 64) qw_lds[w] = own[w];
    }

    // ---- the node's row: survivors in stored order, marked entries as a mask ----
    const int32_t e = lane < R ? p.nbrs[(int64_t)node * R + lane] : -1;
    const float es = lane < R ? p.nsc[(int64_t)node * R + lane] : 0.0f;
    const bool e_ok = e >= 0 && e < p.n;
    const bool e_marked = e_ok && bx_bit(p.marked, e);
    const uint64_t sm = gs_ballot(e_ok && !e_marked), mm = gs_ballot(e_marked);
    const int S = gs_popc(sm);
    if (e_ok && !e_marked) {
        const int at = gs_popc(sm & below);
        sid[at] = e;
        ssc[at] = es;
    }

    // ---- the entries: ids in the low half of a key ----
    int E = 0;
    if (p.given) {
        const int gn = p.given_n[t] < p.G ? p.given_n[t] : p.G;
        const int32_t k = lane < gn ? p.given[(int64_t)t * p.G + lane] : -1;
        const bool ok = k >= 0 && k < p.n && k != node && !bx_bit(p.marked, k);
        const uint64_t m = gs_ballot(ok);
        if (ok) keys[gs_popc(m & below)] = (uint64_t)(uint32_t)k;
        E = gs_popc(m);
    } else {
        for (int j = 0; j < R; ++j) {
            if (!((mm >> j) & 1ull)) continue;   // wave-uniform
            const int32_t mj = (int32_t)gs_shfl((long long)e, j);
            const int32_t k = lane < R ? p.nbrs[(int64_t)mj * R + lane] : -1;
            const bool ok = k >= 0 && k < p.n && k != node && !bx_bit(p.marked, k);
            const uint64_t m = gs_ballot(ok);
            if (ok) keys[E + gs_popc(m & below)] = (uint64_t)(uint32_t)k;   // E + 64 > cap only past R marked rows of R entries
            E += gs_popc(m);
        }
    }
    gs_barrier();

    // ---- a lane per entry: the Hamming distance to the node's own row, the key ----
    int n2 = 1;
    while (n2 < E) n2 <<= 1;   // <= cap
    for (int idx = lane; idx < n2; idx += 64) {
        uint64_t key = 0;   // padding: below every key of an entry (~id has its top bit set)
        if (idx < E) {
            const int32_t k = (int32_t)(uint32_t)keys[idx];
            const uint64_t *r = p.rows + (int64_t)k * W;
            int32_t h = 0;
            if constexpr (WT > 0 && WT % 2 == 0) {
                const bx_w2 *r2 = reinterpret_cast<const bx_w2 *>(r);   // rows of an even width are 16-byte aligned
                bx_w2 v[WT / 2];
#pragma unroll
                for (int w = 0; w < WT / 2; ++w) v[w] = r2[w];
#pragma unroll
                for (int w = 0; w < WT / 2; ++w) h += gs_popc(v[w].x ^ qw[2 * w]) + gs_popc(v[w].y ^ qw[2 * w + 1]);
            } else if constexpr (WT > 0) {
                uint64_t v[WT];
#pragma unroll
                for (int w = 0; w < WT; ++w) v[w] = r[w];
#pragma unroll
                for (int w = 0; w < WT; ++w) h += gs_popc(v[w] ^ qw[w]);
            } else if ((W & 1) == 0) {
                const bx_w2 *r2 = reinterpret_cast<const bx_w2 *>(r);
                for (int w = 0; w < W; w += 2) {
                    const bx_w2 v = r2[w >> 1];
                    h += gs_popc(v.x ^ qw_lds[w]) + gs_popc(v.y ^ qw_lds[w + 1]);
                }
            } else {
                for (int w = 0; w < W; ++w) h += gs_popc(r[w] ^ qw_lds[w]);
            }
            key = ((uint64_t)(uint32_t)(D - h) << 32) | (uint64_t)(uint32_t)(~k);
        }
        keys[idx] = key;
    }
    gs_barrier();

    // ---- bitonic sort, descending ----
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = lane; x < (n2 >> 1); x += 64) {
                const int a = ((x & ~(j - 1)) << 1) | (x & (j - 1)), b = a | j;
                const uint64_t ka = keys[a], kb = keys[b];
                if ((ka < kb) == ((a & k) == 0)) {
                    keys[a] = kb;
                    keys[b] = ka;
                }
            }
            gs_barrier();
        }
    }

    // ---- equal neighbours are one candidate: compacted in place, a chunk of 64 read before it is written ----
    int Cn = 0;
    {
        uint64_t carry = ~0ull;   // no key: a key's upper half is at most D
        for (int base = 0; base < E; base += 64) {
            const int idx = base + lane;
            const uint64_t x = idx < E ? keys[idx] : 0ull;
            const uint64_t prev = lane == 0 ? carry : (idx < E ? keys[idx - 1] : 0ull);
            const bool first = idx < E && x != prev;
            const uint64_t m = gs_ballot(first);
            carry = (uint64_t)gs_shfl((long long)x, 63);
            gs_barrier();
            if (first) keys[Cn + gs_popc(m & below)] = x;
            Cn += gs_popc(m);
            gs_barrier();
        }
    }

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
                if (bx_key_score(keys[mid], D, fD) > su) lo = mid + 1;
                else hi = mid;
            }
            if (lo2 < hi2) {
                const int mid = (lo2 + hi2) >> 1;
                if (bx_key_score(keys[mid], D, fD) >= su) lo2 = mid + 1;
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
                if ((uint32_t)keys[mid] > want) lo = mid + 1;
                else hi = mid;
            }
        }
        if (is_s && lo < cge && (uint32_t)keys[lo] == want) twin = lo;
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
        const uint64_t key = keys[c];
        const float sc = bx_key_score(key, D, fD);
        int lo = 0, hi = c;   // the first candidate of this one's run: keys at or above (upper half, all ones)
        const uint64_t run_top = key | 0xFFFFFFFFull;
        for (int span = cap; span > 0; span >>= 1) {
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[mid] > run_top) lo = mid + 1;
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
                out[at] = (int32_t)~(uint32_t)key;
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
template <int WT>
GS_FN void bx_worker(const BxParams &p, int first, int stride, char *lds)
{
    for (int t = first; t < p.P; t += stride) bx_node<WT>(p, t, lds);
}

}  // namespace jv
