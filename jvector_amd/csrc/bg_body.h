// bg_body.h — device-resident graph traversal over binary-quantized vectors: one 64-lane wavefront runs one query's whole
// GraphSearcher loop with BQVectors.scoreFunctionFor as the approximate score.  The body of bq_graph_search_kernel
// (k_bq_gsearch.hip), written against the wave API of gs_body.h so that the same source compiles for the lane emulator of the
// CPU tests (tests/emu/bg_emu.cpp).
//
// What it computes is GraphSearcher.search(DefaultSearchScoreProvider(bqv.scoreFunctionFor(q, vsf), reranker), topK, rerankK, 0, 0,
// acceptOrds) up to the rerank (B/graph/GraphSearcher.java:263-282 internalSearch, 334-353 initializeInternal, 355-369 stopSearch,
// 406-457 searchOneLayer, 324-331 setEntryPointsFromPreviousLayer, 515-530 addTopCandidate): the kept approximate results, their
// BQ similarities, visitedCount and expandedCount.
//
// Scores.  BQVectors.similarityBetween = 1 - (float) hamming / D is strictly decreasing in the Hamming distance for every D the
// library takes (<= 16383), so the queues hold INTEGER keys: (D - hamming) << 32 | ~node — NodeQueue's order (higher score first,
// the smaller node id on equal score) without a float in the loop.  The f32 formula is applied once, when the results leave.
// A lane scores one neighbour: W 64-bit words of its row (16-byte loads when W is even: rows are then 16-byte aligned, else
// 8-byte loads) against the query's words, v_xor_b32 + v_bcnt_u32_b32 into one integer.  The query's words are wave-uniform: for the
// compiled row widths (WT > 0) they are read through a uniform address into scalar registers, else they sit in LDS.
//
// Traversal state.  gs_body.h's pieces, restated where they were tied to the PQ launch parameters:
//   candidates  an LDS tier of cand_cap keys over a spill tier in global memory (partition at the median of 64 samples, refill when
//               the LDS tier runs dry): bg_partition / bg_refill / bg_push are gs_partition / gs_refill / gs_push over a capacity
//               instead of a GsParams.  At level 0 a fresh neighbour strictly below the worst of a FULL result list is not queued:
//               the result minimum only grows, stopSearch would fire before it could ever be popped.
//   results     LDS array of rerankK keys + cached minimum (rescan on replace).
//   evicted     (levels above 0) kept at the END of the worker's spill slice, growing downwards: no LDS, and one capacity.
//   visited     FAST form: an open-addressing table of 1 << vcap_log2 node ids, kept at most half full — in LDS up to
//               BG_VIS_LDS_MAX_LOG2, else in the worker's slice of global memory.  SAFE form: a bitmap of n_nodes bits in global memory.
// A query that outgrows the FAST form's table or spill slice leaves with GS_OVERFLOW and no results; the host runs it again in
// the SAFE form, whose structures hold every node of the graph (spill slice of n_nodes + 64 keys: a node is in at most one of
// candidates / results / evicted).  Both forms make the same comparisons, so the answers are identical.
#pragma once

#include <cstdint>

#include "bg_params.h"
#include "gs_body.h"

namespace jv {

struct alignas(16) bg_w2 { uint64_t x, y; };

GS_FN long long bg_key(int32_t node, int32_t closeness) { return (long long)(((unsigned long long)(uint32_t)closeness << 32) | (unsigned long long)(uint32_t)(~node)); }
GS_FN int32_t bg_key_hi(long long k) { return (int32_t)(k >> 32); }

// visited.add on the LDS table: gs_visit with an LDS atomic
GS_FN bool bg_visit_lds(uint32_t *tab, uint32_t mask, int shift, int32_t node)
{
    uint32_t h = ((uint32_t)node * 0x9E3779B1u) >> shift;
    for (;;) {
        const uint32_t old = gs_lds_cas(tab + h, 0xFFFFFFFFu, (uint32_t)node);
        if (old == 0xFFFFFFFFu) return true;
        if (old == (uint32_t)node) return false;
        h = (h + 1) & mask;
    }
}

// visited.add on the bitmap: set bit `node`, true iff it was clear
GS_FN bool bg_visit_bits(uint32_t *bm, int32_t node)
{
    int32_t *w = reinterpret_cast<int32_t *>(bm) + (node >> 5);
    const int32_t bit = (int32_t)(1u << (node & 31));
    int32_t expect = 0;
    for (;;) {
        const int32_t old = gs_cas(w, expect, expect | bit);
        if (old == expect) return true;
        if (old & bit) return false;
        expect = old;
    }
}

// gs_partition over a capacity: every LDS-tier key <= the median of 64 samples moves to the spill tier (cand_n >= 64)
GS_FN void bg_partition(GsState &s)
{
    const int lane = gs_lane();
    const uint64_t lt = (1ull << lane) - 1ull;
    const long long mine = s.cand[(int)(((long long)lane * s.cand_n) >> 6)];
    s.samp[lane] = mine;
    gs_barrier();
    int rank = 0;
    for (int j = 0; j < 64; ++j) rank += (s.samp[j] < mine) ? 1 : 0;
    const long long pivot = gs_shfl(mine, gs_first(gs_ballot(rank == 31)));
    int new_n = 0, moved = 0;
    for (int base = 0; base < s.cand_n; base += 64) {
        const int i = base + lane;
        const bool in = i < s.cand_n;
        const long long k = in ? s.cand[i] : 0;
        const bool hi = in && k > pivot;
        const bool lo = in && !hi;
        const uint64_t mh = gs_ballot(hi), ml = gs_ballot(lo);  // every lane has read its key before any lane writes
        if (hi) s.cand[new_n + gs_popc(mh & lt)] = k;          // in place: target index <= i
        if (lo) {
            const int pos = s.spill_n + moved + gs_popc(ml & lt);
            if (pos < s.spill_cap) s.spill[pos] = k;
        }
        new_n += gs_popc(mh);
        moved += gs_popc(ml);
        gs_barrier();
    }
    if (s.spill_n + moved > s.spill_cap) s.status = GS_OVERFLOW;
    s.spill_n += moved;
    s.cand_n = new_n;
    s.spill_max = pivot;  // the pivot itself moved, everything that stayed is larger
}

// gs_refill over a capacity: the LDS tier ran dry while keys wait in the spill tier — bring the best of them back
GS_FN void bg_refill(GsState &s, int cand_cap)
{
    const int lane = gs_lane();
    const uint64_t lt = (1ull << lane) - 1ull;
    gs_fence();
    const int n = s.spill_n;
    if (n <= cand_cap / 2) {
        for (int base = 0; base < n; base += 64)
            if (base + lane < n) s.cand[base + lane] = s.spill[base + lane];
        s.cand_n = n;
        s.spill_n = 0;
        s.spill_max = GS_KEY_MIN;
        gs_barrier();
        return;
    }
    const long long mine = s.spill[(int)(((long long)lane * n) >> 6)];
    s.samp[lane] = mine;
    gs_barrier();
    int rank = 0;
    for (int j = 0; j < 64; ++j) rank += (s.samp[j] < mine) ? 1 : 0;   // keys are unique: the ranks are 0..63, each once
    int r = 63 - (int)(((long long)(cand_cap / 4) * 64) / n);           // ~cand_cap / 4 keys expected above the rank-r sample
    r = r < 1 ? 1 : (r > 62 ? 62 : r);
    long long pivot = 0;
    int above = 0;
    for (int attempt = 0; attempt < 8; ++attempt) {
        pivot = gs_shfl(mine, gs_first(gs_ballot(rank == r)));
        above = 0;
        for (int base = 0; base < n; base += 64) above += gs_popc(gs_ballot(base + lane < n && s.spill[base + lane] > pivot));
        if (above <= cand_cap - 64 || r >= 62) break;   // (r <= 62: at least the largest sample lies above the pivot)
        r += (64 - r) / 2;                                // too many for the tier: a higher pivot
        if (r > 62) r = 62;
    }
    gs_barrier();
    if (above == 0 || above > cand_cap - 64) return;
    int nc = 0, ns = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n;
        const long long k = in ? s.spill[i] : 0;
        const bool hi = in && k > pivot;
        const bool lo = in && !hi;
        const uint64_t mh = gs_ballot(hi), ml = gs_ballot(lo);  // every lane has read its key before any lane writes
        if (hi) s.cand[nc + gs_popc(mh & lt)] = k;
        if (lo) s.spill[ns + gs_popc(ml & lt)] = k;             // in place: target index <= i
        nc += gs_popc(mh);
        ns += gs_popc(ml);
        gs_barrier();
    }
    s.cand_n = nc;
    s.spill_n = ns;
    s.spill_max = pivot;   // the pivot itself stayed behind; everything that moved is larger
    gs_fence();
}

// gs_push over a capacity: candidates.push for up to one key per lane
GS_FN void bg_push(GsState &s, int cand_cap, long long key, bool has)
{
    const int lane = gs_lane();
    const uint64_t lt = (1ull << lane) - 1ull;
    bool to_lds;
    uint64_t ml;
    for (;;) {
        to_lds = has && (s.spill_n == 0 || key > s.spill_max);
        ml = gs_ballot(to_lds);
        if (s.cand_n + gs_popc(ml) <= cand_cap) break;
        bg_partition(s);
        if (s.status != GS_OK) return;
    }
    if (to_lds) s.cand[s.cand_n + gs_popc(ml & lt)] = key;
    s.cand_n += gs_popc(ml);
    const bool to_sp = has && !to_lds;
    const uint64_t ms = gs_ballot(to_sp);
    if (ms) {
        if (s.spill_n + gs_popc(ms) > s.spill_cap) {
            s.status = GS_OVERFLOW;
            return;
        }
        if (to_sp) s.spill[s.spill_n + gs_popc(ms & lt)] = key;
        s.spill_n += gs_popc(ms);
    }
    gs_barrier();
}

// One query.  WT > 0: rows of exactly WT words, the query's words in (scalar) registers; WT == 0: any width, the words in LDS.
template <int WT, bool SAFE>
GS_FN void bg_search_one(const BgParams &p, int q, int worker, char *lds)
{
    const int lane = gs_lane();
    const int W = WT > 0 ? WT : p.W;
    const int D = p.D;
    const int cand_cap = p.cand_cap;
    GsState s;
    s.res = reinterpret_cast<long long *>(lds);
    s.cand = s.res + p.rerankK;
    s.samp = s.cand + cand_cap;
    s.evicted = nullptr;   // (the evicted list is the tail of the spill slice)
    uint64_t *qw_lds = reinterpret_cast<uint64_t *>(s.samp + 64);
    uint32_t *vis_lds = reinterpret_cast<uint32_t *>(qw_lds + (WT > 0 ? 0 : p.W));
    const int spill_total = p.spill_cap;
    s.spill = p.spill + (int64_t)worker * spill_total;
    s.spill_cap = spill_total;
    s.cand_n = s.spill_n = s.res_n = s.ev_n = 0;
    s.res_min_idx = -1;
    s.spill_max = GS_KEY_MIN;
    s.res_min = GS_KEY_MAX;
    s.status = GS_OK;
    const bool vis_in_lds = !SAFE && p.vcap_log2 <= BG_VIS_LDS_MAX_LOG2;
    const int vcap = SAFE ? 0 : (1 << p.vcap_log2);
    const uint32_t vmask = (uint32_t)vcap - 1u;
    const int vshift = 32 - p.vcap_log2;
    int32_t *vis_g = (SAFE || vis_in_lds) ? nullptr : p.visited + (int64_t)worker * vcap;
    uint32_t *bm = SAFE ? p.bitmap + (int64_t)worker * p.bitmap_words : nullptr;
    int n_tab = 0;   // nodes in the FAST form's table (wave-uniform)
    long long n_visited = 0, n_expanded = 0;

    // ---- per-query setup: clear the visited set, fetch the query's words ----
    if (SAFE) {
        gs_u4 *b4 = reinterpret_cast<gs_u4 *>(bm);
        const gs_u4 zero = {0u, 0u, 0u, 0u};
        for (long long i = lane; i < p.bitmap_words / 4; i += 64) b4[i] = zero;
    } else if (vis_in_lds) {
        for (int i = lane; i < vcap; i += 64) vis_lds[i] = 0xFFFFFFFFu;
    } else {
        gs_u4 *v4 = reinterpret_cast<gs_u4 *>(vis_g);
        const gs_u4 ones = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        for (int i = lane; i < vcap / 4; i += 64) v4[i] = ones;
    }
    uint64_t qw[WT > 0 ? WT : 1];
    if constexpr (WT > 0) {
        const uint64_t *src = p.qwords + (int64_t)q * WT;   // q is wave-uniform: scalar loads
#pragma unroll
        for (int i = 0; i < WT; ++i) qw[i] = src[i];
    } else {
        qw[0] = 0;
        const uint64_t *src = p.qwords + (int64_t)q * W;
        for (int i = lane; i < W; i += 64) qw_lds[i] = src[i];
    }
    gs_fence();
    gs_barrier();

    // hammingDistance(query words, row nb): DefaultVectorUtilSupport.hammingDistance, every word's loads issued before the counts
    auto hamming = [&](int32_t nb) -> int32_t {
        int32_t h = 0;
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
    };
    // visited.add for one node per participating lane (divergent: no wave operation inside)
    auto visit = [&](int32_t nb) -> bool {
        if (SAFE) return bg_visit_bits(bm, nb);
        if (vis_in_lds) return bg_visit_lds(vis_lds, vmask, vshift, nb);
        return gs_visit(vis_g, vmask, vshift, nb);
    };

    // ---- initializeInternal :334-353: mark and score the entry node ----
    {
        const int32_t e = p.entry_node;
        if (lane == 0) (void)visit(e);
        n_tab = 1;
        const int32_t h = hamming(e);
        if (lane == 0) s.cand[0] = bg_key(e, D - h);
        s.cand_n = 1;
        gs_fence();
        gs_barrier();
    }
    const unsigned long long *acc = p.accept ? p.accept + (long long)q * p.accept_stride : nullptr;
    const int32_t excluded = p.exclude ? p.exclude[q] : -1;   // (a node id is never negative)

    for (int lvl = p.entry_level; lvl >= 0 && s.status == GS_OK; --lvl) {
        const int rk = lvl > 0 ? 1 : p.rerankK;
        const GsLevel &L = p.lv[lvl];
        // ---- searchOneLayer :406-457 ----
        for (;;) {
            if (s.cand_n == 0 && s.spill_n == 0) break;
            if (s.cand_n == 0) bg_refill(s, cand_cap);
            int idx;
            long long top;
            const bool from_lds = s.cand_n > 0;
            if (from_lds) {
                top = gs_scan_extreme<true>(s.cand, s.cand_n, &idx);
            } else {   // no pivot separated anything: the best candidate is somewhere in the spill tier
                gs_fence();
                top = gs_scan_extreme<true>(s.spill, s.spill_n, &idx);
            }
            const int32_t top_hi = bg_key_hi(top);
            if (s.res_n >= rk && top_hi < bg_key_hi(s.res_min)) break;   // stopSearch :355-369 (strict <)
            // candidates.pop()
            if (from_lds) {
                if (lane == 0) s.cand[idx] = s.cand[s.cand_n - 1];
                s.cand_n--;
            } else {
                if (lane == 0) s.spill[idx] = s.spill[s.spill_n - 1];
                s.spill_n--;
                s.spill_max = top;   // still an upper bound of what is left
                gs_fence();
            }
            gs_barrier();
            const int32_t node = gs_key_node(top);
            // the popped node's adjacency row is requested before the result list is touched
            const int32_t *row = lvl == 0 ? (L.nbrs + (int64_t)node * L.degree) : gs_level_row(L, node);
            int32_t nb0 = -1;
            if (row && lane < L.degree) nb0 = row[lane];
            // addTopCandidate :515-530 (a BQ similarity is never negative or NaN: `score >= threshold` always holds at threshold 0)
            const bool accepted = !(lvl == 0 && (node == excluded || (acc && !((acc[node >> 6] >> (node & 63)) & 1ull))));
            if (!accepted) {
            } else if (s.res_n < rk) {
                if (lane == 0) s.res[s.res_n] = top;
                if (top < s.res_min) {
                    s.res_min = top;
                    s.res_min_idx = s.res_n;
                }
                s.res_n++;
                gs_barrier();
            } else if (top_hi > bg_key_hi(s.res_min)) {
                if (lvl > 0) {   // evictedResults: kept for the next layer's entry points
                    if (s.spill_n >= spill_total - s.ev_n) {
                        s.status = GS_OVERFLOW;
                        break;
                    }
                    if (lane == 0) s.spill[spill_total - 1 - s.ev_n] = s.res_min;
                    s.ev_n++;
                    s.spill_cap = spill_total - s.ev_n;
                }
                if (lane == 0) s.res[s.res_min_idx] = top;
                gs_barrier();
                s.res_min = gs_scan_extreme<false>(s.res, s.res_n, &s.res_min_idx);
            }
            n_expanded++;
            if (!row) continue;
            // ---- the row, 64 neighbours at a time; rows are packed: the first -1 ends them ----
            for (int base = 0; base < L.degree; base += 64) {
                const int i = base + lane;
                const int32_t nb = base == 0 ? nb0 : (i < L.degree ? row[i] : -1);
                const uint64_t bad = gs_ballot(i < L.degree && nb < 0);
                const bool valid = i < L.degree && nb >= 0 && nb < p.n_nodes && lane < gs_first(bad);
                if (!SAFE && (n_tab + 64) * 2 > vcap) {   // the table stays at most half full
                    s.status = GS_OVERFLOW;
                    break;
                }
                const bool fresh = valid && visit(nb);
                const uint64_t fm = gs_ballot(fresh);
                n_tab += gs_popc(fm);
                n_visited += gs_popc(fm);
                if (fm) {
                    int32_t c = 0;
                    if (fresh) c = D - hamming(nb);
                    // level 0: below the worst of a full result list = never popped (the minimum only grows)
                    const bool keep = fresh && !(lvl == 0 && s.res_n >= rk && c < bg_key_hi(s.res_min));
                    bg_push(s, cand_cap, bg_key(nb, c), keep);
                    if (s.status != GS_OK) break;
                }
                if (bad) break;
            }
            if (s.status != GS_OK) break;
        }
        if (s.status != GS_OK) break;
        if (lvl > 0) {   // setEntryPointsFromPreviousLayer :324-331: results and evicted results go back to the candidates
            for (int base = 0; base < s.res_n; base += 64) {
                const bool has = base + lane < s.res_n;
                const long long k = has ? s.res[base + lane] : 0;
                bg_push(s, cand_cap, k, has);
                if (s.status != GS_OK) break;
            }
            gs_fence();
            while (s.ev_n > 0 && s.status == GS_OK) {   // from the most recent one: the reserved tail shrinks as it is consumed
                const int cnt = s.ev_n < 64 ? s.ev_n : 64;
                const bool has = lane < cnt;
                const long long k = has ? s.spill[spill_total - s.ev_n + lane] : 0;
                gs_barrier();
                s.ev_n -= cnt;
                s.spill_cap = spill_total - s.ev_n;
                bg_push(s, cand_cap, k, has);
            }
            s.res_n = 0;
            s.res_min = GS_KEY_MAX;
            s.res_min_idx = -1;
            gs_barrier();
        }
    }

    // ---- hand the kept approximate results to the rerank stage: ids + BQVectors.similarityBetween in f32 ----
    gs_barrier();
    for (int i = lane; i < p.rerankK; i += 64) {
        const bool have = s.status == GS_OK && i < s.res_n;
        const long long k = have ? s.res[i] : 0;
        p.out_ids[(int64_t)q * p.rerankK + i] = have ? gs_key_node(k) : -1;
        p.out_scores[(int64_t)q * p.rerankK + i] = have ? 1.0f - (float)(D - bg_key_hi(k)) / (float)D : -__builtin_inff();
    }
    if (lane == 0) {
        p.out_stats[2 * (int64_t)q] = n_visited;
        p.out_stats[2 * (int64_t)q + 1] = n_expanded;
        p.out_status[q] = s.status;
    }
    gs_barrier();
}

// Persistent worker: pulls queries off the shared counter until none are left.
template <int WT, bool SAFE>
GS_FN void bg_worker(const BgParams &p, int worker, char *lds)
{
    for (;;) {
        long long qv = 0;
        if (gs_lane() == 0) qv = (long long)gs_fetch_add(p.next_query, 1u);
        const int item = (int)gs_shfl(qv, 0);
        if (item >= p.Q) break;
        bg_search_one<WT, SAFE>(p, p.qmap ? p.qmap[item] : item, worker, lds);
    }
}

}  // namespace jv
