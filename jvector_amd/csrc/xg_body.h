// xg_body.h — device-resident graph traversal with EXACT scores: one 64-lane wavefront runs one query's whole GraphSearcher loop
// with VectorSimilarityFunction.compare on the float rows as the score function.  The body of exact_graph_search_kernel
// (k_exact_gsearch.hip).
//
// What it computes is GraphSearcher.search(DefaultSearchScoreProvider(exact score function), topK, rerankK = beamK, 0, 0, acceptOrds)
// up to the final ordering (B/graph/GraphSearcher.java:263-282 internalSearch, 334-353 initializeInternal, 355-369 stopSearch,
// 406-457 searchOneLayer, 324-331 setEntryPointsFromPreviousLayer, 515-530 addTopCandidate — the walk bg_body.h restates): the beamK
// kept results with their scores, visitedCount and expandedCount.
//
// Keys.  The queues hold NodeQueue's own keys, gs_key = sortableInt(score) << 32 | ~node as a SIGNED 64-bit integer: a negative score
// has a negative sortable int and a negative key, and signed comparison orders them as NodeQueue.encode does (-0.0 below +0.0).  The
// walk's own tests — stopSearch's `<`, addTopCandidate's `>` — are the reference's FLOAT comparisons on the decoded scores (-0.0 equals
// +0.0 there), never comparisons of key halves.
//
// Traversal state.  bg_body.h's pieces as they are (none of them looks at a BQ parameter): bg_partition / bg_refill / bg_push over the
// LDS candidate tier and the global spill tier, the result list with its cached minimum, the evicted list at the end of the spill
// slice, bg_visit_lds / gs_visit (FAST) and bg_visit_bits (SAFE).  A query that outgrows the FAST form leaves with GS_OVERFLOW and no
// results; the host runs it again in the SAFE form.  Both forms make the same comparisons.
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
#include "bg_body.h"
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

// One query.
template <int VSF, bool TR, bool SAFE>
GS_FN void xg_search_one(const XgParams &p, int q, int worker, char *lds)
{
    const int lane = gs_lane();
    const uint64_t lt = (1ull << lane) - 1ull;
    const int cand_cap = p.cand_cap;
    // LDS: [score tile][64 fresh ids][results][candidate tier][64 samples][visited table] (the tile first: its b128 accesses want 16 bytes)
    float *tile = reinterpret_cast<float *>(lds);
    int32_t *fr = reinterpret_cast<int32_t *>(tile + XG_TILE_FLOATS);
    GsState s;
    s.res = reinterpret_cast<long long *>(fr + XG_GROUP);
    s.cand = s.res + p.beamK;
    s.samp = s.cand + cand_cap;
    s.evicted = nullptr;   // (the evicted list is the tail of the spill slice)
    uint32_t *vis_lds = reinterpret_cast<uint32_t *>(s.samp + 64);
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

    // ---- per-query setup: clear the visited set ----
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
    gs_fence();
    gs_barrier();

    // visited.add for one node per participating lane (divergent: no wave operation inside)
    auto visit = [&](int32_t nb) -> bool {
        if (SAFE) return bg_visit_bits(bm, nb);
        if (vis_in_lds) return bg_visit_lds(vis_lds, vmask, vshift, nb);
        return gs_visit(vis_g, vmask, vshift, nb);
    };

    // ---- initializeInternal :334-353: mark and score the entry node (a group of one row) ----
    {
        const int32_t e = p.entry_node;
        if (lane == 0) (void)visit(e);
        n_tab = 1;
        const float sc = xg_score_group<VSF, TR>(p, q, lane == 0 ? e : -1, 1, tile);
        if (lane == 0) s.cand[0] = gs_key(e, sc);
        s.cand_n = 1;
        gs_fence();
        gs_barrier();
    }
    const unsigned long long *acc = p.accept ? p.accept + (long long)q * p.accept_stride : nullptr;
    const int32_t excl = p.exclude ? p.exclude[q] : -1;   // (a popped node is never negative)

    for (int lvl = p.entry_level; lvl >= 0 && s.status == GS_OK; --lvl) {
        const int rk = lvl > 0 ? 1 : p.beamK;
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
            const float top_sc = gs_key_score(top);
            if (s.res_n >= rk && top_sc < gs_key_score(s.res_min)) break;   // stopSearch :355-369 (strict <, on the floats)
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
            // addTopCandidate :515-530 (`score >= threshold` at threshold 0: as the reference, a negative or NaN score is expanded, not kept)
            const bool accepted = top_sc >= 0.0f && !(lvl == 0 && (node == excl || (acc && !((acc[node >> 6] >> (node & 63)) & 1ull))));
            if (!accepted) {
            } else if (s.res_n < rk) {
                if (lane == 0) s.res[s.res_n] = top;
                if (top < s.res_min) {
                    s.res_min = top;
                    s.res_min_idx = s.res_n;
                }
                s.res_n++;
                gs_barrier();
            } else if (top_sc > gs_key_score(s.res_min)) {
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
            // ---- the row, 64 slots at a time; rows are packed: the first -1 ends them ----
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
                const int cnt = gs_popc(fm);
                n_tab += cnt;
                n_visited += cnt;
                if (fm) {
                    // compaction: lane j takes the j-th fresh neighbour, then the group is scored one lane per row
                    if (fresh) fr[gs_popc(fm & lt)] = nb;
                    gs_barrier();
                    const int32_t mine = lane < cnt ? fr[lane] : -1;
                    gs_barrier();
                    const float sc = xg_score_group<VSF, TR>(p, q, mine, cnt, tile);
                    // level 0: below the worst of a full result list = never popped (the minimum only grows)
                    const bool keep = mine >= 0 && !(lvl == 0 && s.res_n >= rk && sc < gs_key_score(s.res_min));
                    bg_push(s, cand_cap, gs_key(mine, sc), keep);
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

    // ---- the kept results leave unordered; the host's top-k puts the first topK in NodeQueue order ----
    gs_barrier();
    for (int i = lane; i < p.beamK; i += 64) {
        const bool have = s.status == GS_OK && i < s.res_n;
        const long long k = have ? s.res[i] : 0;
        p.out_ids[(int64_t)q * p.beamK + i] = have ? gs_key_node(k) : -1;
        p.out_scores[(int64_t)q * p.beamK + i] = have ? gs_key_score(k) : -__builtin_inff();
    }
    if (lane == 0) {
        p.out_stats[2 * (int64_t)q] = n_visited;
        p.out_stats[2 * (int64_t)q + 1] = n_expanded;
        p.out_status[q] = s.status;
    }
    gs_barrier();
}

// Persistent worker: pulls queries off the shared counter until none are left.
template <int VSF, bool TR, bool SAFE>
GS_FN void xg_worker(const XgParams &p, int worker, char *lds)
{
    for (;;) {
        long long qv = 0;
        if (gs_lane() == 0) qv = (long long)gs_fetch_add(p.next_query, 1u);
        const int item = (int)gs_shfl(qv, 0);
        if (item >= p.Q) break;
        xg_search_one<VSF, TR, SAFE>(p, p.qmap ? p.qmap[item] : item, worker, lds);
    }
}

}  // namespace jv
