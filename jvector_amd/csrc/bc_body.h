// bc_body.h — compacting a graph under construction over binary-quantized rows (bq_builder.cpp): the sequential renumbering of
// AbstractGraphIndexWriter.sequentialRenumbering (B/graph/disk/AbstractGraphIndexWriter.java:146-159) — the nodes in the graph get the
// ordinals 0, 1, 2 ... in their old relative order — and the rows carried across it, as OrdinalMapper.MapMapper and
// RemappedRandomAccessVectorValues do on the host.  The bodies of the kernels of k_bq_compact.hip, written against the wave API of
// gs_body.h so that the same source compiles for the lane emulator of the CPU tests (tests/emu/bc_emu.cpp).
//
// Rank.  An exclusive scan over the present words in three steps, no atomics:
//   bc_rank_sums   one wavefront per scan block of BC_SCAN_NODES nodes: four words per lane, popcounts summed over the wave
//   bc_rank_scan   one wavefront: the block sums become the nodes before each block; the total is the number of live nodes
//   bc_rank_write  one wavefront per 64 words: the popcounts of the words of its scan block that lie before its own (at most 192, read
//                  again: they are in L2) and a prefix over its own 64 give every word its base; then word after word ONE LANE TAKES
//                  ONE BIT: old_to_new[64 w + j] = base(w) + popcount(word & ((1 << j) - 1)) for a set bit, else -1 — a coalesced
//                  256-byte store — and new_to_old[rank] = 64 w + j for the set bits, consecutive ranks from consecutive lanes.
// Bits at and beyond n in the last word count as clear.
//
// Rows.  bc_rows: the live x R cells of the new adjacency, 64 consecutive cells per step of a wavefront, so every store is one
// coalesced line whatever R is; a lane finds its row and slot from the wave's first cell (one 64-bit division per wave, wave-uniform,
// and a small 32-bit one per lane and step).  Cell (r, e) takes entry e of old row new_to_old[r]: the id goes through old_to_new (-1 stays
// -1), the score bits are copied, slot 0 also copies diverseBefore.  A stored id without an image is written as -1 and COUNTED: one
// atomic add per wavefront into a counter that only ever decides failure, never a position, and the smallest new row holding one is
// kept for the message.  bc_bq_rows: the live x W words of the BQ rows the same way, lanes across words.
// Nothing depends on the order in which waves or lanes run.
#pragma once

#include <cstdint>

#include "bc_params.h"
#include "gs_body.h"

namespace jv {

// word w of the present bitmap as the rank sees it: nothing at and beyond n, nothing past the last word
GS_FN uint64_t bc_present_word(const BcParams &p, int64_t w)
{
    if (w * 64 >= p.n) return 0ull;
    uint64_t m = p.present[w];
    const int64_t left = p.n - w * 64;
    if (left < 64) m &= (1ull << left) - 1ull;
    return m;
}

// scan block b: its number of live nodes into block_base[b]
GS_FN void bc_rank_sums(const BcParams &p, int64_t b)
{
    const int lane = gs_lane();
    uint32_t c = 0;
    for (int i = 0; i < BC_SCAN_WORDS / 64; ++i) c += (uint32_t)gs_popc(bc_present_word(p, b * BC_SCAN_WORDS + i * 64 + lane));
    uint32_t total = 0;
    for (int s = 0; s < 64; ++s) total += gs_bcast32(c, s);
    if (lane == 0) p.block_base[b] = total;
}

// one wave: block_base becomes its own exclusive prefix; the counters are set
GS_FN void bc_rank_scan(const BcParams &p)
{
    const int lane = gs_lane();
    const int64_t blocks = bc_scan_blocks(p.n);
    uint32_t running = 0;
    for (int64_t base = 0; base < blocks; base += 64) {
        const int64_t b = base + lane;
        const uint32_t c = b < blocks ? p.block_base[b] : 0u;
        uint32_t before = 0, total = 0;
        for (int s = 0; s < 64; ++s) {
            const uint32_t cs = gs_bcast32(c, s);
            before += s < lane ? cs : 0u;
            total += cs;
        }
        if (b < blocks) p.block_base[b] = running + before;
        running += total;
    }
    if (lane == 0) {
        p.counters[0] = running;
        p.counters[1] = 0u;
        p.counters[2] = 0x7fffffffu;
    }
}

// words [64 seg, 64 seg + 64): the two maps of their nodes
GS_FN void bc_rank_write(const BcParams &p, int64_t seg)
{
    const int lane = gs_lane();
    const int64_t b = seg / (BC_SCAN_WORDS / 64);
    const int q = (int)(seg - b * (BC_SCAN_WORDS / 64));   // wave-uniform: 64-word pieces of the scan block before this one
    uint32_t c = 0;
    for (int i = 0; i < q; ++i) c += (uint32_t)gs_popc(bc_present_word(p, b * BC_SCAN_WORDS + i * 64 + lane));
    const uint64_t m = bc_present_word(p, seg * 64 + lane);
    const uint32_t mc = (uint32_t)gs_popc(m);
    uint32_t before = 0, prior = 0;
    for (int s = 0; s < 64; ++s) {
        const uint32_t cs = gs_bcast32(mc, s);
        before += s < lane ? cs : 0u;
        prior += gs_bcast32(c, s);
    }
    const uint32_t base = p.block_base[b] + prior + before;   // the rank of the first set bit of this lane's word
    const uint64_t below = (1ull << lane) - 1ull;
    for (int s = 0; s < 64; ++s) {
        const int64_t node = (seg * 64 + s) * 64 + lane;
        if (node - lane >= p.n) break;   // wave-uniform: past the last word
        const uint64_t word = (uint64_t)gs_shfl((long long)m, s);
        const uint32_t wb = gs_bcast32(base, s);
        const bool set = ((word >> lane) & 1ull) != 0;
        const int32_t rank = (int32_t)(wb + (uint32_t)gs_popc(word & below));
        if (node < p.n) p.old_to_new[node] = set ? rank : -1;
        if (set && p.new_to_old) p.new_to_old[rank] = (int32_t)node;   // (a set bit lies below n)
    }
}

// The two gathers below walk BC_WAVE_CELLS consecutive cells of a [rows][width] array, 64 per step.  The steps are unrolled and run
// STAGE BY STAGE — every step's row index, then every step's row data, then every step's images, then the stores — so that a wave has
// all its steps' loads in flight at once: each stage is a dependent load, and taken step by step a wave would wait out three memory
// latencies for every 768 bytes it moves.
constexpr int BC_STEPS = BC_WAVE_CELLS / 64;

// the wave's first cell c_first (wave-uniform): its row and the offset inside it; one 64-bit division per wave
struct BcWalk {
    int64_t r0;
    uint32_t rem;
};
GS_FN BcWalk bc_walk(int64_t c_first, int32_t width)
{
    BcWalk w;
    w.r0 = c_first / width;
    w.rem = (uint32_t)(c_first - w.r0 * width);
    return w;
}
// the lane's cell of step `it`: its row (relative to w.r0) and its slot; the operands stay below width + BC_WAVE_CELLS + 64
GS_FN void bc_cell(const BcWalk &w, int32_t width, int it, int lane, uint32_t &dr, int32_t &slot)
{
    const uint32_t off = w.rem + (uint32_t)(it * 64 + lane);
    dr = off / (uint32_t)width;
    slot = (int32_t)(off - dr * (uint32_t)width);
}

// cells [BC_WAVE_CELLS wave, BC_WAVE_CELLS (wave + 1)) of the new adjacency
GS_FN void bc_rows(const BcParams &p, int64_t wave)
{
    const int lane = gs_lane();
    const int64_t cells = p.live * p.R, c_first = wave * BC_WAVE_CELLS;
    const BcWalk w = bc_walk(c_first, p.R);
    bool on[BC_STEPS];
    uint32_t dr[BC_STEPS];
    int32_t e[BC_STEPS], src[BC_STEPS], id[BC_STEPS], db[BC_STEPS];
    float sc[BC_STEPS];
#pragma unroll
    for (int it = 0; it < BC_STEPS; ++it) {
        bc_cell(w, p.R, it, lane, dr[it], e[it]);
        on[it] = c_first + it * 64 + lane < cells;
        src[it] = on[it] ? p.new_to_old[w.r0 + dr[it]] : 0;   // (the rank wrote it: inside [0, n))
    }
#pragma unroll
    for (int it = 0; it < BC_STEPS; ++it) {
        const int64_t from = (int64_t)src[it] * p.R + e[it];
        id[it] = on[it] ? p.src_nbrs[from] : -1;
        sc[it] = on[it] ? p.src_nsc[from] : 0.0f;
        db[it] = on[it] && e[it] == 0 ? p.src_db[src[it]] : 0;
    }
    bool bad[BC_STEPS];
#pragma unroll
    for (int it = 0; it < BC_STEPS; ++it) {
        bad[it] = false;
        if (id[it] >= 0) {
            id[it] = id[it] < p.n ? p.old_to_new[id[it]] : -1;
            bad[it] = id[it] < 0;
        }
    }
    uint32_t unmapped = 0;
    int32_t first_row = 0x7fffffff;
#pragma unroll
    for (int it = 0; it < BC_STEPS; ++it) {
        const int64_t c = c_first + it * 64 + lane;
        if (on[it]) {
            p.dst_nbrs[c] = id[it];
            p.dst_nsc[c] = sc[it];
            if (e[it] == 0) p.dst_db[w.r0 + dr[it]] = db[it];
        }
        const uint64_t mb = gs_ballot(bad[it]);
        if (mb != 0) {   // wave-uniform
            const int32_t at = (int32_t)(w.r0 + (int64_t)gs_bcast32(dr[it], __builtin_ctzll(mb)));   // rows ascend with the lanes and the steps
            first_row = first_row < at ? first_row : at;
            unmapped += (uint32_t)gs_popc(mb);
        }
    }
    if (unmapped != 0 && lane == 0) {
        gs_fetch_add(p.counters + 1, unmapped);
        int32_t *slot = reinterpret_cast<int32_t *>(p.counters + 2);   // min: the value only grows smaller, whoever comes first
        int32_t expect = 0x7fffffff;
        for (int tries = 0; tries < 64 && expect > first_row; ++tries) {
            const int32_t old = gs_cas(slot, expect, first_row);
            if (old == expect) break;
            expect = old;
        }
    }
}

// words [BC_WAVE_CELLS wave, BC_WAVE_CELLS (wave + 1)) of the new BQ rows
GS_FN void bc_bq_rows(const BcParams &p, int64_t wave)
{
    const int lane = gs_lane();
    const int64_t cells = p.live * p.W, c_first = wave * BC_WAVE_CELLS;
    const BcWalk w = bc_walk(c_first, p.W);
    bool on[BC_STEPS];
    int32_t k[BC_STEPS], src[BC_STEPS];
    uint64_t v[BC_STEPS];
#pragma unroll
    for (int it = 0; it < BC_STEPS; ++it) {
        uint32_t dr;
        bc_cell(w, p.W, it, lane, dr, k[it]);
        on[it] = c_first + it * 64 + lane < cells;
        src[it] = on[it] ? p.new_to_old[w.r0 + dr] : 0;
    }
#pragma unroll
    for (int it = 0; it < BC_STEPS; ++it) v[it] = on[it] ? p.src_rows[(int64_t)src[it] * p.W + k[it]] : 0ull;
#pragma unroll
    for (int it = 0; it < BC_STEPS; ++it)
        if (on[it]) p.dst_rows[c_first + it * 64 + lane] = v[it];
}

}  // namespace jv

