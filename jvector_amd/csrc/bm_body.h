// bm_body.h — the entry point of a graph built from binary-quantized rows alone (bq_builder.cpp): the bitwise-majority row of the top
// level's members and the member nearest to it.  The PQ layered build enters at the top level's node most similar to the mean of the
// top level's vectors; with BQ rows only, the mean's analogue is the row whose bit b is set iff strictly more than half of the
// members have it set, and "most similar" is the minimum Hamming distance (the BQ similarity 1 - (float) h / D is strictly decreasing
// in h for D <= 16383).  The bodies of bq_majority_kernel / bq_nearest_row_kernel / bq_nearest_final_kernel (k_bq_builder.hip), written
// against the wave API of gs_body.h so that the same source compiles for the lane emulator of the CPU tests (tests/emu/bm_emu.cpp).
//
// Majority: one 64-lane wavefront per 64-bit word w.  The lanes stride over the members (lane l reads word w of members l, l + 64,
// ...); for each group of 64 members and each bit b one ballot gathers bit b of the 64 words and its popcount goes to lane b's
// counter.  Lane b ends up with the number of members that have bit 64 w + b set; the centroid word is one more ballot.  Integer
// counters only; padding bits beyond D are zero in every row, so their counts are zero and they stay zero.
// Nearest row: a lane per member, key = (hamming << 32) | id — an integer, so the minimum is exact and a tie goes to the smaller id;
// reduced across the wave (gs_wave_min), one key per wave written out, and one wave of a second launch reduces those.  No atomics.
#pragma once

#include <cstdint>

#include "gs_body.h"

namespace jv {

struct BmParams {
    const uint64_t *rows;      // [n_rows][W] BQ rows
    int64_t n_rows;
    int32_t W;
    const int32_t *members;    // [n] ordinals of the members, ascending, each inside [0, n_rows); nullptr: members 0..n-1
    int32_t n;                 // members, >= 1
    uint64_t *centroid;        // [W] the majority row (written by bm_majority_word, read by bm_nearest_partial)
    long long *partial;        // [waves] one key per wave of bm_nearest_partial
    int32_t waves;
    long long *best;           // [1] the smallest key: (hamming << 32) | id
};

GS_FN int64_t bm_member(const BmParams &p, int i) { return p.members ? (int64_t)p.members[i] : (int64_t)i; }

// word w of the majority row; every lane of the wave takes part
GS_FN void bm_majority_word(const BmParams &p, int w)
{
    const int lane = gs_lane();
    uint32_t count = 0;   // members with bit 64 w + lane set
    for (int base = 0; base < p.n; base += 64) {
        const int i = base + lane;
        uint64_t x = 0;   // a lane past the last member adds nothing to any count
        if (i < p.n) {
            const int64_t id = bm_member(p, i);
            if (id >= 0 && id < p.n_rows) x = p.rows[id * p.W + w];   // (the host names members inside the rows; nothing outside is ever read)
        }
        for (int b = 0; b < 64; ++b) {
            const int c = gs_popc(gs_ballot(((x >> b) & 1ull) != 0));
            if (lane == b) count += (uint32_t)c;
        }
    }
    const uint64_t word = gs_ballot(2ull * (uint64_t)count > (uint64_t)(uint32_t)p.n);   // strictly more than n / 2
    if (lane == 0) p.centroid[w] = word;
}

// wave `wave` of p.waves: the smallest key among members wave * 64 + lane, + 64 p.waves, ...
GS_FN void bm_nearest_partial(const BmParams &p, int wave)
{
    const int lane = gs_lane();
    long long best = GS_KEY_MAX;
    for (int64_t i = (int64_t)wave * 64 + lane; i < p.n; i += (int64_t)p.waves * 64) {
        const int64_t id = bm_member(p, (int)i);
        if (id < 0 || id >= p.n_rows) continue;
        const uint64_t *row = p.rows + id * p.W;
        uint32_t h = 0;
        for (int w = 0; w < p.W; ++w) h += (uint32_t)gs_popc(row[w] ^ p.centroid[w]);
        const long long key = (long long)(((unsigned long long)h << 32) | (unsigned long long)(uint32_t)id);
        best = key < best ? key : best;
    }
    best = gs_wave_min(best);
    if (lane == 0) p.partial[wave] = best;
}

// one wave: the smallest of the p.waves keys
GS_FN void bm_nearest_final(const BmParams &p)
{
    const int lane = gs_lane();
    long long best = GS_KEY_MAX;
    for (int i = lane; i < p.waves; i += 64) best = p.partial[i] < best ? p.partial[i] : best;
    best = gs_wave_min(best);
    if (lane == 0) p.best[0] = best;
}

}  // namespace jv
