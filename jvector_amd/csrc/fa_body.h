// fa_body.h — the flat PQ search under an accept filter (flat_accept.cpp): the accept masks compacted to ascending ordinal lists, and
// the multi-query ADC scan that walks such a list.  The bodies of the kernels of k_flat_accept.hip, written against the wave API of
// gs_body.h so that the same source compiles for the lane emulator of the CPU tests (tests/emu/fa_emu.cpp).  No atomics anywhere:
// the lists are ascending and every result is reproducible.
//
// Mask -> lists.  An exclusive scan over the accept words in three steps, batched over masks (the rank scan of bc_body.h):
//   fa_sums    one wavefront per (mask, scan block of FA_SCAN_ROWS rows): four words per lane, popcounts summed over the wave
//   fa_scan    one wavefront per mask: the block sums become the accepted rows before each block; the total is the list's length
//   fa_write   one wavefront per (list row, 64 words): the popcounts of the words of its scan block that lie before its own (read
//              again: they are in L2) and a prefix over its own 64 give every word its base; then, for each word that holds an accepted
//              row at all (one ballot finds them: a selective mask leaves most words empty), ONE LANE TAKES ONE BIT: list[base(w) + popcount(word & ((1 << j) - 1))] = 64 w + j for a set bit, consecutive ranks from consecutive
//              lanes.  The same wavefront pads its share of [total, L) with -1.
// Bits at and beyond n count as clear and words past ceil(n / 64) are never read: callers hand over bitmaps with junk there.
//
// List ADC.  fa_adc_list is the store form of adc_mq_kernel (k_adc_mq.hip) with row = list[i]: the tables of four queries are
// interleaved in LDS — entry (m, code) is one FaF4 {q0, q1, q2, q3} — and cycled in slices of 16 SLCH subspaces, while each lane keeps
// the running sums of its R list entries x 4 queries in registers.  Per (query, row) the additions happen in ascending m into one
// f32: the association of DefaultVectorUtilSupport.assembleAndSum, so the scores are bit-identical to the scalar reference and to
// adc_mq_kernel.  A lane loads each of its list entries once (consecutive lanes, consecutive entries) and the code bytes of a slice
// with 16-byte loads.  The slice loop is restated here, not shared: the registers of k_adc_mq.hip's kernels are pinned by a baseline.
#pragma once

#include <cstdint>

#include "fa_params.h"
#include "gs_body.h"

namespace jv {

// word w of mask m as the scan sees it: nothing at and beyond n, nothing past the last word
GS_FN uint64_t fa_word(const FaScanParams &p, int64_t m, int64_t w)
{
    if (w * 64 >= p.n) return 0ull;
    uint64_t v = p.bits[m * p.stride_words + w];
    const int64_t left = p.n - w * 64;
    if (left < 64) v &= (1ull << left) - 1ull;
    return v;
}

// scan block b of mask m: its number of accepted rows into block_base[m][b]
GS_FN void fa_sums(const FaScanParams &p, int64_t m, int64_t b)
{
    const int lane = gs_lane();
    uint32_t c = 0;
    for (int i = 0; i < FA_SCAN_WORDS / 64; ++i) c += (uint32_t)gs_popc(fa_word(p, m, b * FA_SCAN_WORDS + i * 64 + lane));
    uint32_t total = 0;
    for (int s = 0; s < 64; ++s) total += gs_bcast32(c, s);
    if (lane == 0) p.block_base[m * p.blocks + b] = total;
}

// one wave per mask: block_base[m] becomes its own exclusive prefix; totals[m] is set
GS_FN void fa_scan(const FaScanParams &p, int64_t m)
{
    const int lane = gs_lane();
    uint32_t *bb = p.block_base + m * p.blocks;
    uint32_t running = 0;
    for (int64_t base = 0; base < p.blocks; base += 64) {
        const int64_t b = base + lane;
        const uint32_t c = b < p.blocks ? bb[b] : 0u;
        uint32_t before = 0, total = 0;
        for (int s = 0; s < 64; ++s) {
            const uint32_t cs = gs_bcast32(c, s);
            before += s < lane ? cs : 0u;
            total += cs;
        }
        if (b < p.blocks) bb[b] = running + before;
        running += total;
    }
    if (lane == 0) p.totals[m] = running;
}

// words [64 seg, 64 seg + 64) of list row y's mask: the ordinals of their accepted rows, and the row's share of the -1 padding
GS_FN void fa_write(const FaScanParams &p, int64_t y, int64_t seg)
{
    const int lane = gs_lane();
    const int64_t m = p.stride_words ? p.first_mask + y : 0;
    int32_t *list = p.lists + y * p.L;
    const int64_t b = seg / (FA_SCAN_WORDS / 64);
    const int q = (int)(seg - b * (FA_SCAN_WORDS / 64));   // wave-uniform: 64-word pieces of the scan block before this one
    uint32_t c = 0;
    for (int i = 0; i < q; ++i) c += (uint32_t)gs_popc(fa_word(p, m, b * FA_SCAN_WORDS + i * 64 + lane));
    const uint64_t w = fa_word(p, m, seg * 64 + lane);
    const uint32_t wc = (uint32_t)gs_popc(w);
    uint32_t before = 0, prior = 0;
    for (int s = 0; s < 64; ++s) {
        const uint32_t cs = gs_bcast32(wc, s);
        before += s < lane ? cs : 0u;
        prior += gs_bcast32(c, s);
    }
    const uint32_t base = p.block_base[m * p.blocks + b] + prior + before;   // the rank of the first set bit of this lane's word
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t todo = gs_ballot(w != 0ull);   // the words that hold an accepted row at all (fa_word: none past the last word); wave-uniform
    while (todo != 0ull) {
        const int s = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int64_t row = (seg * 64 + s) * 64 + lane;
        const uint64_t word = (uint64_t)gs_shfl((long long)w, s);
        const uint32_t wb = gs_bcast32(base, s);
        const int64_t rank = (int64_t)wb + gs_popc(word & below);
        if (((word >> lane) & 1ull) != 0 && rank < p.L) list[rank] = (int32_t)row;   // (a set bit lies below n; L holds every mask's total)
    }
    // [total, L) is at most as long as the segments together cover: segment seg pads entries total + [seg, seg + 1) FA_SEG_ROWS
    const int64_t total = p.totals[m];
    for (int s = 0; s < 64; ++s) {
        const int64_t at = total + seg * FA_SEG_ROWS + s * 64 + lane;
        if (at - lane >= p.L) break;    // wave-uniform
        if (at < p.L) list[at] = -1;
    }
}

// list entries [T R tile, T R (tile + 1)) for queries [4 group, 4 group + 4): out[q][i] = similarity(q, codes[list[i]])
template <int VSF, int SLCH, int R, int T>
GS_FN void fa_adc_list(const FaAdcParams &p, int group, int64_t tile, FaF4 *lds4)
{
    constexpr int SL = 16 * SLCH;   // subspaces per LDS slice
    const int q0 = group * FA_P;
    const int64_t tile_base = tile * (int64_t)(T * R);
    const int tid = gs_tid();
    const int nslices = p.M / SL;

    float acc[R][FA_P];
    int32_t row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int j = 0; j < FA_P; ++j) acc[r][j] = 0.0f;
        const int64_t i = tile_base + (int64_t)r * T + tid;
        const int32_t e = i < p.count ? p.list[i] : -1;
        row[r] = (e >= 0 && e < p.n) ? e : -1;
    }

    // per-query table bases (queries past Q read query Q-1's table; their results are discarded)
    const float *lq[FA_P];
#pragma unroll
    for (int j = 0; j < FA_P; ++j) {
        const int q = q0 + j < p.Q ? q0 + j : p.Q - 1;
        lq[j] = p.luts + (int64_t)q * p.M * FA_CLUSTERS;
    }

    for (int s = 0; s < nslices; ++s) {
        gs_block_barrier();   // readers of the previous slice are done
        const int mb = s * SL;
        for (int idx = tid; idx < SL * FA_CLUSTERS; idx += T) {
            const int off = mb * FA_CLUSTERS + idx;
            FaF4 t;
            t.x = lq[0][off];
            t.y = lq[1][off];
            t.z = lq[2][off];
            t.w = lq[3][off];
            lds4[idx] = t;
        }
        gs_block_barrier();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (row[r] < 0) continue;
            const FaU4 *rp = reinterpret_cast<const FaU4 *>(p.codes + (int64_t)row[r] * p.M + mb);
            FaU4 w[SLCH];
#pragma unroll
            for (int c = 0; c < SLCH; ++c) w[c] = rp[c];
#pragma unroll
            for (int c = 0; c < SLCH; ++c) {
                const uint32_t d[4] = {w[c].x, w[c].y, w[c].z, w[c].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int m = c * 16 + e * 4 + b;
                        const uint32_t code = (d[e] >> (8 * b)) & 0xFFu;
                        const FaF4 t = lds4[m * FA_CLUSTERS + code];
                        acc[r][0] += t.x;
                        acc[r][1] += t.y;
                        acc[r][2] += t.z;
                        acc[r][3] += t.w;
                    }
                }
            }
        }
    }

#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = tile_base + (int64_t)r * T + tid;
        if (i >= p.count) continue;
        const bool ok = row[r] >= 0;
        const float nrm = (VSF == 2 && ok) ? p.norms[row[r]] : 0.0f;
#pragma unroll
        for (int j = 0; j < FA_P; ++j) {
            const int q = q0 + j;
            if (q >= p.Q) continue;
            const float bm = VSF == 2 ? p.bmag[q] : 0.0f;
            p.out[(int64_t)q * p.L + i] = ok ? gs_finish<VSF>(acc[r][j], nrm, bm) : -__builtin_inff();
        }
    }
}

// cell i: a list position becomes the ordinal it holds; -1 (no result) stays -1
GS_FN void fa_map(const FaMapParams &p, int64_t i)
{
    if (i >= p.cells) return;
    const int32_t at = p.ids[i];
    p.ids[i] = (at >= 0 && at < p.count) ? p.list[at] : -1;
}

}  // namespace jv
