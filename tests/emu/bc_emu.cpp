// bc_emu.cpp — compiles the BQ builder's compaction bodies (jvector_amd/csrc/bc_body.h: the three steps of the rank, the adjacency gather
// and the BQ row gather) for the lane emulator.  TEST HARNESS: g++ -O2 -ffp-contract=off, never linked into the product.  The wave API
// is bg_emu.cpp's, taken in unchanged.
#include "bg_emu.cpp"

#include "../../jvector_amd/csrc/bc_body.h"

namespace {
struct BcLaunch {
    const jv::BcParams *p;
    int step;
    int64_t index;
};
void bc_lane_main(void *arg)
{
    const BcLaunch &L = *(const BcLaunch *)arg;
    switch (L.step) {
    case 0: return jv::bc_rank_sums(*L.p, L.index);
    case 1: return jv::bc_rank_scan(*L.p);
    case 2: return jv::bc_rank_write(*L.p, L.index);
    case 3: return jv::bc_rows(*L.p, L.index);
    case 4: return jv::bc_bq_rows(*L.p, L.index);
    default: abort();
    }
}
void run(const jv::BcParams &p, int step, int64_t waves)
{
    for (int64_t i = 0; i < waves; ++i) {
        BcLaunch L{&p, step, i};
        emu::run_wave(bc_lane_main, &L);
    }
}
}  // namespace

extern "C" int bc_emu_scan_nodes() { return jv::BC_SCAN_NODES; }

// the three launches of launch_bq_compact_rank.  present: ceil(n / 64) words (the last may carry garbage at and beyond n);
// old_to_new [n]; new_to_old (nullable) [set bits]; counters_out [3].  Returns 0, -1 on bad arguments.
extern "C" int bc_emu_rank(const uint64_t *present, int64_t n, int32_t *old_to_new, int32_t *new_to_old, uint32_t *counters_out)
{
    if (n < 1 || n > 0x7fffffffLL) return -1;
    std::vector<uint32_t> base((size_t)jv::bc_scan_blocks(n), 0xdeadbeefu);   // garbage: every word must be written before it is read
    jv::BcParams p{};
    p.present = present; p.n = n; p.block_base = base.data(); p.counters = counters_out; p.old_to_new = old_to_new; p.new_to_old = new_to_old;
    run(p, 0, jv::bc_scan_blocks(n));
    run(p, 1, 1);
    run(p, 2, ((n + 63) / 64 + 63) / 64);
    return 0;
}

// launch_bq_compact_rows and launch_bq_compact_bq_rows over the maps of bc_emu_rank.  counters [3] as the rank left them ([1], [2] are
// updated).  dst_* hold at least live rows.  Returns 0, -1 on bad arguments.
extern "C" int bc_emu_rows(int64_t n, int64_t live, int R, const int32_t *old_to_new, const int32_t *new_to_old, const int32_t *src_nbrs,
                           const float *src_nsc, const int32_t *src_db, int32_t *dst_nbrs, float *dst_nsc, int32_t *dst_db, int W,
                           const uint64_t *src_rows, uint64_t *dst_rows, uint32_t *counters)
{
    if (n < 1 || live < 0 || live > n || R < 1 || R > 64 || W < 1) return -1;
    jv::BcParams p{};
    p.n = n; p.live = live; p.R = R; p.counters = counters; p.old_to_new = (int32_t *)old_to_new; p.new_to_old = (int32_t *)new_to_old;
    p.src_nbrs = src_nbrs; p.src_nsc = src_nsc; p.src_db = src_db; p.dst_nbrs = dst_nbrs; p.dst_nsc = dst_nsc; p.dst_db = dst_db;
    p.W = W; p.src_rows = src_rows; p.dst_rows = dst_rows;
    run(p, 3, jv::bc_wave_count(live * R));
    run(p, 4, jv::bc_wave_count(live * W));
    return 0;
}
