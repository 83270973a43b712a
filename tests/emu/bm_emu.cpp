// bm_emu.cpp — compiles the BQ builder's entry-point body (jvector_amd/csrc/bm_body.h: the majority row and the member nearest to it)
// for the lane emulator.  TEST HARNESS: g++ -O2 -ffp-contract=off, never linked into the product.  The wave API is bg_emu.cpp's,
// taken in unchanged.
#include "bg_emu.cpp"

#include "../../jvector_amd/csrc/bm_body.h"

namespace {
struct BmLaunch {
    const jv::BmParams *p;
    int step, index;
};
void bm_lane_main(void *arg)
{
    const BmLaunch &L = *(const BmLaunch *)arg;
    switch (L.step) {
    case 0: jv::bm_majority_word(*L.p, L.index); break;
    case 1: jv::bm_nearest_partial(*L.p, L.index); break;
    default: jv::bm_nearest_final(*L.p); break;
    }
}
}  // namespace

// the three launches of launch_bq_entry, one emulated wave per block: centroid_out [W], best_out [1] = (hamming << 32) | id.
// members nullable (rows 0..n-1).  Returns 0, -1 on bad arguments.
extern "C" int bm_emu_entry(const uint64_t *rows, int64_t n_rows, int W, const int32_t *members, int n, int waves, uint64_t *centroid_out,
                            long long *best_out)
{
    if (n < 1 || W < 1 || waves < 1) return -1;
    std::vector<long long> partial((size_t)waves, 0x5a5a5a5a5a5a5a5all);   // garbage: every slot must be written before it is read
    jv::BmParams p{};
    p.rows = rows; p.n_rows = n_rows; p.W = W; p.members = members; p.n = n; p.centroid = centroid_out; p.partial = partial.data();
    p.waves = waves; p.best = best_out;
    for (int w = 0; w < W; ++w) {
        BmLaunch L{&p, 0, w};
        emu::run_wave(bm_lane_main, &L);
    }
    for (int w = 0; w < waves; ++w) {
        BmLaunch L{&p, 1, w};
        emu::run_wave(bm_lane_main, &L);
    }
    BmLaunch L{&p, 2, 0};
    emu::run_wave(bm_lane_main, &L);
    return 0;
}
