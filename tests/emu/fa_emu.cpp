// fa_emu.cpp — compiles the filtered flat search's bodies (jvector_amd/csrc/fa_body.h: the three steps of the mask compaction, the list
// ADC scan and the position map) for the lane emulator.  TEST HARNESS: g++ -O2 -ffp-contract=off, never linked into the product.  The
// wave API is bg_emu.cpp's, taken in unchanged.  The list ADC body runs as a workgroup of four wavefronts (the emulator's largest): its
// thread count is a template parameter, the device instantiates 1024.
#include "bg_emu.cpp"

#include "../../jvector_amd/csrc/fa_body.h"

namespace {
constexpr int EMU_T = 256;

struct FaLaunch {
    const jv::FaScanParams *p;
    int step;
    int64_t y, index;
};
void fa_lane_main(void *arg)
{
    const FaLaunch &L = *(const FaLaunch *)arg;
    switch (L.step) {
    case 0: return jv::fa_sums(*L.p, L.y, L.index);
    case 1: return jv::fa_scan(*L.p, L.y);
    case 2: return jv::fa_write(*L.p, L.y, L.index);
    default: abort();
    }
}
void run(const jv::FaScanParams &p, int step, int64_t ys, int64_t waves)
{
    for (int64_t y = 0; y < ys; ++y)
        for (int64_t i = 0; i < waves; ++i) {
            FaLaunch L{&p, step, y, i};
            emu::run_wave(fa_lane_main, &L);
        }
}
void count(jv::FaScanParams &p, int masks, std::vector<uint32_t> &base, uint32_t *totals)
{
    p.blocks = jv::fa_scan_blocks(p.n);
    base.assign((size_t)(masks * p.blocks), 0xdeadbeefu);   // garbage: every word must be written before it is read
    p.block_base = base.data();
    p.totals = totals;
    run(p, 0, masks, p.blocks);
    run(p, 1, masks, 1);
}

struct AdcLaunch {
    const jv::FaAdcParams *p;
    int vsf, slch, R, group;
    int64_t tile;
    jv::FaF4 *lds;
};
template <int VSF, int SLCH>
void adc_r(const AdcLaunch &L)
{
    if (L.R == 8) jv::fa_adc_list<VSF, SLCH, 8, EMU_T>(*L.p, L.group, L.tile, L.lds);
    else jv::fa_adc_list<VSF, SLCH, 4, EMU_T>(*L.p, L.group, L.tile, L.lds);
}
template <int VSF>
void adc_slch(const AdcLaunch &L)
{
    if (L.slch == 2) adc_r<VSF, 2>(L);
    else adc_r<VSF, 1>(L);
}
void adc_lane_main(void *arg)
{
    const AdcLaunch &L = *(const AdcLaunch *)arg;
    switch (L.vsf) {
    case 0: return adc_slch<0>(L);
    case 1: return adc_slch<1>(L);
    case 2: return adc_slch<2>(L);
    default: abort();
    }
}

struct MapLaunch {
    const jv::FaMapParams *p;
    int64_t wave;
};
void map_lane_main(void *arg)
{
    const MapLaunch &L = *(const MapLaunch *)arg;
    jv::fa_map(*L.p, L.wave * 64 + gs_lane());
}
}  // namespace

extern "C" int fa_emu_scan_rows() { return jv::FA_SCAN_ROWS; }
extern "C" int fa_emu_tile(int R) { return EMU_T * R; }

// launch_flat_accept_count: bits holds stride_words * (masks - 1) + ceil(n / 64) words; totals [masks].  Returns 0, -1 on bad arguments.
extern "C" int fa_emu_count(const uint64_t *bits, int64_t stride_words, int64_t n, int masks, uint32_t *totals)
{
    if (n < 1 || n > 0x7fffffffLL || masks < 1 || (masks > 1 && stride_words < (n + 63) / 64)) return -1;
    jv::FaScanParams p{};
    p.bits = bits; p.stride_words = stride_words; p.n = n;
    std::vector<uint32_t> base;
    count(p, masks, base, totals);
    return 0;
}

// the count again, then launch_flat_accept_write: lists [rows][L], row y from mask first_mask + y (mask 0 when stride_words == 0)
extern "C" int fa_emu_lists(const uint64_t *bits, int64_t stride_words, int64_t n, int masks, int first_mask, int rows, int64_t L, int32_t *lists)
{
    if (n < 1 || n > 0x7fffffffLL || masks < 1 || rows < 1 || L < 1 || L > jv::fa_segments(n) * jv::FA_SEG_ROWS) return -1;
    if (stride_words ? first_mask + rows > masks : masks != 1) return -1;
    jv::FaScanParams p{};
    p.bits = bits; p.stride_words = stride_words; p.n = n;
    std::vector<uint32_t> base, totals((size_t)masks, 0xdeadbeefu);
    count(p, masks, base, totals.data());
    p.first_mask = first_mask; p.lists = lists; p.L = L;
    run(p, 2, rows, jv::fa_segments(n));
    return 0;
}

// launch_flat_accept_adc_list with workgroups of 256 lanes: out [Q][L], columns [0, count) are written
extern "C" int fa_emu_adc(const float *luts, const float *bmag, const uint8_t *codes_in, const float *norms, const int32_t *list, int64_t count,
                          int64_t n, int64_t L, int Q, int M, int vsf, int R, float *out)
{
    if (Q < 1 || M < 16 || M % 16 != 0 || count < 0 || count > L || vsf < 0 || vsf > 2 || (R != 4 && R != 8)) return -1;
    uint8_t *codes = (uint8_t *)aligned_alloc(64, ((size_t)n * M + 63) / 64 * 64 + 64);   // rows are read as 16-byte words
    memcpy(codes, codes_in, (size_t)n * M);
    const int slch = M % 32 == 0 ? 2 : 1;
    const size_t lds_bytes = jv::fa_adc_lds_bytes(slch);
    char *lds = (char *)aligned_alloc(64, lds_bytes + 64);
    jv::FaAdcParams p{};
    p.luts = luts; p.bmag = bmag; p.codes = codes; p.norms = norms; p.list = list; p.out = out;
    p.n = n; p.count = count; p.L = L; p.Q = Q; p.M = M;
    bool bad = false;
    const int64_t tiles = (count + EMU_T * R - 1) / (EMU_T * R);
    for (int g = 0; g < (Q + jv::FA_P - 1) / jv::FA_P; ++g)
        for (int64_t t = 0; t < tiles; ++t) {
            memset(lds, 0xa5, lds_bytes);
            memset(lds + lds_bytes, 0x3c, 64);   // canary behind the block
            AdcLaunch A{&p, vsf, slch, R, g, t, (jv::FaF4 *)lds};
            emu::run_block(adc_lane_main, &A, EMU_T / 64);
            for (int i = 0; i < 64; ++i) bad = bad || lds[lds_bytes + i] != 0x3c;
        }
    free(lds);
    free(codes);
    return bad ? -3 : 0;
}

extern "C" int fa_emu_map(const int32_t *list, int64_t count, int32_t *ids, int64_t cells)
{
    if (cells < 0 || count < 0) return -1;
    jv::FaMapParams p{};
    p.list = list; p.ids = ids; p.cells = cells; p.count = count;
    for (int64_t w = 0; w < (cells + 63) / 64; ++w) {
        MapLaunch M{&p, w};
        emu::run_wave(map_lane_main, &M);
    }
    return 0;
}
