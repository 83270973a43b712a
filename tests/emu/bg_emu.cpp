// bg_emu.cpp — compiles the BQ graph traversal body (jvector_amd/csrc/bg_body.h) for the lane emulator and exposes one C entry
// point to the CPU tests.  TEST HARNESS: g++ -O2 -ffp-contract=off, never linked into the product.  The wave API below is
// gs_emu.cpp's.
#include <vector>

#include "hip_emu.h"

#define GS_FN inline
#define GS_SCHED_FENCE() ((void)0)
#define GS_NOINLINE static
#define GS_LDS_AS
#define GS_GLOBAL_AS
static inline int gs_lane() { return emu::lane(); }
// gs_body.h's sync point is wave-scope here: in a one-wave block (every form but WGX) that IS the block barrier, and in the
// workgroup form (gx_body.h) the control wave must not wait for the expander waves
static inline void gs_barrier() { emu::wave_barrier(); }
static inline int gs_tid() { return emu::lane(); }
static inline int gs_block_threads() { return emu::current()->nl; }
static inline void gs_block_barrier() { emu::barrier(); }
// LDS flags between waves: plain accesses (one host thread runs all lanes); a spin-wait must let the other lanes run
static inline int32_t gs_lds_load(const int32_t *p) { return *(const volatile int32_t *)p; }
static inline void gs_lds_store(int32_t *p, int32_t v) { *(volatile int32_t *)p = v; }
static inline int32_t gs_lds_add(int32_t *p, int32_t v)
{
    const int32_t old = *p;
    *p = old + v;
    return old;
}
static inline void gs_spin_pause() { emu::switch_to_next_live(); }
static inline uint64_t gs_ballot(bool p) { return emu::ballot(p); }
static inline long long gs_shfl(long long v, int src) { return emu::shfl(v, src); }
static inline uint32_t gs_bcast32(uint32_t v, int src) { return (uint32_t)emu::shfl((long long)v, src); }
static inline long long gs_shfl_xor(long long v, int m) { return emu::shfl(v, emu::lane() ^ m); }
static inline int32_t gs_shfl32(int32_t v, int src) { return (int32_t)emu::shfl((long long)v, src); }
static inline uint32_t gs_perm(uint32_t hi, uint32_t lo, uint32_t sel)   // v_perm_b32 (selectors 0..7 and 0x0c only)
{
    const uint64_t pool = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t sb = (sel >> (8 * i)) & 0xFFu;
        const uint32_t byte = sb < 8 ? (uint32_t)((pool >> (8 * sb)) & 0xFFu) : (sb == 0x0c ? 0u : 0xFFu);
        r |= byte << (8 * i);
    }
    return r;
}
#define GS_OPAQUE_I32(x) ((void)0)
static inline int32_t gs_cas(int32_t *p, int32_t expect, int32_t desired)
{
    const int32_t old = *p;
    if (old == expect) *p = desired;
    return old;
}
static inline uint32_t gs_lds_cas(uint32_t *p, uint32_t expect, uint32_t desired)
{
    const uint32_t old = *p;
    if (old == expect) *p = desired;
    return old;
}
static inline void gs_prefetch_lds(const void *g, void *lds)
{
    // the emulated lane really performs the touch: an address outside the arrays it names would fault here, and the landing
    // bytes are scribbled so that any read of them shows up as a wrong result
    ((volatile uint32_t *)lds)[emu::lane() & 63] = *(const volatile uint32_t *)g ^ 0xA5A5A5A5u;
}
static inline uint32_t gs_fetch_add(uint32_t *p, uint32_t v)
{
    const uint32_t old = *p;
    *p = old + v;
    return old;
}
static inline void gs_fetch_add64(unsigned long long *p, unsigned long long v) { *p += v; }
static inline void gs_fence() {}
static inline double gs_sqrt(double x) { return std::sqrt(x); }
static inline float gs_rsq_approx(float x) { return 1.0f / std::sqrt(x); }
static inline void gs_gather64(float v, float (&out)[64]) { emu::gather64(v, out); }

#include "../../jvector_amd/csrc/bg_body.h"
#include "../../jvector_amd/csrc/gs_host.h"

namespace {
struct Launch {
    const jv::BgParams *p;
    int wt, safe, worker;
    char *lds;
};

template <bool SAFE>
void run_wt(const Launch &L)
{
    switch (L.wt) {   // the widths k_bq_gsearch.hip compiles, and the generic form
    case 0: jv::bg_worker<0, SAFE>(*L.p, L.worker, L.lds); break;
    case 1: jv::bg_worker<1, SAFE>(*L.p, L.worker, L.lds); break;
    case 2: jv::bg_worker<2, SAFE>(*L.p, L.worker, L.lds); break;
    case 4: jv::bg_worker<4, SAFE>(*L.p, L.worker, L.lds); break;
    case 12: jv::bg_worker<12, SAFE>(*L.p, L.worker, L.lds); break;
    default: abort();
    }
}
void lane_main(void *arg)
{
    const Launch &L = *(const Launch *)arg;
    if (L.safe) run_wt<true>(L);
    else run_wt<false>(L);
}
}  // namespace

// safe = 0: the FAST form (visited table of 1 << vcap_log2 slots, spill slice of spill_cap keys); safe = 1: the SAFE form (bitmap of
// n_nodes bits, spill slice of n_nodes + 64 keys).  wt: the compiled row width to run (must equal W) or 0 for the generic form.
// qmap (nullable): n_items work items naming the queries to run; else items 0..Q-1.
extern "C" long bg_emu_search(int n_levels, const int32_t *const *lv_nodes, const int32_t *const *lv_nbrs, const int32_t *lv_count,
                              const int32_t *lv_degree, int entry_node, int entry_level, int n_nodes, const uint64_t *rows_in,
                              const uint64_t *qwords_in, int D, int W, int Q, int rerankK, const uint64_t *accept, long long accept_stride,
                              int safe, int vcap_log2, int cand_cap, int spill_cap, int workers, int wt, const int32_t *qmap, int n_items,
                              int32_t *out_ids, float *out_scores, long long *out_stats, int32_t *out_status)
{
    if (n_levels < 1 || n_levels > jv::GS_MAX_LEVELS || cand_cap < jv::BG_MIN_CAND_CAP || (wt != 0 && wt != W)) return -1;
    if (!safe && (vcap_log2 < jv::BG_MIN_VCAP_LOG2 || vcap_log2 > jv::BG_MAX_VCAP_LOG2)) return -2;
    jv::BgParams p{};
    std::vector<jv::GsLevelMap> maps((size_t)n_levels);
    for (int l = 0; l < n_levels; ++l) {
        p.lv[l].nbrs = lv_nbrs[l];
        p.lv[l].count = lv_count[l];
        p.lv[l].degree = lv_degree[l];
        if (l > 0) {
            maps[l] = jv::gs_build_level_map(lv_nodes[l], lv_count[l]);
            p.lv[l].hkeys = maps[l].keys.data();
            p.lv[l].hvals = maps[l].vals.data();
            p.lv[l].hmask = maps[l].mask;
            p.lv[l].hshift = maps[l].shift;
        }
    }
    // 16-byte aligned copies: rows of an even width are read as 16-byte words
    uint64_t *rows = (uint64_t *)aligned_alloc(64, ((sizeof(uint64_t) * (size_t)n_nodes * W + 63) / 64 + 1) * 64);
    uint64_t *qwords = (uint64_t *)aligned_alloc(64, ((sizeof(uint64_t) * (size_t)Q * W + 63) / 64 + 1) * 64);
    memcpy(rows, rows_in, sizeof(uint64_t) * (size_t)n_nodes * W);
    memcpy(qwords, qwords_in, sizeof(uint64_t) * (size_t)Q * W);
    p.entry_node = entry_node;
    p.entry_level = entry_level;
    p.n_nodes = n_nodes;
    p.rows = rows;
    p.qwords = qwords;
    p.D = D;
    p.W = W;
    p.rerankK = rerankK;
    p.qmap = qmap;
    p.accept = (const unsigned long long *)accept;
    p.accept_stride = accept_stride;
    p.vcap_log2 = safe ? 0 : vcap_log2;
    p.cand_cap = cand_cap;
    p.spill_cap = safe ? n_nodes + 64 : spill_cap;
    p.bitmap_words = ((n_nodes + 31) / 32 + 3) / 4 * 4;
    const size_t vcap = safe ? 4 : (size_t)1 << vcap_log2;
    int32_t *visited = (int32_t *)aligned_alloc(64, sizeof(int32_t) * vcap * workers + 64);
    uint32_t *bitmap = (uint32_t *)aligned_alloc(64, sizeof(uint32_t) * (size_t)p.bitmap_words * workers + 64);
    long long *spill = (long long *)aligned_alloc(64, sizeof(long long) * (size_t)(p.spill_cap > 0 ? p.spill_cap : 1) * workers + 64);
    memset(visited, 0x5a, sizeof(int32_t) * vcap * workers);   // garbage: the kernel must clear what it uses itself
    memset(bitmap, 0x5a, sizeof(uint32_t) * (size_t)p.bitmap_words * workers);
    p.visited = visited;
    p.bitmap = bitmap;
    p.spill = spill;
    p.out_ids = out_ids;
    p.out_scores = out_scores;
    p.out_stats = out_stats;
    p.out_status = out_status;
    uint32_t next = 0;
    p.next_query = &next;
    const int items = qmap ? n_items : Q;
    long collectives = 0;
    // "workers" waves run one after another; each drains part of the queue: scratch reuse across queries and distinct slices
    for (int w = 0; w < workers; ++w) {
        jv::BgParams pw = p;
        pw.Q = (int)((long long)items * (w + 1) / workers);
        const size_t lds_bytes = jv::bg_lds_bytes(rerankK, cand_cap, wt ? 0 : W, p.vcap_log2);
        char *lds = (char *)aligned_alloc(64, (lds_bytes + 63) / 64 * 64 + 64);
        memset(lds, 0xa5, lds_bytes);
        memset(lds + lds_bytes, 0x3c, 64);   // canary behind the block
        Launch L{&pw, wt, safe, w, lds};
        collectives += emu::run_wave(lane_main, &L);
        next = (uint32_t)pw.Q;   // the drained worker overshot the counter by one
        bool bad = false;
        for (int i = 0; i < 64; ++i) bad = bad || lds[lds_bytes + i] != 0x3c;
        free(lds);
        if (bad) return -3;   // the worker wrote past its LDS block
    }
    free(visited);
    free(bitmap);
    free(spill);
    free(rows);
    free(qwords);
    return collectives;
}
