// bd_emu.cpp — compiles the BQ robust prune body (jvector_amd/csrc/bd_body.h) and the BQ graph traversal body (bg_body.h, for the
// node-seeded search with self-exclusion) for the lane emulator.  TEST HARNESS: g++ -O2 -ffp-contract=off, never linked into the
// product.  The wave API, the traversal's Launch / lane_main and bg_emu_search are bg_emu.cpp's, taken in unchanged.
#include "bg_emu.cpp"

#include "../../jvector_amd/csrc/bd_body.h"

namespace {
struct BdLaunch {
    const jv::BdParams *p;
    int wt, node;
    char *lds;
};
void bd_lane_main(void *arg)
{
    const BdLaunch &L = *(const BdLaunch *)arg;
    switch (L.wt) {   // widths k_bq_retain.hip compiles, and the generic form
    case 0: jv::bd_node<0>(*L.p, L.node, L.lds); break;
    case 1: jv::bd_node<1>(*L.p, L.node, L.lds); break;
    case 2: jv::bd_node<2>(*L.p, L.node, L.lds); break;
    case 12: jv::bd_node<12>(*L.p, L.node, L.lds); break;
    case 16: jv::bd_node<16>(*L.p, L.node, L.lds); break;
    default: abort();
    }
}
}  // namespace

// wt: the compiled row width to run (must equal W) or 0 for the generic form.  alpha goes into the parameter block as it is given, the
// values jv_hip_bq_retain_diverse refuses included: the body has to end its rounds by itself.  Returns 0, -1 on bad arguments, -3 if a node wrote past
// its LDS block.
extern "C" int bd_emu_retain(const uint64_t *rows, int64_t n, int D, int W, const int32_t *cand_nodes, const float *cand_scores,
                             const int32_t *cand_count, const int32_t *diverse_before, int P, int C, int maxDegree, float alpha, int wt,
                             int32_t *selected_out, int32_t *n_selected_out, float *short_edges_out)
{
    if (C < 1 || C > jv::BD_MAX_CANDIDATES || maxDegree < 1 || maxDegree > 64 || (wt != 0 && wt != W)) return -1;
    jv::BdParams p{};
    p.rows = rows; p.n = n; p.D = D; p.W = W; p.cand_nodes = cand_nodes; p.cand_scores = cand_scores; p.cand_count = cand_count;
    p.diverse_before = diverse_before; p.P = P; p.C = C; p.maxDegree = maxDegree; p.alpha = alpha;
    p.selected_out = selected_out; p.n_selected_out = n_selected_out; p.short_edges_out = short_edges_out;
    const size_t lds_bytes = jv::bd_lds_bytes(C, W);
    char *lds = (char *)aligned_alloc(64, (lds_bytes + 63) / 64 * 64 + 64);
    int rc = 0;
    for (int node = 0; node < P && rc == 0; ++node) {
        memset(lds, 0xa5, lds_bytes);         // stale LDS must never reach a result
        memset(lds + lds_bytes, 0x3c, 64);    // canary behind the block
        BdLaunch L{&p, wt, node, lds};
        emu::run_wave(bd_lane_main, &L);
        for (int i = 0; i < 64; ++i)
            if (lds[lds_bytes + i] != 0x3c) rc = -3;
    }
    free(lds);
    return rc;
}

// bg_emu_search with the query words of item q = row nodes[q] and, if exclude_self, BgParams::exclude = nodes.  One level-0-only or
// layered graph as there; FAST form (safe = 0) or SAFE form (safe = 1); qmap as there.
extern "C" long bd_emu_search_nodes(int n_levels, const int32_t *const *lv_nodes, const int32_t *const *lv_nbrs, const int32_t *lv_count,
                                    const int32_t *lv_degree, int entry_node, int entry_level, int n_nodes, const uint64_t *rows_in, int D, int W,
                                    const int32_t *nodes, int Q, int rerankK, int exclude_self, int safe, int vcap_log2, int cand_cap,
                                    int spill_cap, int workers, int wt, const int32_t *qmap, int n_items, int32_t *out_ids, float *out_scores,
                                    long long *out_stats, int32_t *out_status)
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
    uint64_t *rows = (uint64_t *)aligned_alloc(64, ((sizeof(uint64_t) * (size_t)n_nodes * W + 63) / 64 + 1) * 64);
    uint64_t *qwords = (uint64_t *)aligned_alloc(64, ((sizeof(uint64_t) * (size_t)Q * W + 63) / 64 + 1) * 64);
    memcpy(rows, rows_in, sizeof(uint64_t) * (size_t)n_nodes * W);
    for (int q = 0; q < Q; ++q) memcpy(qwords + (size_t)q * W, rows_in + (size_t)nodes[q] * W, sizeof(uint64_t) * (size_t)W);
    p.entry_node = entry_node;
    p.entry_level = entry_level;
    p.n_nodes = n_nodes;
    p.rows = rows;
    p.qwords = qwords;
    p.D = D;
    p.W = W;
    p.rerankK = rerankK;
    p.qmap = qmap;
    p.exclude = exclude_self ? nodes : nullptr;
    p.vcap_log2 = safe ? 0 : vcap_log2;
    p.cand_cap = cand_cap;
    p.spill_cap = safe ? n_nodes + 64 : spill_cap;
    p.bitmap_words = ((n_nodes + 31) / 32 + 3) / 4 * 4;
    const size_t vcap = safe ? 4 : (size_t)1 << vcap_log2;
    int32_t *visited = (int32_t *)aligned_alloc(64, sizeof(int32_t) * vcap * workers + 64);
    uint32_t *bitmap = (uint32_t *)aligned_alloc(64, sizeof(uint32_t) * (size_t)p.bitmap_words * workers + 64);
    long long *spill = (long long *)aligned_alloc(64, sizeof(long long) * (size_t)(p.spill_cap > 0 ? p.spill_cap : 1) * workers + 64);
    memset(visited, 0x5a, sizeof(int32_t) * vcap * workers);
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
    for (int w = 0; w < workers; ++w) {
        jv::BgParams pw = p;
        pw.Q = (int)((long long)items * (w + 1) / workers);
        const size_t lds_bytes = jv::bg_lds_bytes(rerankK, cand_cap, wt ? 0 : W, p.vcap_log2);
        char *lds = (char *)aligned_alloc(64, (lds_bytes + 63) / 64 * 64 + 64);
        memset(lds, 0xa5, lds_bytes);
        Launch L{&pw, wt, safe, w, lds};
        collectives += emu::run_wave(lane_main, &L);
        next = (uint32_t)pw.Q;
        free(lds);
    }
    free(visited);
    free(bitmap);
    free(spill);
    free(rows);
    free(qwords);
    return collectives;
}
