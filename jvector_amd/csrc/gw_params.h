// gw_params.h — what the one-wave graph walks (gw_body.h) share of their launch parameters: the graph, the work list, the filters, the
// visited structures, the candidate tiers and the outputs.  BgParams (bg_params.h) and XgParams (xg_params.h) derive from it and add
// their rows and queries; the host driver in graph_walk.cpp fills this part.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

#include "gs_params.h"

namespace jv {

constexpr int BG_VIS_LDS_MAX_LOG2 = 13;   // 8192 entries = 32 KB
constexpr int BG_MIN_VCAP_LOG2 = 8, BG_MAX_VCAP_LOG2 = 24;
constexpr int BG_MIN_CAND_CAP = 128;      // gw_partition samples 64 keys of a full tier

// (The order of the fields is a measured one, here and in BgParams: the kernels fetch their arguments with merged scalar loads, and the
// order decides how many SGPRs those keep alive; DESIGN.md §9 "One walk, one driver" has the figures.)
struct GwParams {
    GsLevel lv[GS_MAX_LEVELS];
    int32_t entry_node, entry_level;
    int32_t n_nodes;           // rows a neighbour id may name (a caller-owned level 0 is not validated by the host: ids beyond are skipped)
    int32_t Q, rerankK;        // work items; length of the kept list, GraphSearcher's rerankK (exact: beamK)
    const int32_t *qmap;       // nullptr: work items are the query indices; else item i runs query qmap[i] (the SAFE pass)
    const unsigned long long *accept;   // acceptOrds bit array or nullptr; layer 0 only
    long long accept_stride;
    const int32_t *exclude;    // nullptr: off; else [Q] node ids: query q traverses node exclude[q] at layer 0 but never keeps it — the accept
                               // mask of query q with that one bit cleared (the node-seeded searches, exclude_self)
    int32_t vcap_log2;         // FAST: log2 of the visited table's slots
    int32_t *visited;          // FAST, vcap_log2 > BG_VIS_LDS_MAX_LOG2: [workers][1 << vcap_log2]
    uint32_t *bitmap;          // SAFE: [workers][bitmap_words]
    long long bitmap_words;    // a multiple of 4, >= ceil(n_nodes / 32)
    int32_t *out_ids;          // [Q][rerankK] kept results (unordered), -1 padded
    float *out_scores;         // [Q][rerankK] their scores (BQ similarities / exact scores), -inf padded
    long long *out_stats;      // [Q][2] visitedCount, expandedCount
    int32_t *out_status;       // [Q] GS_OK / GS_OVERFLOW
    uint32_t *next_query;      // work counter (zeroed by the host before the launch)
    int32_t cand_cap;          // LDS tier of the candidates
    long long *spill;          // [workers][spill_cap]: spill tier from the front, evicted list from the back
    int32_t spill_cap;
};

// LDS bytes of the walk's own structures: [results][candidate tier][64 samples] + [visited table (if it fits)]
constexpr size_t gw_lds_bytes(int K, int cand_cap, int vcap_log2 /* 0 = SAFE */)
{
    return sizeof(long long) * ((size_t)K + (size_t)cand_cap + 64) + ((vcap_log2 > 0 && vcap_log2 <= BG_VIS_LDS_MAX_LOG2) ? ((size_t)4 << vcap_log2) : 0);
}

}  // namespace jv
