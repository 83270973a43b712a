// bg_params.h — launch parameters of the graph traversal over binary-quantized vectors (bg_body.h / k_bq_gsearch.hip), shared with
// the host driver in bq_graph.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

#include "gs_params.h"

namespace jv {

constexpr int BG_VIS_LDS_MAX_LOG2 = 13;   // 8192 entries = 32 KB
constexpr int BG_MIN_VCAP_LOG2 = 8, BG_MAX_VCAP_LOG2 = 24;
constexpr int BG_MIN_CAND_CAP = 128;      // bg_partition samples 64 keys of a full tier

struct BgParams {
    GsLevel lv[GS_MAX_LEVELS];
    int32_t entry_node, entry_level;
    int32_t n_nodes;           // rows of `rows` a neighbour id may name (a caller-owned level 0 is not validated by the host: ids beyond are skipped)
    const uint64_t *rows;      // [n][W] BQ rows
    const uint64_t *qwords;    // [Q][W] encoded queries
    int32_t D, W;
    int32_t Q, rerankK;
    const int32_t *qmap;       // nullptr: work items are the query indices; else item i runs query qmap[i] (the SAFE pass)
    const unsigned long long *accept;   // acceptOrds bit array or nullptr; layer 0 only
    long long accept_stride;
    const int32_t *exclude;    // nullptr: off; else [Q] node ids: query q traverses node exclude[q] at layer 0 but never keeps it — the accept
                               // mask of query q with that one bit cleared (jv_hip_bq_graph_search_nodes, exclude_self)
    int32_t vcap_log2;         // FAST: log2 of the visited table's slots
    int32_t *visited;          // FAST, vcap_log2 > BG_VIS_LDS_MAX_LOG2: [workers][1 << vcap_log2]
    uint32_t *bitmap;          // SAFE: [workers][bitmap_words]
    long long bitmap_words;    // a multiple of 4, >= ceil(n_nodes / 32)
    int32_t cand_cap;          // LDS tier of the candidates
    long long *spill;          // [workers][spill_cap]: spill tier from the front, evicted list from the back
    int32_t spill_cap;
    int32_t *out_ids;          // [Q][rerankK] kept approximate results (unordered), -1 padded
    float *out_scores;         // [Q][rerankK] their BQ similarities, -inf padded
    long long *out_stats;      // [Q][2] visitedCount, expandedCount
    int32_t *out_status;       // [Q] GS_OK / GS_OVERFLOW
    uint32_t *next_query;      // work counter (zeroed by the host before the launch)
};

// LDS bytes of one worker: [results][candidate tier][64 samples][query words (generic width only)][visited table (if it fits)]
constexpr size_t bg_lds_bytes(int rerankK, int cand_cap, int lds_query_words, int vcap_log2 /* 0 = SAFE */)
{
    return sizeof(long long) * ((size_t)rerankK + (size_t)cand_cap + 64 + (size_t)lds_query_words) +
           ((vcap_log2 > 0 && vcap_log2 <= BG_VIS_LDS_MAX_LOG2) ? ((size_t)4 << vcap_log2) : 0);
}

}  // namespace jv
