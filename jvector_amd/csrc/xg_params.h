// xg_params.h — launch parameters of the exact-score graph traversal (xg_body.h / k_exact_gsearch.hip), shared with the host driver in
// exact_graph.cpp.  Plain data only.
#pragma once

#include <cstddef>
#include <cstdint>

#include "bg_params.h"
#include "gs_params.h"

struct ihipStream_t;

namespace jv {

constexpr int XG_TILE_FLOATS = 64 * 68;   // the score phase's LDS tile: 64 x (64 + 4), 32 x (128 + 4) or 16 x (256 + 4) dwords, the largest
constexpr int XG_GROUP = 64;              // fresh neighbours scored together: one lane per row

struct XgParams {
    GsLevel lv[GS_MAX_LEVELS];
    int32_t entry_node, entry_level;
    int32_t n_nodes;           // rows of `rows` a neighbour id may name (ids beyond are skipped, as in BgParams)
    const float *rows;         // [n][D] float rows
    const float *vnorm;        // [n] per-row sums of squares (launch_row_sqnorms); COSINE with the transposing score phase only
    const float *queries;      // [Q][D]
    const float *qnorm;        // [Q] query sums of squares (launch_query_sqnorms); COSINE only
    int32_t D;
    int32_t Q, beamK;
    const int32_t *qmap;       // nullptr: work items are the query indices; else item i runs query qmap[i] (the SAFE pass)
    const unsigned long long *accept;   // acceptOrds bit array or nullptr; layer 0 only
    long long accept_stride;
    const int32_t *exclude;    // [Q] or nullptr: query q never keeps node exclude[q] at layer 0 (it is traversed and expanded as ever)
    int32_t vcap_log2;         // FAST: log2 of the visited table's slots
    int32_t *visited;          // FAST, vcap_log2 > BG_VIS_LDS_MAX_LOG2: [workers][1 << vcap_log2]
    uint32_t *bitmap;          // SAFE: [workers][bitmap_words]
    long long bitmap_words;    // a multiple of 4, >= ceil(n_nodes / 32)
    int32_t cand_cap;          // LDS tier of the candidates
    long long *spill;          // [workers][spill_cap]: spill tier from the front, evicted list from the back
    int32_t spill_cap;
    int32_t *out_ids;          // [Q][beamK] kept results (unordered), -1 padded
    float *out_scores;         // [Q][beamK] their exact scores, -inf padded
    long long *out_stats;      // [Q][2] visitedCount, expandedCount
    int32_t *out_status;       // [Q] GS_OK / GS_OVERFLOW
    uint32_t *next_query;      // work counter (zeroed by the host before the launch)
};

// LDS bytes of one worker: [results][candidate tier][64 samples][score tile][64 fresh ids][visited table (if it fits)].  The query takes
// none: it is wave-uniform and comes through scalar loads.
constexpr size_t xg_lds_bytes(int beamK, int cand_cap, int vcap_log2 /* 0 = SAFE */)
{
    return sizeof(long long) * ((size_t)beamK + (size_t)cand_cap + 64) + sizeof(float) * XG_TILE_FLOATS + sizeof(int32_t) * XG_GROUP +
           ((vcap_log2 > 0 && vcap_log2 <= BG_VIS_LDS_MAX_LOG2) ? ((size_t)4 << vcap_log2) : 0);
}

// k_exact_gsearch.hip (libjvector_hip_xg.so).  vsf: VSF_L2 / VSF_DOT / VSF_COS.  tr: the transposing score phase (rows 16-byte aligned,
// D % 8 == 0), else a lane walks its own row.  Returns JV_OK, JV_ERR_INVALID (bad parameters), JV_ERR_UNSUPPORTED (LDS) or JV_ERR_HIP.
int launch_exact_graph_search(ihipStream_t *s, const XgParams &p, size_t p_bytes, int vsf, bool tr, int workers, bool safe);

}  // namespace jv
