// xg_params.h — launch parameters of the exact-score graph traversal (xg_body.h / k_exact_gsearch.hip), shared with the host front end
// in exact_graph.cpp.  Plain data only.
#pragma once

#include "gw_params.h"

struct ihipStream_t;

namespace jv {

constexpr int XG_TILE_FLOATS = 64 * 68;   // the score phase's LDS tile: 64 x (64 + 4), 32 x (128 + 4) or 16 x (256 + 4) dwords, the largest
constexpr int XG_GROUP = 64;              // fresh neighbours scored together: one lane per row

struct XgParams : GwParams {   // rerankK: beamK; out_scores: the kept results' exact scores
    const float *rows;         // [n][D] float rows
    const float *vnorm;        // [n] per-row sums of squares (launch_row_sqnorms); COSINE with the transposing score phase only
    const float *queries;      // [Q][D]
    const float *qnorm;        // [Q] query sums of squares (launch_query_sqnorms); COSINE only
    int32_t D;
};

// LDS bytes of one worker: [score tile][64 fresh ids][results][candidate tier][64 samples][visited table (if it fits)].  The query takes
// none: it is wave-uniform and comes through scalar loads.
constexpr size_t xg_lds_bytes(int beamK, int cand_cap, int vcap_log2 /* 0 = SAFE */)
{
    return gw_lds_bytes(beamK, cand_cap, vcap_log2) + sizeof(float) * XG_TILE_FLOATS + sizeof(int32_t) * XG_GROUP;
}

// k_exact_gsearch.hip (libjvector_hip_xg.so).  vsf: VSF_L2 / VSF_DOT / VSF_COS.  tr: the transposing score phase (rows 16-byte aligned,
// D % 8 == 0), else a lane walks its own row.  Returns JV_OK, JV_ERR_INVALID (bad parameters), JV_ERR_UNSUPPORTED (LDS) or JV_ERR_HIP.
int launch_exact_graph_search(ihipStream_t *s, const XgParams &p, size_t p_bytes, int vsf, bool tr, int workers, bool safe);

}  // namespace jv
