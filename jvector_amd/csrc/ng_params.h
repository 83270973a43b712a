// ng_params.h — launch parameters of the graph traversal scored on NVQ rows (ng_body.h / k_nvq_gsearch.hip), shared with the host front
// end in nvq_graph.cpp.  Plain data only.
#pragma once

#include "gw_params.h"

struct ihipStream_t;

namespace jv {

constexpr int NG_TILE_FLOATS = 64 * 68;   // the score phase's LDS tile of decoded floats: 64 x (64 + 4), 32 x (128 + 4) or 16 x (256 + 4) dwords
constexpr int NG_GROUP = 64;              // fresh neighbours scored together: lane j owns row j in the chain phase

struct NgParams : GwParams {   // rerankK: beamK; out_scores: the kept results' NVQScorer scores
    const uint8_t *bytes;      // [n][ld] one byte per dimension, 16-byte aligned rows
    const float *derived;      // [n][S][4] {1 / scaledGrowthRate, scaledMidpoint, logisticScale, logisticBias} (nvq_derive_kernel)
    const float *cosnorm;      // [n] query-independent normalisation sums; COSINE only
    const float *mean;         // [D] globalMean; COSINE only
    const float *queries;      // [Q][D]; EUCLIDEAN: query - globalMean (nvq_query_prep_kernel's qwork)
    const float *qaux;         // [Q] DOT_PRODUCT: dotProduct(query, globalMean); COSINE: the query's magnitude
    int32_t ld, D, S;
};

// LDS bytes of one worker: [float tile][64 fresh ids][results][candidate tier][64 samples][visited table (if it fits)] — the block of the
// exact-score walk, so the largest beamK is the same.  The query takes none: it comes through scalar loads.
constexpr size_t ng_lds_bytes(int beamK, int cand_cap, int vcap_log2 /* 0 = SAFE */)
{
    return gw_lds_bytes(beamK, cand_cap, vcap_log2) + sizeof(float) * NG_TILE_FLOATS + sizeof(int32_t) * NG_GROUP;
}

// k_nvq_gsearch.hip (libjvector_hip_ng.so).  vsf: VSF_L2 / VSF_DOT / VSF_COS.  Returns JV_OK, JV_ERR_INVALID (bad parameters),
// JV_ERR_UNSUPPORTED (LDS) or JV_ERR_HIP.
int launch_nvq_graph_search(ihipStream_t *s, const NgParams &p, size_t p_bytes, int vsf, int workers, bool safe);

}  // namespace jv
