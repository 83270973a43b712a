// bg_params.h — launch parameters of the graph traversal over binary-quantized vectors (bg_body.h / k_bq_gsearch.hip), shared with
// the host front end in bq_graph.cpp.  Plain data only.
#pragma once

#include "gw_params.h"

namespace jv {

struct BgParams : GwParams {   // out_scores: the kept results' BQ similarities
    const uint64_t *rows;      // [n][W] BQ rows
    int32_t D, W;
    const uint64_t *qwords;    // [Q][W] encoded queries
};

// LDS bytes of one worker: [results][candidate tier][64 samples][query words (generic width only)][visited table (if it fits)]
constexpr size_t bg_lds_bytes(int rerankK, int cand_cap, int lds_query_words, int vcap_log2 /* 0 = SAFE */)
{
    return gw_lds_bytes(rerankK, cand_cap, vcap_log2) + sizeof(long long) * (size_t)lds_query_words;
}

}  // namespace jv
