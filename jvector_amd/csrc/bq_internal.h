// bq_internal.h — binary quantization internals shared by bq.cpp and k_bq.hip (not part of the ABI)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/jvector_bq.h"
#include "bg_params.h"
#include "bd_params.h"
#include "bx_params.h"
#include "bc_params.h"

struct jv_bq_vectors {
    int device = 0;
    int D = 0, W = 0;           // W = ceil(D / 64) words per row
    int64_t count = 0;
    uint64_t *d_rows = nullptr; // count x W, row-major
};

namespace jv {

constexpr int kBqMaxDim = 16383;   // the scan's per-block histogram (D + 1 counters per query of the tile) fits 64 KB at a tile of one

// arguments of the flat scan's kernels (k_bq.hip); per-query arrays are Q long, per-(query, row block) arrays Q x X
struct BqScanArgs {
    int64_t N = 0;
    int D = 0, W = 0;
    int Q = 0, tiles = 0;
    int64_t X = 0, R = 0;                 // row blocks and rows per block: block xb owns rows [xb R, min(N, (xb + 1) R))
    const uint64_t *accept = nullptr;     // jv_hip_graph_search_filtered's bit layout (nullable)
    int64_t accept_stride = 0;
    uint32_t *hist = nullptr;             // Q x (D + 1) distance counts of the accepted rows
    int32_t *thr = nullptr;               // threshold distance t_q
    int32_t *need = nullptr;              // rows with h == t_q still needed after every row with h < t_q
    int32_t *all_ties = nullptr;          // 1: every tie fits the list (top-k keeps the smallest ids); 0: ties go in by rank
    uint32_t *tiec = nullptr;             // Q x X ties per row block (queries with all_ties == 0)
    uint32_t *tie_prefix = nullptr;       // Q x X exclusive prefix of tiec
    int32_t *cand_ids = nullptr;          // Q x cap
    float *cand_sc = nullptr;             // Q x cap BQ similarities
    unsigned int *cand_cnt = nullptr;     // Q
    int cap = 0;
};

int launch_bq_encode(hipStream_t s, const float *d_src, int64_t count, int D, int W, int tq, uint64_t *d_out);
int launch_bq_gather(hipStream_t s, const uint64_t *d_rows, int64_t N, int W, int D, const uint64_t *d_qwords, const int32_t *d_node1,
                     int P, const int32_t *d_ord, int B, float *d_out);
// one pass of the scan (mode 0 histogram, 1 emit, 2 ranked ties); qt in {1, 8, 16, 32}
int launch_bq_scan(hipStream_t s, const uint64_t *d_rows, const uint64_t *d_qw, const BqScanArgs &a, int qt, int mode);
// the whole selection: histogram pass, thresholds, emit pass, tie prefixes, ranked-tie pass (a no-op unless a query's ties overflowed)
int launch_bq_select(hipStream_t s, const uint64_t *d_rows, const uint64_t *d_qw, const BqScanArgs &a, int qt, int k1);

// graph traversal over BQ rows (k_bq_gsearch.hip; parameters and body in bg_body.h).  safe: the form whose structures hold every node
int bq_graph_compiled_width(int W);   // W when rows of W words have a build of their own, else 0 (the generic form: query words in LDS)
size_t bq_graph_lds_bytes(int rerankK, int cand_cap, int W, int vcap_log2 /* 0 = the safe form */);
int launch_bq_graph_search(hipStream_t s, const BgParams &p, int workers, bool safe);

// jv_hip_bq_graph_search in two halves around the step that produces the query words (bq_graph.cpp): an encode of float queries there,
// a gather of stored rows in bq_build.cpp.  bq_graph_begin runs every check and fills p's graph view; bq_graph_finish is the
// traversal, the pass that runs overflowed queries again, the rerank (vectors != NULL), the top-K, the outputs and the counters.
struct BqGraphCall {
    const char *who;            // the entry point's name in error messages
    const jv_graph *g;
    const jv_bq_vectors *bq;
    const jv_vectors *vectors;  // nullable
    int Q;
    jv_vsf vsf;
    int topK, rerankK;
    const uint64_t *accept_bits;
    int64_t accept_stride_words;
    int32_t *out_ids;
    float *out_scores;
    int64_t *stats;
    bool empty;                 // (begin) Q == 0: nothing to do
    BgParams p;                 // (begin) levels, entry node and level, n_nodes
};
int bq_graph_begin(jv_ctx *ctx, BqGraphCall &c, const void *input);
int bq_graph_finish(jv_ctx *ctx, const BqGraphCall &c, const float *d_q, const uint64_t *d_qw, const int32_t *d_exclude,
                    const int32_t *d_blank_nodes);
// rows of ids / scores (Q x K) and counters (Q x 2) of the items whose ordinal lies outside [0, n_rows) become -1 / -INFINITY / 0 (bq_build.cpp)
// out row q = row nodes[q] of d_rows (zero words for an ordinal outside [0, n_rows)): the query words of a node-seeded search, and the
// compacted rows of an upper level in bq_builder.cpp
int launch_bq_gather_rows(hipStream_t s, const uint64_t *d_rows, int64_t n_rows, int W, const int32_t *d_nodes, int64_t Q, uint64_t *d_out);
int launch_bq_blank_rows(hipStream_t s, const int32_t *d_nodes, int64_t n_rows, int Q, int K, int32_t *d_ids, float *d_scores, long long *d_stats);

// batched robust prune over BQ rows (k_bq_retain.hip; parameters in bd_params.h, body in bd_body.h)
int bq_retain_compiled_width(int W);
size_t bq_retain_lds_bytes(int C, int W);
int launch_bq_retain(hipStream_t s, const jv_ctx *ctx, const BdParams &p);

// the entry point of a graph built from BQ rows (k_bq_builder.hip; body in bm_body.h): the majority row of the n members (ordinals
// d_members, nullptr = rows 0..n-1) and the member nearest to it; *d_best points at the key (hamming << 32 | id) inside d_work
int bq_entry_waves(int n);
size_t bq_entry_work_bytes(int W, int n);
int launch_bq_entry(hipStream_t s, const uint64_t *d_rows, int64_t n_rows, int W, const int32_t *d_members, int n, void *d_work, long long **d_best);

// deleting nodes from a graph built over BQ rows (k_bq_delete.hip; parameters in bx_params.h, bodies in bx_body.h).  The bitmaps hold
// ceil(n / 64) words; _affected fills p.affected / p.tasks (ascending) / p.task_count; _merge runs the P tasks (p.list == nullptr:
// lengths and candidate counts only); _retire blanks the marked nodes' rows, clears their present bits and then every mark
int bq_delete_compiled_width(int W);
int launch_bq_delete_set_bits(hipStream_t s, const int32_t *d_ids, int B, int64_t n, uint64_t *d_bits);
int launch_bq_delete_live_bits(hipStream_t s, const uint64_t *d_present, const uint64_t *d_marked, int64_t n, uint64_t *d_out);
int launch_bq_delete_affected(hipStream_t s, const BxParams &p);
int launch_bq_delete_merge(hipStream_t s, const jv_ctx *ctx, const BxParams &p);
int launch_bq_delete_retire(hipStream_t s, uint64_t *d_present, uint64_t *d_marked, int64_t n, int R, int32_t *d_nbrs, float *d_nsc, int32_t *d_db);

// compacting a graph built over BQ rows (k_bq_compact.hip; parameters in bc_params.h, bodies in bc_body.h).  _rank fills p.block_base,
// p.counters, p.old_to_new and (nullable) p.new_to_old from the present bits; _rows and _bq_rows gather rows [0, p.live) of the
// destination under the two maps, _rows counting the stored ids without an image in p.counters; _fill_bits sets bits [0, live) of n.
// They live in a library of their own, libjvector_hip_bqc.so, and return a status without an error text: the caller sets it
#define JV_BQC_API __attribute__((visibility("default")))
// (p_bytes: the caller's sizeof(BcParams); a library built from another bc_params.h answers JV_ERR_INVALID instead of reading a skewed struct)
JV_BQC_API int launch_bq_compact_rank(hipStream_t s, const BcParams &p, size_t p_bytes = sizeof(BcParams));
JV_BQC_API int launch_bq_compact_rows(hipStream_t s, const BcParams &p, size_t p_bytes = sizeof(BcParams));
JV_BQC_API int launch_bq_compact_bq_rows(hipStream_t s, const BcParams &p, size_t p_bytes = sizeof(BcParams));
JV_BQC_API int launch_bq_compact_fill_bits(hipStream_t s, uint64_t *d_bits, int64_t n, int64_t live);

}  // namespace jv
