/*
 * jvector_bq_compact.h — compacting a graph under construction over binary-quantized vectors: after deletions a jv_bq_builder still
 * spans every row it ever had; this is the step that renumbers the nodes in the graph 0, 1, 2 ... and packs their rows, on the device,
 * into a builder that takes inserts again.  It is also how a builder grows.  Includes jvector_bq_builder.h; conventions are
 * jvector_hip.h's.
 *
 * Reference (B/ = jvector-base/src/main/java/io/github/jbellis/jvector/): AbstractGraphIndexWriter.sequentialRenumbering
 * (B/graph/disk/AbstractGraphIndexWriter.java:146-159) gives the surviving nodes the ordinals 0, 1, 2 ... in their old relative order;
 * OrdinalMapper.MapMapper and RemappedRandomAccessVectorValues carry rows and neighbour ids across.  The renumbering is monotone
 * (i < j => map[i] < map[j]) and every order this engine defines breaks ties to the smaller id, so the compacted builder is the same
 * graph under another naming: searches, inserts and improves on it give, id for mapped id and bit for bit, what they give on the source.
 */
#ifndef JVECTOR_BQ_COMPACT_H
#define JVECTOR_BQ_COMPACT_H

#include "jvector_bq_builder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What compact returns when the source builder contradicts its own invariants (rule 12); jv_hip_last_error() says where. */
#define JV_ERR_INTERNAL (-6)

/* sequentialRenumbering of the builder's graph.  *live_out = nodes in the graph.
 * old_to_new: n int32 (n = rows of the builder), -1 for a row not in the graph (never inserted, or removed).
 * new_to_old: at least *live_out int32 — the caller sizes it from counts5[2] of jv_hip_bq_builder_stats.
 * Each output nullable, host or device memory.  The builder is not changed. */
JV_API int jv_hip_bq_builder_renumbering(jv_ctx *ctx, const jv_bq_builder *b, int32_t *old_to_new, int32_t *new_to_old,
                                         int64_t *live_out);

/* A NEW builder over dst_bq holding src's graph under the sequential renumbering; src is not changed.  old_to_new / new_to_old /
 * live_out as above.  The rules (live = nodes in src's graph, n = rows of src):
 *   1. capacity = jv_hip_bq_count(dst_bq).  dst_bq has src's dimension, is not src's own jv_bq_vectors, and capacity >= max(live, 1).
 *   2. Rows [0, live) of dst_bq receive the BQ rows of the live nodes, new row r from old row new_to_old[r], words unchanged.
 *   3. Rows [live, capacity) of dst_bq are not written: the caller may have encoded the rows of future nodes there already.
 *   4. The new builder has src's maxDegree, beamWidth, alpha, neighborOverflow and row width R.  The caller keeps dst_bq alive for it.
 *   5. New row r holds old row new_to_old[r]: every id goes through old_to_new, -1 stays -1; order, score bits and the diverseBefore
 *      mark are unchanged.  Nothing is re-scored, re-sorted or pruned.
 *   6. Rows [live, capacity) of the new builder are blank — ids -1, scores 0, diverseBefore 0: "never inserted" rows, so
 *      insert_batch takes them.
 *   7. entry of the new builder is old_to_new[entry], or -1 if src is empty; then seed works as on a fresh builder.
 *   8. The new builder's deleted_count is (0, 0), no id of it counts as removed, stats gives seconds3 = 0 and
 *      counts5 = {0, 0, live, 0, 0}, live_bits has bits [0, live) set.
 *   9. JV_ERR_INVALID while marks are pending on src (a node marked and not yet removed): call remove_deleted first.
 *  10. JV_ERR_INVALID as well: a NULL handle or a NULL out; a dimension mismatch; dst_bq equal to src's vectors; a capacity below
 *      max(live, 1); handles on another device than the context's.
 *  11. A refused call (JV_ERR_INVALID, JV_ERR_UNSUPPORTED, JV_ERR_INTERNAL) leaves src and dst_bq as they were and creates nothing.  A
 *      HIP runtime failure (JV_ERR_HIP, JV_ERR_OOM) creates nothing either but may leave rows [0, live) of dst_bq partly written.
 *  12. A stored id with no image — it names a row that is not in the graph, which the builder's invariants exclude — is never written
 *      silently: the remap kernel counts such ids, and if there is one the call fails with JV_ERR_INTERNAL, the message names the
 *      first new row holding one, no builder is returned and dst_bq has not been written.
 *  13. The result is a function of src and the capacity only: no atomic decides a position, two runs are byte-identical.
 *  14. With nothing removed and capacity > n this is how a builder grows: identity map, more rows.
 * Not covered: merging several builders, compacting a finished jv_layered, the caller's float rows (new_to_old is what they need). */
JV_API int jv_hip_bq_builder_compact(jv_ctx *ctx, const jv_bq_builder *src, jv_bq_vectors *dst_bq, int32_t *old_to_new,
                                     int32_t *new_to_old, int64_t *live_out, jv_bq_builder **out);

#ifdef __cplusplus
}
#endif

#endif /* JVECTOR_BQ_COMPACT_H */
