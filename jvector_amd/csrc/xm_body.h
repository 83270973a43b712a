// xm_body.h — what a layered build over float rows needs on the device beside the search and the prune: the compacted copy of an upper
// level's rows, and the entry point.  The bodies of k_exact_builder.hip's kernels.
//
// Row gather (xm_gather_rows).  out[i] = rows[ids[i]].  A group of LPR lanes owns a row: 16, 32 or 64 lanes by the row's length in
// 16-byte pieces (D / 4 <= 16, <= 32, more), so a short row does not leave three quarters of a wavefront without a piece, and a
// workgroup of 256 threads moves 16, 8 or 4 rows per pass.  Rows whose length is a multiple of four floats are 16-byte aligned on both
// sides and travel as float4; any other D leaves neither side aligned from the second row on, and the row travels as dwords, the
// group sized by D itself.  Up to four pieces of a row are loaded before the first is stored.
//
// Entry point (xm_mean, xm_nearest, xm_pick).  The entry is a function of (rows, vsf) only:
//   mean     c[d] = (sum over the members in ascending id of v[id][d], added sequentially in f32 from 0) * (1.0f / count) — addInPlace,
//            then scale.  A lane owns a dimension and walks the members: every wave reads 64 consecutive floats of one row per
//            load, the ids come through scalar loads, and the loads of the next eight members are in flight while the eight before
//            them are added (the adds are the only dependent chain).  ceil(D / 64) wavefronts, count dependent adds each.
//   nearest  every member scored against c with the chains of xc_chain.h — the bits of jv_hip_exact_scores(query = c) — one lane per
//            member through xg_body.h's LDS row tile (xg_tr_rows, 64 rows x 64 floats per chunk), c wave-uniform through scalar loads
//            like a query of exact_graph_search_kernel; rows that are not 16-byte aligned or D % 8 != 0: a lane walks its own row
//            (exact_row / cosine_row).  c's own sum of squares (cosine) is the sequential sum query_sqnorm_kernel forms, computed by
//            every wave for itself.  A lane keeps the best NodeQueue key (sortableInt(score) << 32 | ~id, signed: higher score
//            first, ties to the smaller id) of the members it scored; a DPP reduction gives the wave's, stored per workgroup.
//   pick     one wavefront over the per-wave winners.  No atomic anywhere: the result does not depend on the launch shape.
#pragma once

#include <cstdint>

#include "xm_params.h"
#include "xg_body.h"

namespace jv {

typedef const __attribute__((address_space(4))) int32_t xm_cint;   // wave-uniform, never written while the kernel runs: s_load

template <int LPR, bool AL>
GS_FN void xm_gather_rows(const XmGatherParams &p, int tid, int block, int blocks)
{
    constexpr int RPB = 256 / LPR;   // rows per workgroup and pass
    const int sub = tid % LPR;
    const int D = p.D;
    for (int64_t i = (int64_t)block * RPB + tid / LPR; i < p.count; i += (int64_t)blocks * RPB) {
        const int32_t id = p.ids[i];
        const bool ok = id >= 0 && id < p.n;
        const float *__restrict__ src = p.rows + (int64_t)(ok ? id : 0) * D;
        float *__restrict__ dst = p.out + i * D;
        if (AL) {
            const int nv = D >> 2;
            for (int v = sub; v < nv; v += 4 * LPR) {
                float4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (v + u * LPR < nv) x[u] = ok ? *reinterpret_cast<const float4 *>(src + 4 * (v + u * LPR)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (v + u * LPR < nv) *reinterpret_cast<float4 *>(dst + 4 * (v + u * LPR)) = x[u];
            }
        } else {
            for (int d = sub; d < D; d += 4 * LPR) {
                float x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (d + u * LPR < D) x[u] = ok ? src[d + u * LPR] : 0.0f;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (d + u * LPR < D) dst[d + u * LPR] = x[u];
            }
        }
    }
}

// dimension d of the mean row (a lane past D reads column 0 and writes nothing)
GS_FN void xm_mean(const XmEntryParams &p, int d)
{
    constexpr int U = 8;
    xm_cint *ids = (xm_cint *)p.ids;
    const int D = p.D, cnt = p.count;
    const bool in = d < D;
    const float *col = p.rows + (in ? d : 0);
    // (the host has looked at every id; the clamp keeps a read inside the rows whatever the parameter block holds)
    auto load = [&](int m) {
        const int32_t id = ids[m];
        return col[(int64_t)((id >= 0 && id < p.n) ? id : 0) * D];
    };
    float acc = 0.0f;
    float cur[U], nxt[U];
    int m = 0;
    if (cnt >= U) {
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = load(u);
        for (; m + U <= cnt; m += U) {
            const bool more = m + 2 * U <= cnt;   // (wave-uniform)
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = load(m + U + u);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) acc += cur[u];
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) cur[u] = nxt[u];
            }
        }
    }
    for (; m < cnt; ++m) acc += load(m);
    if (in) p.mean[d] = acc * (1.0f / (float)cnt);
}

// VectorSimilarityFunction.compare(c, row my_node) for the cnt rows of a group, lane j < cnt holding the j-th (others -1)
template <int VSF, bool TR>
GS_FN float xm_score_group(const XmEntryParams &p, float cnorm, int32_t my_node, int cnt, float *tile)
{
    const int D = p.D;
    float raw = 0.0f;
    if (TR) {
        raw = xg_tr_rows<VSF, 64, 64>(p.rows, D, my_node, cnt, (xg_cfloat *)p.mean, tile);
        if (VSF == VSF_COS && my_node >= 0) raw = cosine_finish(raw, cnorm, p.vnorm[my_node]);
    } else if (my_node >= 0) {
        const float *b = p.rows + (int64_t)my_node * D;
        if (VSF == VSF_COS) {
            float sum, norm2;
            cosine_row(p.mean, b, D, sum, norm2);
            raw = cosine_finish(sum, cnorm, norm2);
        } else {
            raw = exact_row<VSF>(p.mean, b, D);
        }
    }
    return score_from_raw(VSF, raw);
}

// one wavefront: groups wave, wave + waves, ... of 64 members; its best key to wave_best[wave]
template <int VSF, bool TR>
GS_FN void xm_nearest(const XmEntryParams &p, int wave, float *tile)
{
    const int lane = gs_lane();
    float cnorm = 0.0f;
    if (VSF == VSF_COS) {   // norm1 of DefaultVectorUtilSupport.cosine: the sequential sum of e * e
        xg_cfloat *c = (xg_cfloat *)p.mean;
        for (int j = 0; j < p.D; ++j) cnorm += c[j] * c[j];
    }
    long long best = GS_KEY_MIN;
    const int groups = (p.count + 63) >> 6;
    for (int g = wave; g < groups; g += p.waves) {
        const int m = g * 64 + lane;
        const int cnt = p.count - g * 64 < 64 ? p.count - g * 64 : 64;
        int32_t mine = m < p.count ? p.ids[m] : -1;
        if (mine >= p.n) mine = -1;   // (the host has looked at every id)
        const float sc = xm_score_group<VSF, TR>(p, cnorm, mine, cnt, tile);
        const long long key = mine >= 0 ? gs_key(mine, sc) : GS_KEY_MIN;
        best = key > best ? key : best;
    }
    best = gs_wave_max(best);
    if (lane == 0) p.wave_best[wave] = best;
}

// one wavefront over the per-wave winners
GS_FN void xm_pick(const XmEntryParams &p)
{
    const int lane = gs_lane();
    long long best = GS_KEY_MIN;
    for (int w = lane; w < p.waves; w += 64) {
        const long long k = p.wave_best[w];
        best = k > best ? k : best;
    }
    best = gs_wave_max(best);
    if (lane == 0) *p.best = best;
}

}  // namespace jv
