// xc_chain.h — the exact score chains in the reference's association order (DefaultVectorUtilSupport.java:38-105 dot, :158-193 L2,
// :121-139 cosine), non-fused multiply and add: the helpers k_exact.hip's kernels run, lifted here unchanged so that the exact-score
// graph traversal (xg_body.h) scores a row with the same bits as jv_hip_exact_scores.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "jv_device.h"

namespace jv {

// --- per-8-block updates in the reference's association order -----------------------------------
__device__ __forceinline__ float dot8(const float *__restrict__ a, const float4 v0, const float4 v1)
{
    // b[i+0]*a[i+0] + b[i+1]*a[i+1] + ... left to right   (a = query, b = candidate; product commutes)
    float t = v0.x * a[0] + v0.y * a[1];
    t = t + v0.z * a[2];
    t = t + v0.w * a[3];
    t = t + v1.x * a[4];
    t = t + v1.y * a[5];
    t = t + v1.z * a[6];
    t = t + v1.w * a[7];
    return t;
}

__device__ __forceinline__ float l28(const float *__restrict__ a, const float4 v0, const float4 v1)
{
    const float d0 = a[0] - v0.x, d1 = a[1] - v0.y, d2 = a[2] - v0.z, d3 = a[3] - v0.w;
    const float d4 = a[4] - v1.x, d5 = a[5] - v1.y, d6 = a[6] - v1.z, d7 = a[7] - v1.w;
    float t = d0 * d0 + d1 * d1;
    t = t + d2 * d2;
    t = t + d3 * d3;
    t = t + d4 * d4;
    t = t + d5 * d5;
    t = t + d6 * d6;
    t = t + d7 * d7;
    return t;
}

// Scores one candidate row against one query held in (LDS) memory `a`.  Generic in D.
template <int VSF>
__device__ __forceinline__ float exact_row(const float *__restrict__ a, const float *__restrict__ b, int D)
{
    if (VSF == VSF_DOT) {
        float res = 0.0f;
        int i = 0;
        const int rem = D % 8;
        for (; i < rem; ++i) res += b[i] * a[i];
        if (D < 8) return res;
        if (rem == 0 && ((reinterpret_cast<uintptr_t>(b) & 15) == 0)) {
            for (; i + 7 < D; i += 8) {
                const float4 v0 = *reinterpret_cast<const float4 *>(b + i);
                const float4 v1 = *reinterpret_cast<const float4 *>(b + i + 4);
                res += dot8(a + i, v0, v1);
            }
        } else {
            for (; i + 7 < D; i += 8) {
                const float4 v0 = make_float4(b[i], b[i + 1], b[i + 2], b[i + 3]);
                const float4 v1 = make_float4(b[i + 4], b[i + 5], b[i + 6], b[i + 7]);
                res += dot8(a + i, v0, v1);
            }
        }
        return res;
    } else if (VSF == VSF_L2) {
        float sq = 0.0f;
        int i = 0;
        if ((reinterpret_cast<uintptr_t>(b) & 15) == 0) {
            for (; i + 8 <= D; i += 8) {
                const float4 v0 = *reinterpret_cast<const float4 *>(b + i);
                const float4 v1 = *reinterpret_cast<const float4 *>(b + i + 4);
                sq += l28(a + i, v0, v1);
            }
        } else {
            for (; i + 8 <= D; i += 8) {
                const float4 v0 = make_float4(b[i], b[i + 1], b[i + 2], b[i + 3]);
                const float4 v1 = make_float4(b[i + 4], b[i + 5], b[i + 6], b[i + 7]);
                sq += l28(a + i, v0, v1);
            }
        }
        for (; i < D; ++i) {
            const float d = a[i] - b[i];
            sq += d * d;
        }
        return sq;
    } else {
        // cosine: three sequential accumulators; norm1 (query side) is candidate independent and is
        // passed in pre-accumulated by the caller, here we return sum and norm2 packed by reference.
        return 0.0f;
    }
}

__device__ __forceinline__ void cosine_row(const float *__restrict__ a, const float *__restrict__ b, int D,
                                           float &sum, float &norm2)
{
    float s = 0.0f, n2 = 0.0f;
    int i = 0;
    if ((reinterpret_cast<uintptr_t>(b) & 15) == 0) {
        for (; i + 4 <= D; i += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(b + i);
            s += a[i] * v.x;
            n2 += v.x * v.x;
            s += a[i + 1] * v.y;
            n2 += v.y * v.y;
            s += a[i + 2] * v.z;
            n2 += v.z * v.z;
            s += a[i + 3] * v.w;
            n2 += v.w * v.w;
        }
    }
    for (; i < D; ++i) {
        const float e2 = b[i];
        s += a[i] * e2;
        n2 += e2 * e2;
    }
    sum = s;
    norm2 = n2;
}

}  // namespace jv
