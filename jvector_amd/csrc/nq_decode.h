// nq_decode.h — the de-quantisation of one NVQ byte (scaledLogitFunctionNQT of the reference), shared by the kernels that score
// NVQ rows: the gather form (k_nvq.hip) and the flat search's tile form (k_nvq_flat.hip).  Device code only; the line numbers are
// those of B/vector/DefaultVectorUtilSupport.java, as in k_nvq.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace jv {

__device__ __forceinline__ int nq_bits(float x) { return (x != x) ? 0x7fc00000 : __float_as_int(x); }   // Float.floatToIntBits
// logitNQT :450-459
__device__ __forceinline__ float nq_logit(float value, float inverseAlpha, float x0)
{
    const float z = value / (1.0f - value);
    const int temp = nq_bits(z);
    const int e = temp & 0x7f800000;
    const float p = (float)((e >> 23) - 128);
    const float m = __int_as_float((temp & 0x007fffff) + 0x3f800000);
    return __builtin_fmaf(m + p, inverseAlpha, x0);
}
// scaledLogitFunctionNQT :466-469
__device__ __forceinline__ float nq_scaled_logit(float v, float inv, float smid, float scale, float bias)
{
    return nq_logit(__builtin_fmaf(v, scale, bias), inv, smid);
}

// a / b for operands well inside the normal range: the fma sequence the compiler's IEEE division is made of (reciprocal
// estimate, one Newton step on it, quotient with two residual corrections — correctly rounded) without the v_div_scale /
// v_div_fmas / v_div_fixup wrapping that only matters at the ends of the exponent range.  Plain fma chains also let the
// compiler pair two dimensions per v_pk_fma_f32.
__device__ __forceinline__ float nq_div_fast(float a, float b)
{
    float r = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    float q = a * r;
    float t = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(t, r, q);
    t = __builtin_fmaf(-b, q, a);
    return __builtin_fmaf(t, r, q);
}
// is every byte of a sub-vector with these derived numbers safe for nq_div_fast?  sv = fma(byte, scale, bias) is monotone in
// the byte, so both ends inside [2^-40, 1 - 2^-20] put every sv there, 1 - sv inside [2^-20, 1) and the quotient inside
// [2^-41, 2^20]: finite, normal, never NaN.  (Comparisons are false for NaN parameters -> the IEEE path.)
__device__ __forceinline__ bool nq_fast_ok(const float4 prm)
{
    const float s0 = prm.w, s1 = __builtin_fmaf(255.0f, prm.z, prm.w);
    const float lo = s0 < s1 ? s0 : s1, hi = s0 < s1 ? s1 : s0;
    return lo >= 9.094947017729282e-13f && hi <= 0.99999905f;
}

}  // namespace jv
