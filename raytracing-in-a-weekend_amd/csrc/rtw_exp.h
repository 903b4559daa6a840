// rtw_exp.h -- exp_plain, the f32 exponential of the guided filter (rtw_filter.hip): one __host__ __device__ definition
// for the kernel, for the host path and for the host entry point rtw_exp_plain (rtw_shim.hip) that the CPU tests call.  In the style of
// pow_plain (rtw_mixed.h): explicit fmaf, no ocml, no v_exp_f32, no second path behind a range check, the special cases are selects.
//
// Domain x <= 0 (-0, -inf and NaN included):  q = x log2(e) as q_hi + q_lo (the product's remainder through fmaf, log2(e) in two parts);
// n = rint(q_hi), r = (q_hi - n) + q_lo, |r| <= 1/2 (+ a rounding);  2^r = 1 + r E(r), pow_plain's tail with its coefficients;  the result
// is 2^r 2^n.  The scale is applied as 2^(n + 64) first -- a normal number for every n that can matter -- and a result that would be below
// 2^-126 is returned as +0, so no subnormal is ever formed and host and device cannot disagree on one.
//   exp_plain(+-0) = 1 exactly (q = 0, r = 0, E irrelevant);  exp_plain(-inf) = 0;  NaN gives NaN;  x > 0 is outside the domain: NaN.
// Maximum error against f64 exp over EVERY f32 in [-104, 0] (scripts/sweep_exp_plain.py): DESIGN.md 8b.
#pragma once
#include "rtw_mixed.h"

namespace rtw {

__host__ __device__ __forceinline__ float exp_plain(float x) {
    // computed on x clamped to [-88, 0]: e^-88 < 2^-126 is +0 either way, and a NaN or an x > 0 (-88 / 0 here) is selected away below,
    // so n stays in [-127, 0] and its conversion to an integer is defined for every input
    const float xc = x >= -88.0f ? (x <= 0.0f ? x : 0.0f) : -88.0f;
    const float L2E_HI = 1.4426950216293335f, L2E_LO = 1.925963033500011e-08f;
    const float q_hi = xc * L2E_HI;
    float q_lo = __builtin_fmaf(xc, L2E_HI, -q_hi);                        // exact remainder of the rounded product
    q_lo = __builtin_fmaf(xc, L2E_LO, q_lo);
    const float n = __builtin_rintf(q_hi);                                 // in [-127, 0]
    const float r = (q_hi - n) + q_lo;                                     // (q_hi - n is exact)
    float E = 1.529732435301412e-05f;
    E = __builtin_fmaf(E, r, 0.00015461444854736328f); E = __builtin_fmaf(E, r, 0.0013333501992747188f); E = __builtin_fmaf(E, r, 0.009618056938052177f);
    E = __builtin_fmaf(E, r, 0.05550410971045494f);    E = __builtin_fmaf(E, r, 0.24022650718688965f);   E = __builtin_fmaf(E, r, 0.6931471824645996f);
    const float v = __builtin_fmaf(r, E, 1.0f);
    const float scaled = v * mx_bits_to_float((uint32_t)((int32_t)n + 64 + 127) << 23);   // v 2^(n + 64): exact, normal
    float res = scaled < 0x1p-62f ? 0.0f : scaled * 0x1p-64f;              // below 2^-126: +0; else exact
    res = x < -88.0f ? 0.0f : res;
    return (x != x || x > 0.0f) ? __builtin_nanf("") : res;
}

} // namespace rtw
