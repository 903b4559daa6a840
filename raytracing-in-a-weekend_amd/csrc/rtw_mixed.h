// rtw_mixed.h -- Rust2's MixedMaterial, the Phong-lobe surface (Rust2/src/objects/material.rs:235-297, onb.rs:30-44), and the three
// elementary functions it calls.  Everything here is __host__ __device__: one definition for the mixed build of the render kernels
// (SPEC 10) and for the host entry points rtw_mixed_dir / rtw_mixed_pdf / rtw_pow_plain / rtw_sin_plain / rtw_cos_plain (rtw_shim.hip)
// that the CPU tests call.  f32, one rounding per written operation, no contraction (-ffp-contract=off) except where an fmaf is written
// out, the reference's operation order.
//
// Rust's f32::powf / sin / cos are the platform libm's, good to about an ulp; which ulp decides nothing here but the last bits of a
// direction or of a pdf.  The three below are classic reductions with polynomials fitted for this file (Chebyshev interpolants of the
// remainders), written with explicit fmaf so that host and device give the same bits.  No ocml, no v_log_f32 / v_exp_f32, no second path
// behind a range check: they are total on their domains, the special cases are selects at the end (atan2_plain / acos_plain, rtw_device.h,
// are the precedent).  Maximum error against f64, every intermediate rounded to f32 (tests/test_mixed_cpu.py re-measures all of it):
//   pow_plain   bases 1 - xi for all 2^24 stream values xi at gen_exp 1/2, 1/4, 1/11:  0.90 / 0.89 / 0.89 ulp
//               cosines in [0, 1] (2^22 + 1 evenly spaced and 2^20 random ones) at exp 1, 3, 10:  0 (exact) / 0.92 / 1.05 ulp
//   sin_plain   phi = (xi * 2) * PI for all 2^24 stream values:  1.44 ulp
//   cos_plain   the same:  1.43 ulp
// (the precedent: atan2_plain 2.03 ulp, acos_plain 1.25 ulp)
#pragma once
#include "rtw_light.h"

namespace rtw {

__host__ __device__ __forceinline__ float mx_bits_to_float(uint32_t b) { union { uint32_t u; float f; } c; c.u = b; return c.f; }
__host__ __device__ __forceinline__ uint32_t mx_float_to_bits(float f) { union { uint32_t u; float f; } c; c.f = f; return c.u; }

// pow(x, y) for x >= 0 (0, 1, inf and NaN included) and finite y >= 0:  2^(y log2 x), the logarithm and the product kept as hi + lo pairs.
//   x = 2^e m, m in [sqrt(1/2), sqrt(2));  s = (m - 1) / (m + 1) as s_hi + s_lo (the quotient's remainder through fmaf);
//   ln m = 2 s + s^3 Q(s^2);  log2 x = e + ln m * log2(e);  q = y log2 x;  n = rint(q), r = q - n;  2^r = 1 + r E(r);  result = 2^r 2^n,
//   the scale applied in two factors so that a subnormal result is rounded once.
// Specials as libm's: pow(x, 0) = 1 for every x, a NaN included; pow(0, y > 0) = 0; pow(inf, y > 0) = inf; pow(1, y) = 1 exactly
// (log2 1 = 0 exactly); a NaN x gives NaN.  x < 0 is outside the domain (a negative cosine returns before the call) and gives NaN.
__host__ __device__ __forceinline__ float pow_plain(float x, float y) {
    const bool tiny = x < 0x1p-126f;                                       // a subnormal base: rescaled (exact)
    const float xs = tiny ? x * 0x1p24f : x;
    const uint32_t b = mx_float_to_bits(xs);
    float e = (float)((int32_t)((b >> 23) & 0xFFu) - 127) - (tiny ? 24.0f : 0.0f);
    const uint32_t man = b & 0x7FFFFFu;
    const bool upper = man >= 0x3504F3u;                                   // m >= sqrt(2): halve it
    const float m = mx_bits_to_float(man | (upper ? 0x3F000000u : 0x3F800000u));
    e = upper ? e + 1.0f : e;
    const float f = m - 1.0f;                                              // exact
    const float dh = m + 1.0f, dl = m - (dh - 1.0f);                       // m + 1 = dh + dl exactly
    const float s_hi = f / dh;
    float rem = __builtin_fmaf(-s_hi, dh, f);                              // exact remainder of the rounded quotient
    rem = __builtin_fmaf(-s_hi, dl, rem);
    const float s_lo = rem / dh;
    const float z = s_hi * s_hi;
    float Q = 0.23330962657928467f;
    Q = __builtin_fmaf(Q, z, 0.28550803661346436f); Q = __builtin_fmaf(Q, z, 0.4000012278556824f); Q = __builtin_fmaf(Q, z, 0.6666666865348816f);
    const float t_hi = s_hi + s_hi;                                        // ln m = t_hi + c
    const float c = __builtin_fmaf(s_hi * z, Q, s_lo + s_lo);
    const float L2E_HI = 1.4426950216293335f, L2E_LO = 1.925963033500011e-08f;
    const float p_hi = t_hi * L2E_HI;
    float p_lo = __builtin_fmaf(t_hi, L2E_HI, -p_hi);
    p_lo = __builtin_fmaf(t_hi, L2E_LO, p_lo);
    p_lo = __builtin_fmaf(c, L2E_HI, p_lo);
    const float a_hi = e + p_hi;                                           // log2 x = a_hi + a_lo (|e| >= |p_hi| or e == 0: the error term is exact)
    const float a_lo = (p_hi - (a_hi - e)) + p_lo;
    const float q_hi = y * a_hi;
    const float q_lo = __builtin_fmaf(y, a_lo, __builtin_fmaf(y, a_hi, -q_hi));
    const float n = __builtin_rintf(fminf(fmaxf(q_hi, -252.0f), 254.0f));  // beyond: 0 or inf either way
    const float r = fminf(fmaxf((q_hi - n) + q_lo, -1.0f), 1.0f);
    float E = 1.529732435301412e-05f;
    E = __builtin_fmaf(E, r, 0.00015461444854736328f); E = __builtin_fmaf(E, r, 0.0013333501992747188f); E = __builtin_fmaf(E, r, 0.009618056938052177f);
    E = __builtin_fmaf(E, r, 0.05550410971045494f);    E = __builtin_fmaf(E, r, 0.24022650718688965f);   E = __builtin_fmaf(E, r, 0.6931471824645996f);
    const float v = __builtin_fmaf(r, E, 1.0f);
    const int32_t ni = (int32_t)n, n1 = ni >> 1, n2 = ni - n1;             // both in [-126, 127]
    float res = (v * mx_bits_to_float((uint32_t)(n1 + 127) << 23)) * mx_bits_to_float((uint32_t)(n2 + 127) << 23);
    res = x == 0.0f ? 0.0f : res;
    res = x == __builtin_inff() ? __builtin_inff() : res;
    res = (x != x || x < 0.0f) ? __builtin_nanf("") : res;
    return y == 0.0f ? 1.0f : res;
}

// sin and cos of phi in [0, 2 pi] (NaN for NaN):  k = rint(phi * 2/pi) in 0 .. 4, r = phi - k pi/2 with pi/2 in two parts (fmaf: the products
// are exact), |r| <= pi/4 (+ a rounding);  sin r = r + r s S(s), cos r = 1 - s/2 + s^2 C(s) with s = r^2 (the 1 - s/2 in fdlibm's compensated
// form);  then the quadrant.
__host__ __device__ __forceinline__ void sincos_plain(float phi, float &sn, float &cs) {
    const float k = __builtin_rintf(phi * 0.6366197466850281f);
    float r = __builtin_fmaf(-k, 1.5707963705062866f, phi);
    r = __builtin_fmaf(-k, -4.371138828673793e-08f, r);
    r = __builtin_fmaf(-k, -1.7151245100058819e-15f, r);                  // (the f32 nearest 3 pi/2 leaves r = 1.2e-8 after two parts: a third)
    const float s = r * r;
    float S = 2.7243811473454116e-06f;
    S = __builtin_fmaf(S, s, -0.00019840039021801203f); S = __builtin_fmaf(S, s, 0.008333331905305386f); S = __builtin_fmaf(S, s, -0.1666666716337204f);
    const float sr = __builtin_fmaf(r * s, S, r);
    float Cq = -2.7295945415062306e-07f;
    Cq = __builtin_fmaf(Cq, s, 2.4800561732263304e-05f); Cq = __builtin_fmaf(Cq, s, -0.00138888880610466f); Cq = __builtin_fmaf(Cq, s, 0.0416666679084301f);
    const float h = 0.5f * s, w = 1.0f - h;
    const float cr = w + __builtin_fmaf(s * s, Cq, (1.0f - w) - h);
    const bool swap = k == 1.0f || k == 3.0f;
    const float a = swap ? cr : sr, bq = swap ? sr : cr;
    sn = (k == 2.0f || k == 3.0f) ? -a : a;
    cs = (k == 1.0f || k == 2.0f) ? -bq : bq;
}
__host__ __device__ __forceinline__ float sin_plain(float phi) { float s, c; sincos_plain(phi, s, c); return s; }
__host__ __device__ __forceinline__ float cos_plain(float phi) { float s, c; sincos_plain(phi, s, c); return c; }

__host__ __device__ __forceinline__ lv3 lcross(lv3 a, lv3 b) {           // Vec3::cross (vec3.rs:212-218)
    return lmk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// MixedMaterial::new(exp).on_hit(h)'s direction for the two uniform draws xi_phi, xi_cos (in that order):
// ONB::new_from_w(h.n).from_local(gen_random_dir()).  h.n as the hit reports it: NOT flipped for a back-face hit.
__host__ __device__ __forceinline__ lv3 mixed_dir(float exp, float xi_phi, float xi_cos, lv3 n) {
    const float gen_exp = 1.0f / (exp + 1.0f);
    const lv3 w = lunit(n);
    const lv3 a = __builtin_fabsf(w.x) > 0.9f ? lmk(0.0f, 1.0f, 0.0f) : lmk(1.0f, 0.0f, 0.0f);
    const lv3 v = lunit(lcross(w, a));
    const lv3 u = lunit(lcross(w, v));
    const float phi = (xi_phi * 2.0f) * 3.14159265358979323846f;
    const float cos_theta = pow_plain(1.0f - xi_cos, gen_exp);
    const float sin_theta = __builtin_sqrtf(1.0f - cos_theta * cos_theta);
    float sp, cp;
    sincos_plain(phi, sp, cp);
    const float x = cp * sin_theta, y = sp * sin_theta;
    return ladd(ladd(lscale(u, x), lscale(v, y)), lscale(w, cos_theta));
}

// MixedMaterial::material_pdf(h, r) (material.rs:280-296), h = {p, n, incoming direction din}, r = {ro, rd}.  No clamp at 1; a NaN cosine
// passes the `cos < 0` test and flows on.
__host__ __device__ __forceinline__ float mixed_pdf(float exp, lv3 p, lv3 n, lv3 din, lv3 ro, lv3 rd) {
    if (!leq(ro, p)) return 0.0f;
    const float c0 = ldot(lunit(rd), lunit(n));
    const float cosv = ldot(din, n) < 0.0f ? c0 : -c0;
    if (cosv < 0.0f) return 0.0f;
    const float FRAC_1_2PI = 1.0f / 2.0f / 3.14159265358979323846f;
    return pow_plain(cosv, exp) * (exp + 1.0f) * FRAC_1_2PI;
}

} // namespace rtw
