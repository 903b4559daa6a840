// rtw_svgf.h -- the variance-steered a-trous filter and the variance estimate that feeds it (Schied et al. 2017, SVGF's filter stage;
// include/rtw.h "variance estimate" and "variance-steered a-trous filter"): the rule of one pixel of each pass as ONE
// __host__ __device__ definition.  The host forms (rtw_svgf.cpp) and the kernels (rtw_svgf.hip) run these with the same plan, so the device
// writes the host forms' bytes: f32, one rounding per written operation under -ffp-contract=off, exp_plain for the exponential, the taps
// in the order dy outer, dx inner.  The guide terms, the tap weights and the demodulation are the a-trous filter's (rtw_atrous.h).
#pragma once
#include "rtw_atrous.h"

namespace rtw {

// lum(c) = (0.2126f r + 0.7152f g) + 0.0722f b: the temporal accumulation's luminance (rtw_temporal.h)
__host__ __device__ inline float svgf_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// ---- the variance estimate -------------------------------------------------------------------------------------------------------------
// What every pixel of a call shares: checked and derived once by variance_check (rtw_svgf.cpp).  lv carries the guide terms for
// atrous_exponent / atrous_gate: no colour term, depth scale 1.
struct VariancePlan {
    AtrousLevel lv = {};
    float min_history = 1.0f;
    int radius = 1;
};

// Pixel (x, y).  `src` answers m1, m2, len and guide for pixels inside the frame: plain memory on the host and in the direct kernel, the
// workgroup's tile in the LDS kernel; a guide whose term is off is not read.
template <class Src>
__host__ __device__ inline float variance_pixel(const VariancePlan &pl, const Src &src, int x, int y) {
    const float n = src.len(x, y);
    if (n >= pl.min_history) {
        const float m1 = src.m1(x, y), m2 = src.m2(x, y);
        const float v = m2 - m1 * m1;
        return v > 0.0f ? v : 0.0f;
    }
    const AtrousColor none = { 0.0f, 0.0f, 0.0f };
    const AtrousGuide gp = src.guide(x, y);
    float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
    for (int dy = -pl.radius; dy <= pl.radius; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)pl.lv.h) continue;
        for (int dx = -pl.radius; dx <= pl.radius; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)pl.lv.w) continue;
            if (!(src.len(qx, qy) > 0.0f)) continue;                                     // (a hole: 0, or NaN)
            const AtrousGuide gq = src.guide(qx, qy);
            const float g = atrous_gate(pl.lv, atrous_exponent(pl.lv, none, gp, none, gq), gp, gq);
            if (g > 0.0f) {
                s1 = s1 + g * src.m1(qx, qy);
                s2 = s2 + g * src.m2(qx, qy);
                ws = ws + g;
            }
        }
    }
    if (!(ws > 0.0f)) return 0.0f;
    const float M1 = s1 / ws, M2 = s2 / ws;
    float v = M2 - M1 * M1;
    v = v > 0.0f ? v : 0.0f;
    return v * (pl.min_history / (n >= 1.0f ? n : 1.0f));                                // SVGF's boost of a short history
}

// The source both sides read from plain memory.
struct VarianceMemSrc {
    const float *moments, *length;
    AtrousMemSrc g;                                                                      // (its colour is not read)
    __host__ __device__ size_t at(int x, int y) const { return (size_t)y * g.w + (size_t)x; }
    __host__ __device__ float m1(int x, int y) const { return moments[2 * at(x, y)]; }
    __host__ __device__ float m2(int x, int y) const { return moments[2 * at(x, y) + 1]; }
    __host__ __device__ float len(int x, int y) const { return length[at(x, y)]; }
    __host__ __device__ AtrousGuide guide(int x, int y) const { return g.guide(x, y); }
};

// ---- the variance-steered a-trous filter -----------------------------------------------------------------------------------------------
// What a level needs beside the a-trous filter's: checked and derived once per call by svgf_check (rtw_svgf.cpp).
struct SvgfPlan {
    AtrousPlan at;
    int lum_on = 0;                  // sigma_luminance > 0
    int prefilter = 0;
    float sl2 = 0.0f;                // 2 * sigma_luminance * sigma_luminance
    float epsilon = 0.0f;
};
struct SvgfLevel {
    AtrousLevel lv;
    int lum_on, prefilter;
    float sl2, epsilon;
};
struct SvgfPixel { AtrousColor c; float v; };

// la * la of the rule: the square of the luminance of the albedo the demodulation divides pixel p by (exactly 1 without albedo)
__host__ __device__ inline float svgf_albedo_lum2(const float *albedo, size_t p, float floor_) {
    const float la = svgf_lum(atrous_albedo(albedo, 3 * p, floor_), atrous_albedo(albedo, 3 * p + 1, floor_), atrous_albedo(albedo, 3 * p + 2, floor_));
    return la * la;
}
// V0[p]: NaN and negatives become 0, +inf stays
__host__ __device__ inline float svgf_demodulate_variance(const float *variance, const float *albedo, float floor_, size_t p) {
    const float v = variance[p];
    return v > 0.0f ? v / svgf_albedo_lum2(albedo, p, floor_) : 0.0f;
}
__host__ __device__ inline float svgf_remodulate_variance(float v, const float *albedo, float floor_, size_t p) {
    return v * svgf_albedo_lum2(albedo, p, floor_);
}

// Pixel (x, y) of one level.  `src` answers color, guide and var for pixels inside the frame, as atrous_pixel's does.  The 3 x 3 prefilter
// of the variance steps by 1 at every level, so it stays within one pixel of the centre.
template <class Src>
__host__ __device__ inline SvgfPixel svgf_pixel(const SvgfLevel &sv, const Src &src, int x, int y) {
    const AtrousLevel &lv = sv.lv;
    const float K[3] = { 0.375f, 0.25f, 0.0625f };
    const AtrousColor cp = src.color(x, y);
    const AtrousGuide gp = src.guide(x, y);
    const float vp = src.var(x, y);
    float lp = 0.0f, den = 1.0f;
    if (sv.lum_on) {
        lp = svgf_lum(cp.r, cp.g, cp.b);
        float vbar = vp;
        if (sv.prefilter) {
            const float G[2] = { 0.5f, 0.25f };
            float num = 0.0f, gs = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int qy = y + dy;
                if (qy < 0 || qy >= (int)lv.h) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= (int)lv.w) continue;
                    const float gw = G[dx < 0 ? -dx : dx] * G[dy < 0 ? -dy : dy];
                    num = num + gw * src.var(qx, qy);
                    gs = gs + gw;
                }
            }
            vbar = num / gs;
        }
        den = sv.sl2 * vbar + sv.epsilon;
    }
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wsum = 0.0f, vs = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * lv.step;
        if (qy < 0 || qy >= (int)lv.h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * lv.step;
            if (qx < 0 || qx >= (int)lv.w) continue;
            const float hw = K[dx < 0 ? -dx : dx] * K[dy < 0 ? -dy : dy];
            const AtrousColor cq = src.color(qx, qy);
            const AtrousGuide gq = src.guide(qx, qy);
            float a = atrous_exponent(lv, cp, gp, cq, gq);
            if (sv.lum_on) {
                const float dl = svgf_lum(cq.r, cq.g, cq.b) - lp;
                a = a + (dl * dl) / den;
            }
            const float wt = hw * atrous_gate(lv, a, gp, gq);
            if (wt > 0.0f) {
                s0 = s0 + cq.r * wt;
                s1 = s1 + cq.g * wt;
                s2 = s2 + cq.b * wt;
                wsum = wsum + wt;
                vs = vs + (wt * wt) * src.var(qx, qy);
            }
        }
    }
    SvgfPixel o = { cp, vp };
    if (wsum > 0.0f) { o.c.r = s0 / wsum; o.c.g = s1 / wsum; o.c.b = s2 / wsum; o.v = vs / (wsum * wsum); }
    return o;
}

// The source both sides read from plain memory: the a-trous filter's plus the level's variance plane [h][w].
struct SvgfMemSrc {
    AtrousMemSrc m;
    const float *v;
    __host__ __device__ AtrousColor color(int x, int y) const { return m.color(x, y); }
    __host__ __device__ AtrousGuide guide(int x, int y) const { return m.guide(x, y); }
    __host__ __device__ float var(int x, int y) const { return v[(size_t)y * m.w + (size_t)x]; }
};

inline SvgfLevel svgf_level(const SvgfPlan &pl, uint32_t i, uint32_t w, uint32_t h) {
    return SvgfLevel{ atrous_level(pl.at, i, w, h), pl.lum_on, pl.prefilter, pl.sl2, pl.epsilon };
}

// Everything rtw_variance_estimate refuses (rtw.h); fills `pl`.  RTW_OK or RTW_E_INVALID.  (rtw_svgf.cpp)
int variance_check(const float *moments, const float *len, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                   const RtwVarianceEstimate *p, const float *out, VariancePlan &pl);
// Everything rtw_svgf_filter refuses (rtw.h): atrous_check's, and its own; fills `pl`.  (rtw_svgf.cpp)
int svgf_check(const float *in, const float *variance, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
               const float *albedo, const RtwAtrous *p, const RtwSvgf *vp, const float *out, const float *out_variance, SvgfPlan &pl);
// Window entries inside the frame, (2 radius + 1)^2 per pixel away from the border: RtwFilterStats.taps of the variance estimate.
uint64_t variance_taps(uint32_t w, uint32_t h, uint32_t radius);

} // namespace rtw
