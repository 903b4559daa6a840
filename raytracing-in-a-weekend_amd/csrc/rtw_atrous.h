// rtw_atrous.h -- the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; include/rtw.h "a-trous filter"): the rule
// of one pixel of one level, and of the demodulation around the levels, as ONE __host__ __device__ definition each.  The host form
// (rtw_atrous.cpp) and both kernels (rtw_atrous.hip) run these, so the device writes the host form's bytes: f32, one rounding per written
// operation under -ffp-contract=off, exp_plain for the exponential, the 25 taps in the order dy = -2..2 (outer), dx = -2..2 (inner).
#pragma once
#include "rtw_exp.h"
#include "rtw.h"

namespace rtw {

constexpr int ATROUS_COLOR = 1, ATROUS_DEPTH = 2, ATROUS_NORMAL = 4, ATROUS_IDX = 8;    // the terms that are on

struct AtrousColor { float r, g, b; };
struct AtrousGuide { float z, nx, ny, nz; int32_t id; };

// What a level needs beside its source: checked and derived once per call by atrous_check (rtw_atrous.cpp).
struct AtrousPlan {
    int terms = 0;
    uint32_t levels = 0;
    float inv_color[RTW_ATROUS_MAX_LEVELS] = {};     // 0.5 / (sigma_color 2^-i)^2
    float depth_scale[RTW_ATROUS_MAX_LEVELS] = {};   // 2^-i
    float inv_depth = 0.0f, inv_normal = 0.0f;
    float albedo_floor = 0.0f;
};

// The arguments of one level that are the same for every pixel.
struct AtrousLevel {
    int terms;
    int step;                                        // 1 << i
    uint32_t w, h;
    float inv_color, inv_depth, depth_scale, inv_normal;
};

// a_c of the rule: the albedo channel a pixel is divided by and multiplied back with
__host__ __device__ inline float atrous_albedo(const float *albedo, size_t i, float floor_) {
    if (!albedo) return 1.0f;
    const float a = albedo[i];
    return a >= floor_ ? a : 1.0f;
}

// C0[p][c] = (in[p][c] - e_c) / a_c, component i of the frame
__host__ __device__ inline float atrous_demodulate(const float *in, const float *albedo, const float *emitted, float floor_, size_t i) {
    const float e = emitted ? emitted[i] : 0.0f;
    return (in[i] - e) / atrous_albedo(albedo, i, floor_);
}

// out[p][c] = C[p][c] * a_c + e_c
__host__ __device__ inline float atrous_remodulate(float c, const float *albedo, const float *emitted, float floor_, size_t i) {
    const float e = emitted ? emitted[i] : 0.0f;
    return c * atrous_albedo(albedo, i, floor_) + e;
}

// The guide weight of tap q for centre p (with the colour difference): the guided filter's (rtw_filter.hip), a colour term in front and the
// depth difference scaled by 2^-i.
// Its two halves are separate so that the variance-steered filter (rtw_svgf.h) can add a term to `a` between them.
__host__ __device__ inline float atrous_exponent(const AtrousLevel &lv, const AtrousColor &cp, const AtrousGuide &gp, const AtrousColor &cq,
                                                 const AtrousGuide &gq) {
    float a = 0.0f;
    if (lv.terms & ATROUS_COLOR) {
        const float dx = cq.r - cp.r, dy = cq.g - cp.g, dz = cq.b - cp.b;
        a = a + lv.inv_color * ((dx * dx + dy * dy) + dz * dz);
    }
    if (lv.terms & ATROUS_DEPTH) {
        const float dz = (gq.z - gp.z) * lv.depth_scale;
        a = a + lv.inv_depth * (dz * dz);
    }
    if (lv.terms & ATROUS_NORMAL) {
        const float dx = gq.nx - gp.nx, dy = gq.ny - gp.ny, dz = gq.nz - gp.nz;
        a = a + lv.inv_normal * ((dx * dx + dy * dy) + dz * dz);
    }
    return a;
}
__host__ __device__ inline float atrous_gate(const AtrousLevel &lv, float a, const AtrousGuide &gp, const AtrousGuide &gq) {
    float g = a >= 0.0f ? exp_plain(-a) : 0.0f;
    if ((lv.terms & ATROUS_IDX) && gq.id != gp.id) g = 0.0f;
    return g;
}
__host__ __device__ inline float atrous_weight(const AtrousLevel &lv, const AtrousColor &cp, const AtrousGuide &gp, const AtrousColor &cq,
                                               const AtrousGuide &gq) {
    return atrous_gate(lv, atrous_exponent(lv, cp, gp, cq, gq), gp, gq);
}

// Pixel (x, y) of one level.  `src` answers color(qx, qy) and guide(qx, qy) for pixels inside the frame -- from global memory on the host
// and in the kernel that leaves the reuse to the caches, from the workgroup's tile in the LDS kernel; a guide whose term is off is not read.
// A tap outside the frame is skipped, and so is one whose weight is not > 0: for finite values that changes no bit (x + 0 * y == x, and a
// sum that only ever met zero weights is not used), and it is what lets a NaN or infinite tap drop out instead of entering as 0 * NaN.
template <class Src>
__host__ __device__ inline AtrousColor atrous_pixel(const AtrousLevel &lv, const Src &src, int x, int y) {
    const float K[3] = { 0.375f, 0.25f, 0.0625f };
    const AtrousColor cp = src.color(x, y);
    const AtrousGuide gp = src.guide(x, y);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wsum = 0.0f;
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
            const float wt = hw * atrous_weight(lv, cp, gp, cq, src.guide(qx, qy));
            if (wt > 0.0f) {
                s0 = s0 + cq.r * wt;
                s1 = s1 + cq.g * wt;
                s2 = s2 + cq.b * wt;
                wsum = wsum + wt;
            }
        }
    }
    AtrousColor o = cp;
    if (wsum > 0.0f) { o.r = s0 / wsum; o.g = s1 / wsum; o.b = s2 / wsum; }
    return o;
}

// The source both sides read from plain memory: the level's input [h][w][3] and the caller's guide planes.
struct AtrousMemSrc {
    const float *c;
    const float *depth, *normal;
    const int32_t *idx;
    uint32_t w;
    int terms;
    __host__ __device__ AtrousColor color(int x, int y) const {
        const float *p = c + 3 * ((size_t)y * w + (size_t)x);
        return AtrousColor{ p[0], p[1], p[2] };
    }
    __host__ __device__ AtrousGuide guide(int x, int y) const {
        const size_t i = (size_t)y * w + (size_t)x;
        AtrousGuide g = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
        if (terms & ATROUS_DEPTH) g.z = depth[i];
        if (terms & ATROUS_NORMAL) { g.nx = normal[3 * i]; g.ny = normal[3 * i + 1]; g.nz = normal[3 * i + 2]; }
        if (terms & ATROUS_IDX) g.id = idx[i];
        return g;
    }
};

inline AtrousLevel atrous_level(const AtrousPlan &pl, uint32_t i, uint32_t w, uint32_t h) {
    return AtrousLevel{ pl.terms, 1 << i, w, h, pl.inv_color[i], pl.inv_depth, pl.depth_scale[i], pl.inv_normal };
}

// Everything rtw_atrous_filter refuses (rtw.h); fills `pl`.  RTW_OK or RTW_E_INVALID.  (rtw_atrous.cpp)
int atrous_check(const float *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx, const float *albedo,
                 const RtwAtrous *p, const float *out, AtrousPlan &pl);
// In-frame taps of all levels of a w x h frame: RtwFilterStats.taps.  (rtw_atrous.cpp)
uint64_t atrous_taps(uint32_t w, uint32_t h, uint32_t levels);

} // namespace rtw
