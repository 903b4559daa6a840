// rtw_upsample.h -- guide-steered upsampling of a low-resolution frame (joint bilateral upsampling, Kopf et al. 2007, on demodulated colour;
// include/rtw.h "guided upsampling"): the rule of one output pixel as ONE __host__ __device__ definition.  The host form
// (rtw_upsample.cpp) and both kernels (rtw_upsample.hip) run it with the same plan, so the device writes the host form's bytes: f32, one
// rounding per written operation under -ffp-contract=off, a correctly rounded divide, exp_plain for the exponential, the footprint formed in
// integers, the taps in the order ky outer, kx inner.
#pragma once
#include "rtw_exp.h"
#include "rtw.h"

namespace rtw {

constexpr int UPSAMPLE_DEPTH = 1, UPSAMPLE_NORMAL = 2, UPSAMPLE_IDX = 4;       // the guide terms that are on

// What every pixel of a call shares: checked and derived once by upsample_check (rtw_upsample.cpp).
struct UpsamplePlan {
    uint32_t w = 0, h = 0, w_lo = 0, h_lo = 0;
    int scale = 1, radius = 1;
    int terms = 0;
    float inv_s = 1.0f;                              // 1.0f / (float)scale
    float inv_depth = 0.0f, inv_normal = 0.0f;
    float albedo_floor = 0.0f;
};

struct UpsampleColor { float r, g, b; };
struct UpsampleGuide { float z, nx, ny, nz; int32_t id; };

// The caller's buffers as every pixel sees them (guide pointers whose term is off are null).
struct UpsampleBufs {
    const float *lo;
    RtwGuides g_lo, g_hi;
    float *out, *wsum;
};

__host__ __device__ inline bool upsample_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }    // (false for NaN)

// a_c of the rule: the albedo channel a pixel is divided by on the way in, or multiplied with on the way out
__host__ __device__ inline float upsample_albedo(const float *albedo, size_t i, float floor_) {
    if (!albedo) return 1.0f;
    const float a = albedo[i];
    return a >= floor_ ? a : 1.0f;
}

// L[q] = (lo[q] - e) / a of low pixel number q
__host__ __device__ inline UpsampleColor upsample_demodulate(const float *lo, const float *albedo, const float *emitted, float floor_, size_t q) {
    float L[3];
    for (int c = 0; c < 3; c++) {
        const size_t i = 3 * q + (size_t)c;
        const float e = emitted ? emitted[i] : 0.0f;
        L[c] = (lo[i] - e) / upsample_albedo(albedo, i, floor_);
    }
    return UpsampleColor{ L[0], L[1], L[2] };
}

// The guides of pixel number q of one side; a guide whose term is off is not read.
__host__ __device__ inline UpsampleGuide upsample_guide(const RtwGuides &g, int terms, size_t q) {
    UpsampleGuide o = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
    if (terms & UPSAMPLE_DEPTH) o.z = g.depth[q];
    if (terms & UPSAMPLE_NORMAL) { o.nx = g.normal[3 * q]; o.ny = g.normal[3 * q + 1]; o.nz = g.normal[3 * q + 2]; }
    if (terms & UPSAMPLE_IDX) o.id = g.idx[q];
    return o;
}

// The footprint of output coordinate i at scale s: I0 = floor((2 i + 1 - s) / (2 s)) and t = the remainder over 2 s, i.e. the position of
// the output pixel's centre between the centres of low pixels I0 and I0 + 1.  With i = s a + b the numerator is 2 s a + (2 b + 1 - s), whose
// second part lies in [1 - s, s - 1]: the floor is a - 1 or a, and nothing overflows for any i below RTW_ATROUS_MAX_SIDE.
__host__ __device__ inline int upsample_foot(int i, int s, float &t) {
    const int a = i / s, r = 2 * (i - a * s) + 1 - s;           // N = 2 s a + r
    const int below = r < 0 ? 1 : 0;
    t = (float)(r + below * 2 * s) / (float)(2 * s);
    return a - below;
}

// The tent weight of tap k (-(radius-1) .. radius) at fraction t: 1 - |k - t| / radius scaled by radius; the bilinear weights at radius 1.
__host__ __device__ inline float upsample_tent(int k, int radius, float t) {
    return k <= 0 ? (float)(radius + k) - t : (float)(radius - k) + t;
}

// Output pixel (i, j) before remodulation: c is C of the rule; the return value is wsum (0 exactly where the fallback was taken).  `src`
// answers color(I, J) -- the DEMODULATED low pixel -- and guide(I, J) for low pixels inside the low frame: plain memory on the host and in
// the direct kernel, the workgroup's tile in the LDS kernel.
template <class Src>
__host__ __device__ inline float upsample_pixel(const UpsamplePlan &pl, const Src &src, const UpsampleGuide &gp, int i, int j, UpsampleColor &c) {
    float tx, ty;
    const int I0 = upsample_foot(i, pl.scale, tx), J0 = upsample_foot(j, pl.scale, ty);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wsum = 0.0f;
    for (int ky = -(pl.radius - 1); ky <= pl.radius; ky++) {
        const int qy = J0 + ky;
        if (qy < 0 || qy >= (int)pl.h_lo) continue;
        const float wy = upsample_tent(ky, pl.radius, ty);
        for (int kx = -(pl.radius - 1); kx <= pl.radius; kx++) {
            const int qx = I0 + kx;
            if (qx < 0 || qx >= (int)pl.w_lo) continue;
            const float wx = upsample_tent(kx, pl.radius, tx);
            const float hw = wx * wy;
            const UpsampleGuide gq = src.guide(qx, qy);
            float a = 0.0f;
            if (pl.terms & UPSAMPLE_DEPTH) {
                const float dz = (gq.z - gp.z) * pl.inv_s;
                a = a + pl.inv_depth * (dz * dz);
            }
            if (pl.terms & UPSAMPLE_NORMAL) {
                const float dx = gq.nx - gp.nx, dy = gq.ny - gp.ny, dz = gq.nz - gp.nz;
                a = a + pl.inv_normal * ((dx * dx + dy * dy) + dz * dz);
            }
            float g = a >= 0.0f ? exp_plain(-a) : 0.0f;
            if ((pl.terms & UPSAMPLE_IDX) && gq.id != gp.id) g = 0.0f;
            const float wt = hw * g;
            if (!(wt > 0.0f)) continue;
            const UpsampleColor L = src.color(qx, qy);
            if (!(upsample_finite(L.r) && upsample_finite(L.g) && upsample_finite(L.b))) continue;
            s0 = s0 + L.r * wt;
            s1 = s1 + L.g * wt;
            s2 = s2 + L.b * wt;
            wsum = wsum + wt;
        }
    }
    if (wsum > 0.0f) { c.r = s0 / wsum; c.g = s1 / wsum; c.b = s2 / wsum; }
    else c = src.color(i / pl.scale, j / pl.scale);             // the covering low pixel, unguided; a NaN there passes through
    return wsum;
}

// The source both sides read from plain memory: the low frame, demodulated tap by tap, and the low guides.
struct UpsampleMemSrc {
    const float *lo;
    RtwGuides g;
    uint32_t w_lo;
    int terms;
    float albedo_floor;
    __host__ __device__ size_t at(int x, int y) const { return (size_t)y * w_lo + (size_t)x; }
    __host__ __device__ UpsampleColor color(int x, int y) const { return upsample_demodulate(lo, g.albedo, g.emitted, albedo_floor, at(x, y)); }
    __host__ __device__ UpsampleGuide guide(int x, int y) const { return upsample_guide(g, terms, at(x, y)); }
};

// Output pixel (i, j) of a call, from `src` into the caller's buffers: the rule's result, remodulated with the output-size albedo and
// emission.
template <class Src>
__host__ __device__ inline void upsample_write(const UpsamplePlan &pl, const Src &src, const UpsampleBufs &b, int i, int j) {
    const size_t p = (size_t)j * pl.w + (size_t)i;
    UpsampleColor c;
    const float wsum = upsample_pixel(pl, src, upsample_guide(b.g_hi, pl.terms, p), i, j, c);
    const float C[3] = { c.r, c.g, c.b };
    for (int k = 0; k < 3; k++) {
        const size_t n = 3 * p + (size_t)k;
        const float e = b.g_hi.emitted ? b.g_hi.emitted[n] : 0.0f;
        b.out[n] = C[k] * upsample_albedo(b.g_hi.albedo, n, pl.albedo_floor) + e;
    }
    if (b.wsum) b.wsum[p] = wsum;
}

// Everything rtw_upsample_filter refuses (rtw.h); fills `pl` and `b` (off guides null).  RTW_OK or RTW_E_INVALID.  (rtw_upsample.cpp)
int upsample_check(const float *lo, uint32_t w_lo, uint32_t h_lo, const RtwGuides *g_lo, uint32_t w, uint32_t h, const RtwGuides *g_hi,
                   const RtwUpsample *p, float *out, float *wsum_out, UpsamplePlan &pl, UpsampleBufs &b);
// Taps inside the low frame over all output pixels: RtwFilterStats.taps.  (rtw_upsample.cpp)
uint64_t upsample_taps(const UpsamplePlan &pl);

} // namespace rtw
