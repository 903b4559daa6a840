// rtw_bounds.h -- neighbourhood colour bounds (variance clipping; include/rtw.h "neighbourhood colour bounds"): the rule of
// one pixel as ONE __host__ __device__ definition.  The host form (rtw_bounds.cpp) and both kernels (rtw_bounds.hip) run it with the same
// plan, so the device writes the host form's bytes: f32, one rounding per written operation under -ffp-contract=off, a correctly rounded
// divide and sqrtf, the taps in the order dy outer, dx inner, the mean in one sweep and the squared deviations from it in a second.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// What every pixel of a call shares: checked once by bounds_check (rtw_bounds.cpp).
struct BoundsPlan {
    uint32_t w = 0, h = 0;
    int radius = 1;
    float k = 0.0f;
    int same_object = 0, exclude_centre = 0;
};

struct BoundsColor { float r, g, b; };
struct BoundsBox { float lo[3], hi[3]; };

__host__ __device__ inline bool bounds_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // (false for NaN)

// x clipped to [lo, hi], written exactly so: a NaN bound clips nothing, and an x that is not finite stays as it is
__host__ __device__ inline float bounds_clip(float x, float lo, float hi) {
    if (!bounds_finite(x)) return x;
    return x < lo ? lo : (x > hi ? hi : x);
}

// Does the tap at (x + dx, y + dy) count for the centre (x, y) with id `idp`?  If so `c` is its colour.  The rule's four refusals in the
// rule's order; nothing is read from a tap outside the frame, and no colour from a tap on another object.
template <class Src>
__host__ __device__ inline bool bounds_tap(const BoundsPlan &pl, const Src &src, int x, int y, int dx, int dy, int32_t idp, BoundsColor &c) {
    const int qx = x + dx, qy = y + dy;
    if (qy < 0 || qy >= (int)pl.h || qx < 0 || qx >= (int)pl.w) return false;
    if (pl.exclude_centre && dx == 0 && dy == 0) return false;
    if (pl.same_object && src.id(qx, qy) != idp) return false;
    c = src.color(qx, qy);
    return bounds_finite(c.r) && bounds_finite(c.g) && bounds_finite(c.b);
}

// The box of pixel (x, y).  `src` answers color(qx, qy), and with same_object id(qx, qy), for pixels inside the frame: plain memory on the
// host and in the direct kernel, the workgroup's tile in the LDS kernel.  Both sweeps ask bounds_tap, so they add the same taps in the same
// order.
template <class Src>
__host__ __device__ inline BoundsBox bounds_pixel(const BoundsPlan &pl, const Src &src, int x, int y) {
    const int32_t idp = pl.same_object ? src.id(x, y) : 0;
    uint32_t n = 0;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    BoundsColor c;
    for (int dy = -pl.radius; dy <= pl.radius; dy++)
        for (int dx = -pl.radius; dx <= pl.radius; dx++) {
            if (!bounds_tap(pl, src, x, y, dx, dy, idp, c)) continue;
            n++;
            s0 = s0 + c.r;
            s1 = s1 + c.g;
            s2 = s2 + c.b;
        }
    BoundsBox o;
    if (n == 0) {
        for (int k = 0; k < 3; k++) { o.lo[k] = -__builtin_inff(); o.hi[k] = __builtin_inff(); }
        return o;
    }
    const float nf = (float)n;
    const float mu0 = s0 / nf, mu1 = s1 / nf, mu2 = s2 / nf;
    float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
    for (int dy = -pl.radius; dy <= pl.radius; dy++)
        for (int dx = -pl.radius; dx <= pl.radius; dx++) {
            if (!bounds_tap(pl, src, x, y, dx, dy, idp, c)) continue;
            const float d0 = c.r - mu0, d1 = c.g - mu1, d2 = c.b - mu2;
            q0 = q0 + d0 * d0;
            q1 = q1 + d1 * d1;
            q2 = q2 + d2 * d2;
        }
    const float e0 = pl.k * sqrtf(q0 / nf), e1 = pl.k * sqrtf(q1 / nf), e2 = pl.k * sqrtf(q2 / nf);
    o.lo[0] = mu0 - e0; o.hi[0] = mu0 + e0;
    o.lo[1] = mu1 - e1; o.hi[1] = mu1 + e1;
    o.lo[2] = mu2 - e2; o.hi[2] = mu2 + e2;
    return o;
}

// The source both sides read from plain memory.
struct BoundsMemSrc {
    const float *c;
    const int32_t *idx;
    uint32_t w;
    __host__ __device__ size_t at(int x, int y) const { return (size_t)y * w + (size_t)x; }
    __host__ __device__ BoundsColor color(int x, int y) const {
        const float *p = c + 3 * at(x, y);
        return BoundsColor{ p[0], p[1], p[2] };
    }
    __host__ __device__ int32_t id(int x, int y) const { return idx[at(x, y)]; }
};

// Pixel (x, y) of a call, from `src` into the caller's buffers (clamped may be null).
template <class Src>
__host__ __device__ inline void bounds_write(const BoundsPlan &pl, const Src &src, int x, int y, float *lo, float *hi, float *clamped) {
    const BoundsBox o = bounds_pixel(pl, src, x, y);
    const size_t p = 3 * ((size_t)y * pl.w + (size_t)x);
    lo[p] = o.lo[0]; lo[p + 1] = o.lo[1]; lo[p + 2] = o.lo[2];
    hi[p] = o.hi[0]; hi[p + 1] = o.hi[1]; hi[p + 2] = o.hi[2];
    if (clamped) {
        const BoundsColor c = src.color(x, y);
        clamped[p] = bounds_clip(c.r, o.lo[0], o.hi[0]);
        clamped[p + 1] = bounds_clip(c.g, o.lo[1], o.hi[1]);
        clamped[p + 2] = bounds_clip(c.b, o.lo[2], o.hi[2]);
    }
}

// Everything rtw_colour_bounds refuses (rtw.h); fills `pl`.  RTW_OK or RTW_E_INVALID.  (rtw_bounds.cpp)
int bounds_check(const float *in, uint32_t w, uint32_t h, const int32_t *idx, const RtwColourBounds *p, const float *out_lo, const float *out_hi,
                 const float *out_clamped, BoundsPlan &pl);

} // namespace rtw
