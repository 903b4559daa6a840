// rtw_direct.h -- the sampling rule of direct lighting (rtw_light_samples / rtw_light_reduce / rtw_ctx_direct_light /
// rtw_ctx_direct_light_map): which ray is sample k of item (point i, light l) under a seed, whether it is cast, and what it
// weighs.  Everything here is __host__ __device__: one definition for direct_light_kernel (rtw_occluded.hip) and for the host forms
// (rtw_direct.cpp), so the kernel's rays and weights are rtw_light_samples' bit for bit.  f32, one rounding per written operation, no FMA
// (-ffp-contract=off) but sincos_plain's own.
//
// The ray is a SEGMENT: origin p, direction y - p to the sampled point y of the light, not normalised, walked over [lo, hi] in units of the
// segment (Renderer.segments_occluded's convention), so the light's own surface at t = 1 lies outside the range.  A sphere light is sampled
// uniformly over the hemisphere that faces the point; the part of that hemisphere beyond the sphere's own horizon is hidden by the sphere
// itself (its near side is met at t < 1), so those samples count as blocked.  That is intended: the estimate stays unbiased, the visible
// share of an unoccluded sphere light is its visible cap's share of the hemisphere, not 1.
#pragma once
#include "rtw_ao.h"

namespace rtw {

#define RTW_DIRECT_STREAM 0x4C495445u  /* "LITE": keeps an item's stream apart from the AO stream and the render's of the same index */
#define RTW_DIRECT_TWO_PI 6.2831855f

// One light as the rule reads it: four 16-byte rows, formed by direct_row_* below from the scene's RtwSphere / RtwQuad (the host forms read
// them from the scene, rtw_ctx_set_lights keeps them for the kernel's table).
struct alignas(16) DirectRow {
    float o[3]; uint32_t kind;            // quad: origin; sphere: RtwSphere.center (its place at time 0, the velocity is not read).  kind: RTW_LIGHT_*
    float u[3]; float r;                  // quad: edge u; sphere: r = the radius
    float v[3]; float area;               // quad: edge v; sphere: area = 6.2831855f * (r * r), the hemisphere's
    float g[3]; float pad;                // quad: cross(u, v)
};
static_assert(sizeof(DirectRow) == 64, "DirectRow is four f4 rows");

__host__ __device__ __forceinline__ DirectRow direct_row_sphere(const float c[3], float r) {
    DirectRow L;
    L.o[0] = c[0]; L.o[1] = c[1]; L.o[2] = c[2]; L.kind = 0u;      // RTW_LIGHT_SPHERE
    L.u[0] = L.u[1] = L.u[2] = 0.0f; L.r = r;
    L.v[0] = L.v[1] = L.v[2] = 0.0f; L.area = RTW_DIRECT_TWO_PI * (r * r);
    L.g[0] = L.g[1] = L.g[2] = 0.0f; L.pad = 0.0f;
    return L;
}
__host__ __device__ __forceinline__ DirectRow direct_row_quad(const float o[3], const float u[3], const float v[3]) {
    DirectRow L;
    const lv3 g = lcross(lmk(u[0], u[1], u[2]), lmk(v[0], v[1], v[2]));
    L.o[0] = o[0]; L.o[1] = o[1]; L.o[2] = o[2]; L.kind = 1u;      // RTW_LIGHT_QUAD
    L.u[0] = u[0]; L.u[1] = u[1]; L.u[2] = u[2]; L.r = 0.0f;
    L.v[0] = v[0]; L.v[1] = v[1]; L.v[2] = v[2]; L.area = 0.0f;
    L.g[0] = g.x; L.g[1] = g.y; L.g[2] = g.z; L.pad = 0.0f;
    return L;
}

// The (seed, point, light) prefix of the chain: ao_point_base's with this pass's stream constant, then the light's position in the list
__host__ __device__ __forceinline__ uint32_t direct_item_base(uint32_t seed, uint32_t i, uint32_t l) {
    uint32_t h = ao_mix32(seed + 0x9E3779B9U);
    h = ao_mix32(h ^ RTW_DIRECT_STREAM);
    h = ao_mix32(h ^ i);
    return ao_mix32(h ^ (l + 1u));
}

// Sample k of the item with stream prefix `base`: the direction d = y - p of its segment and its weight G (the geometric term; the normal as
// given).  Returns "the sample is cast": the normal is not exactly (0, 0, 0) and dot(n, d) > 0 (a NaN fails).  d and G are written either way;
// a sample that is not cast walks nothing and weighs +0.
__host__ __device__ __forceinline__ bool direct_sample(const DirectRow &L, uint32_t base, uint32_t k, lv3 p, lv3 n, lv3 &d, float &G) {
    float xi1, xi2;
    ao_draws(base, k, xi1, xi2);
    const lv3 o = lmk(L.o[0], L.o[1], L.o[2]);
    float num;
    if (L.kind == 1u) {
        const lv3 y = ladd(ladd(o, lscale(lmk(L.u[0], L.u[1], L.u[2]), xi1)), lscale(lmk(L.v[0], L.v[1], L.v[2]), xi2));
        d = lsub(y, p);
        num = ldot(n, d) * __builtin_fabsf(ldot(lmk(L.g[0], L.g[1], L.g[2]), d));     // the quad emits to both sides
    } else {
        const float z = 1.0f - 2.0f * xi1;
        const float s = __builtin_sqrtf(1.0f - z * z);
        float sn, cs;
        sincos_plain(RTW_DIRECT_TWO_PI * xi2, sn, cs);
        lv3 w = lmk(s * cs, s * sn, z);
        if (ldot(w, lsub(p, o)) < 0.0f) w = lneg(w);                                  // towards the point
        d = lsub(ladd(o, lscale(w, L.r)), p);
        const float m = -ldot(w, d);
        const float cl = m > 0.0f ? m : 0.0f;                                         // max(-dot(w, d), 0); a NaN gives 0
        num = (ldot(n, d) * cl) * L.area;
    }
    const float dd = ldot(d, d);
    G = num / (dd * dd);
    return !ao_skipped(n) && ldot(n, d) > 0.0f;
}

// The fixed association of an item's weights w[0 .. samples): with L = min(samples, 64), lane g adds w[g], w[g + L], ... to +0 in ascending
// order, then s[g] = s[g] + s[g + off] for g < off, off = L/2, L/4, ..., 1; the sum is s[0].  The kernel keeps s[g] in lane g of the item's group.
__host__ __device__ __forceinline__ float direct_sum(const float *w, uint32_t samples) {
    const uint32_t L = samples < 64u ? samples : 64u;
    float s[64];
    for (uint32_t g = 0; g < L; g++) {
        float a = 0.0f;
        for (uint32_t k = g; k < samples; k += L) a = a + w[k];
        s[g] = a;
    }
    for (uint32_t off = L >> 1; off > 0u; off >>= 1)
        for (uint32_t g = 0; g < off; g++) s[g] = s[g] + s[g + off];
    return s[0];
}

} // namespace rtw
