// rtw_refit.h -- what the triangle tree's builder (rtw_tri.cpp) and its refit (host: rtw_tri.cpp, device: rtw_refit.hip) share: the inflated
// box of one triangle, the outward roundings, and the two steps of a refit -- one leaf node, one inner node.  One
// __host__ __device__ definition each; every translation unit that includes this is built with -ffp-contract=off.
#pragma once
#include "rtw_tri.h"

namespace rtw {

// The box of one triangle in double, inflated by the static part of the cull's error radius (DESIGN.md "Rust2 triangles"), and its centre.
struct TriBox { double lo[3], hi[3], c[3]; };

// std::min / std::max as the builder has always used them (the first argument stays on a tie or a NaN), spelled out so that host and device
// select alike
__host__ __device__ __forceinline__ double box_min(double a, double b) { return b < a ? b : a; }
__host__ __device__ __forceinline__ double box_max(double a, double b) { return a < b ? b : a; }
__host__ __device__ __forceinline__ float box_minf(float a, float b) { return b < a ? b : a; }
__host__ __device__ __forceinline__ float box_maxf(float a, float b) { return a < b ? b : a; }

// The f32 neighbour of f towards -inf / +inf (std::nextafter(f, -+INFINITY)) for a number; on the bits, so that no library stands between
// the two sides
__host__ __device__ __forceinline__ float box_next(float f, bool upward) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    if (f == 0.0f) b = upward ? 0x00000001u : 0x80000001u;
    else if (((b >> 31) != 0u) == upward) b = b - 1u;                            // towards zero (from an infinity: the largest number)
    else if ((b & 0x7FFFFFFFu) != 0x7F800000u) b = b + 1u;                       // away from zero (an infinity stays)
    __builtin_memcpy(&f, &b, 4);
    return f;
}
// The outward roundings of a double to f32: the largest f32 <= x, the smallest f32 >= x (NaN stays NaN)
__host__ __device__ __forceinline__ float box_down(double x) { float f = (float)x; if ((double)f > x) f = box_next(f, false); return f; }
__host__ __device__ __forceinline__ float box_up(double x) { float f = (float)x; if ((double)f < x) f = box_next(f, true); return f; }

// The inflated box of a prepared triangle (derived fields set); false: a condition of the cull's derivation fails, the tree must not be used
__host__ __device__ inline bool tri_box(const DevTri &t, TriBox &b) {
    bool ok = true;
    const float *f[] = { t.origin, t.u, t.v, t.normal, t.w };
    for (const float *p : f) for (int k = 0; k < 3; k++) if (!__builtin_isfinite(p[k])) ok = false;
    if (!__builtin_isfinite(t.d)) ok = false;
    if (!ok) {
        for (int k = 0; k < 3; k++) { b.lo[k] = b.hi[k] = b.c[k] = 0.0; }
        return false;
    }
    double amax = 0.0;
    for (int k = 0; k < 3; k++) {
        const double a = t.origin[k], p = a + (double)t.u[k], q = a + (double)t.v[k];
        b.lo[k] = box_min(a, box_min(p, q)); b.hi[k] = box_max(a, box_max(p, q));
        amax = box_max(amax, box_max(__builtin_fabs(b.lo[k]), __builtin_fabs(b.hi[k])));
        if (!(__builtin_fabs((double)t.w[k]) <= 0x1p40)) ok = false;
    }
    const double lu = __builtin_sqrt((double)t.u[0] * t.u[0] + (double)t.u[1] * t.u[1] + (double)t.u[2] * t.u[2]);
    const double lv = __builtin_sqrt((double)t.v[0] * t.v[0] + (double)t.v[1] * t.v[1] + (double)t.v[2] * t.v[2]);
    const double nx = (double)t.u[1] * t.v[2] - (double)t.u[2] * t.v[1], ny = (double)t.u[2] * t.v[0] - (double)t.u[0] * t.v[2],
                 nz = (double)t.u[0] * t.v[1] - (double)t.u[1] * t.v[0];
    const double nl = __builtin_sqrt(nx * nx + ny * ny + nz * nz), e = box_max(lu, lv);
    const double kappa = nl > 0.0 ? e * e / nl : __builtin_huge_val();
    if (!(amax <= 0x1p40) || !(kappa <= 256.0)) ok = false;
    const double r = 0x1p-24 * (256.0 * amax + 4096.0 * kappa * (1.0 + kappa) * e) + 0x1p-100;
    for (int k = 0; k < 3; k++) {
        b.lo[k] -= r; b.hi[k] += r;
        b.c[k] = 0.5 * (b.lo[k] + b.hi[k]);
    }
    return ok;
}

// ---- the refit -----------------------------------------------------------------------------------------------------------
// The topology stays: skip links, leaf words, the leaf order and every `index`.  Both steps are the whole of what either side runs.
//
// One leaf node: each of its triangles takes origin, u, v of its index from `ouv` ([n][9] f32), Triangle::new's derived fields, and is
// written to its slot of `leaf` and to `list[index]` -- rows 0 to 4 without the w words of rows 1 to 4 (index, metallicness, opacity, ir);
// rows 5 and 6 stay.  The node's box becomes the union of the triangles' boxes rounded outward.  Returns how many of them tri_box refuses.
__host__ __device__ inline uint32_t refit_leaf_node(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, uint32_t node) {
    TriNode &nd = nodes[node];
    const uint32_t first = nd.leaf >> 3, cnt = nd.leaf & 7u;
    float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
    uint32_t bad = 0;
    for (uint32_t j = first; j < first + cnt; j++) {
        DevTri &slot = leaf[j];
        const uint32_t index = slot.index;
        const float *s = ouv + 9 * (size_t)index;
        DevTri t;
        for (int k = 0; k < 3; k++) { t.origin[k] = s[k]; t.u[k] = s[3 + k]; t.v[k] = s[6 + k]; }
        tri_derive(t.origin, t.u, t.v, t.normal, t.d, t.w);
        DevTri &row = list[index];
        for (int k = 0; k < 3; k++) {
            slot.origin[k] = row.origin[k] = t.origin[k]; slot.u[k] = row.u[k] = t.u[k]; slot.v[k] = row.v[k] = t.v[k];
            slot.normal[k] = row.normal[k] = t.normal[k]; slot.w[k] = row.w[k] = t.w[k];
        }
        slot.d = row.d = t.d;
        TriBox b;
        if (!tri_box(t, b)) bad++;
        for (int k = 0; k < 3; k++) {
            const float l = box_down(b.lo[k]), h = box_up(b.hi[k]);
            lo[k] = j == first ? l : box_minf(lo[k], l); hi[k] = j == first ? h : box_maxf(hi[k], h);
        }
    }
    for (int k = 0; k < 3; k++) { nd.lo[k] = lo[k]; nd.hi[k] = hi[k]; }
    return bad;
}
// One inner node, after both children: down and up are monotone, so the f32 union of the children's boxes is the outward rounding of the
// double union the builder forms
__host__ __device__ inline void refit_inner_node(TriNode *nodes, uint32_t node) {
    const TriNode &l = nodes[node + 1];
    const TriNode &r = nodes[l.skip];
    TriNode &nd = nodes[node];
    for (int k = 0; k < 3; k++) { nd.lo[k] = box_minf(l.lo[k], r.lo[k]); nd.hi[k] = box_maxf(l.hi[k], r.hi[k]); }
}

// ---- host (rtw_tri.cpp) ---------------------------------------------------------------------------------------------------------------------
// The order a refit visits the nodes in: `order` holds every node index sorted by height (a leaf: 0; an inner node: 1 + the higher child),
// ties by index; height h owns order[first[h] .. first[h + 1]), first.size() = heights + 1.  Height 0 is the leaf pass, each further height
// one launch.  False when memory runs out.
struct RefitSchedule {
    std::vector<uint32_t> order, first;
};
bool tri_refit_schedule(const TriNode *nodes, uint32_t n_nodes, RefitSchedule &out);
// The refit on the host, over the same schedule: returns the number of triangles tri_box refuses
uint32_t tri_refit_host(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, const RefitSchedule &s);

// ---- device (rtw_refit.hip) -----------------------------------------------------------------------------------------------------------------
// The refit on `stream`: the leaf pass, then one launch per height; device pointers, `order` = RefitSchedule.order uploaded, `first` the host
// array; *bad (device u32, zeroed by the caller) receives the count.  Allocates nothing.
void launch_tri_refit(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, const uint32_t *order, const uint32_t *first,
                      uint32_t n_heights, uint32_t *bad, hipStream_t stream);

} // namespace rtw
