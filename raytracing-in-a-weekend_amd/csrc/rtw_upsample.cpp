// rtw_upsample.cpp -- the host form of the guide-steered upsampling (rtw_upsample_filter, include/rtw.h), the argument check it shares with
// the device path (rtw_upsample.hip), and rtw_camera_scaled.  Pure host code: no HIP call.  One thread over the output pixels, each running
// upsample_write (rtw_upsample.h), which the kernels run too.
#include "rtw_upsample.h"

#include <chrono>
#include <cmath>
#include <cstddef>

namespace rtw {

int upsample_check(const float *lo, uint32_t w_lo, uint32_t h_lo, const RtwGuides *g_lo, uint32_t w, uint32_t h, const RtwGuides *g_hi,
                   const RtwUpsample *p, float *out, float *wsum_out, UpsamplePlan &pl, UpsampleBufs &b) {
    if (!lo || !out || !p) return RTW_E_INVALID;
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (w > RTW_ATROUS_MAX_SIDE || h > RTW_ATROUS_MAX_SIDE) return RTW_E_INVALID;
    if (p->scale < 1 || p->scale > RTW_UPSAMPLE_MAX_SCALE) return RTW_E_INVALID;
    if (p->radius < 1 || p->radius > RTW_UPSAMPLE_MAX_RADIUS) return RTW_E_INVALID;
    if (w_lo != (w + p->scale - 1) / p->scale || h_lo != (h + p->scale - 1) / p->scale) return RTW_E_INVALID;
    if (!(p->sigma_depth >= 0.0f) || !std::isfinite(p->sigma_depth)) return RTW_E_INVALID;
    if (!(p->sigma_normal >= 0.0f) || !std::isfinite(p->sigma_normal)) return RTW_E_INVALID;
    if (p->same_object > 1) return RTW_E_INVALID;
    const RtwGuides none = { nullptr, nullptr, nullptr, nullptr, nullptr };
    const RtwGuides gl = g_lo ? *g_lo : none, gh = g_hi ? *g_hi : none;
    if ((gl.albedo || gh.albedo) && (!(p->albedo_floor > 0.0f) || !std::isfinite(p->albedo_floor))) return RTW_E_INVALID;
    pl = UpsamplePlan();
    pl.w = w; pl.h = h; pl.w_lo = w_lo; pl.h_lo = h_lo;
    pl.scale = (int)p->scale;
    pl.radius = (int)p->radius;
    pl.inv_s = 1.0f / (float)p->scale;
    pl.albedo_floor = p->albedo_floor;
    b = UpsampleBufs{ lo, { nullptr, nullptr, nullptr, gl.albedo, gl.emitted }, { nullptr, nullptr, nullptr, gh.albedo, gh.emitted }, out, wsum_out };
    if (p->sigma_depth > 0.0f) {
        pl.inv_depth = 0.5f / (p->sigma_depth * p->sigma_depth);
        if (!gl.depth || !gh.depth || !std::isfinite(pl.inv_depth)) return RTW_E_INVALID;
        pl.terms |= UPSAMPLE_DEPTH;
        b.g_lo.depth = gl.depth; b.g_hi.depth = gh.depth;
    }
    if (p->sigma_normal > 0.0f) {
        pl.inv_normal = 0.5f / (p->sigma_normal * p->sigma_normal);
        if (!gl.normal || !gh.normal || !std::isfinite(pl.inv_normal)) return RTW_E_INVALID;
        pl.terms |= UPSAMPLE_NORMAL;
        b.g_lo.normal = gl.normal; b.g_hi.normal = gh.normal;
    }
    if (p->same_object) {
        if (!gl.idx || !gh.idx) return RTW_E_INVALID;
        pl.terms |= UPSAMPLE_IDX;
        b.g_lo.idx = gl.idx; b.g_hi.idx = gh.idx;
    }
    // an output that is an input that is read, or the other output (the sizes differ: nothing is filtered in place)
    const void *ins[11] = { lo, b.g_lo.depth, b.g_lo.normal, b.g_lo.idx, b.g_lo.albedo, b.g_lo.emitted,
                            b.g_hi.depth, b.g_hi.normal, b.g_hi.idx, b.g_hi.albedo, b.g_hi.emitted };
    for (const void *q : ins)
        if (q && (q == out || q == wsum_out)) return RTW_E_INVALID;
    if (wsum_out == out) return RTW_E_INVALID;
    return RTW_OK;
}

uint64_t upsample_taps(const UpsamplePlan &pl) {
    // the taps are a product of a column set and a row set
    auto inside = [&](uint32_t n, uint32_t n_lo) {
        uint64_t k = 0;
        for (uint32_t i = 0; i < n; i++) {
            float t;
            const int64_t first = (int64_t)upsample_foot((int)i, pl.scale, t) - (pl.radius - 1), last = first + 2 * pl.radius - 1;
            const int64_t a = first < 0 ? 0 : first, b = last >= (int64_t)n_lo ? (int64_t)n_lo - 1 : last;
            if (b >= a) k += (uint64_t)(b - a + 1);
        }
        return k;
    };
    return inside(pl.w, pl.w_lo) * inside(pl.h, pl.h_lo);
}

} // namespace rtw

using namespace rtw;

static_assert(sizeof(RtwUpsample) == 24, "POD layout");
static_assert(sizeof(RtwGuides) == 5 * sizeof(void *), "POD layout");

extern "C" int rtw_upsample_filter(const float *lo, uint32_t w_lo, uint32_t h_lo, const RtwGuides *guides_lo, uint32_t w, uint32_t h,
                                   const RtwGuides *guides_hi, const RtwUpsample *params, float *out, float *wsum_out, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    UpsamplePlan pl;
    UpsampleBufs b;
    const int rc = upsample_check(lo, w_lo, h_lo, guides_lo, w, h, guides_hi, params, out, wsum_out, pl, b);
    if (rc != RTW_OK) return rc;
    const UpsampleMemSrc src = { b.lo, b.g_lo, w_lo, pl.terms, pl.albedo_floor };
    for (uint32_t j = 0; j < h; j++)
        for (uint32_t i = 0; i < w; i++) upsample_write(pl, src, b, (int)i, (int)j);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, upsample_taps(pl) };
    }
    return RTW_OK;
}

extern "C" int rtw_camera_scaled(const RtwCamera *cam, uint32_t scale, RtwCamera *out) {
    if (!cam || !out || scale < 1 || scale > RTW_UPSAMPLE_MAX_SCALE) return RTW_E_INVALID;
    RtwCamera c = *cam;
    const float s = (float)scale;
    for (int k = 0; k < 3; k++) { c.delta_u[k] = cam->delta_u[k] * s; c.delta_v[k] = cam->delta_v[k] * s; }
    *out = c;
    return RTW_OK;
}
