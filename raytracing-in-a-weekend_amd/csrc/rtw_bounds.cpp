// rtw_bounds.cpp -- the host form of the neighbourhood colour bounds (rtw_colour_bounds, include/rtw.h) and the argument check it shares
// with the device path (rtw_bounds.hip).  Pure host code: no HIP call.  One thread over the pixels, each running bounds_write
// (rtw_bounds.h), which the kernels run too.
#include "rtw_bounds.h"
#include "rtw_svgf.h"

#include <chrono>
#include <cmath>
#include <cstddef>

namespace rtw {

int bounds_check(const float *in, uint32_t w, uint32_t h, const int32_t *idx, const RtwColourBounds *p, const float *out_lo, const float *out_hi,
                 const float *out_clamped, BoundsPlan &pl) {
    if (!in || !p || !out_lo || !out_hi) return RTW_E_INVALID;
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (w > RTW_ATROUS_MAX_SIDE || h > RTW_ATROUS_MAX_SIDE) return RTW_E_INVALID;
    if (p->radius < 1 || p->radius > RTW_BOUNDS_MAX_RADIUS) return RTW_E_INVALID;
    if (!(p->k >= 0.0f) || !std::isfinite(p->k)) return RTW_E_INVALID;
    if (p->same_object > 1 || p->exclude_centre > 1) return RTW_E_INVALID;
    if (p->same_object && !idx) return RTW_E_INVALID;
    if (out_lo == out_hi || (out_clamped && (out_clamped == out_lo || out_clamped == out_hi))) return RTW_E_INVALID;
    if (out_lo == in || out_hi == in || out_clamped == in) return RTW_E_INVALID;           // neighbours gather from in
    pl = BoundsPlan();
    pl.w = w; pl.h = h;
    pl.radius = (int)p->radius;
    pl.k = p->k;
    pl.same_object = (int)p->same_object;
    pl.exclude_centre = (int)p->exclude_centre;
    return RTW_OK;
}

} // namespace rtw

using namespace rtw;

static_assert(sizeof(RtwColourBounds) == 16, "POD layout");

extern "C" int rtw_colour_bounds(const float *in, uint32_t w, uint32_t h, const int32_t *idx, const RtwColourBounds *params, float *out_lo,
                                 float *out_hi, float *out_clamped, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    BoundsPlan pl;
    const int rc = bounds_check(in, w, h, idx, params, out_lo, out_hi, out_clamped, pl);
    if (rc != RTW_OK) return rc;
    const BoundsMemSrc src = { in, idx, w };
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) bounds_write(pl, src, (int)x, (int)y, out_lo, out_hi, out_clamped);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, variance_taps(w, h, params->radius) };
    }
    return RTW_OK;
}
