// rtw_atrous.cpp -- the host form of the a-trous filter (rtw_atrous_filter, include/rtw.h) and the argument checks it shares with the
// device path (rtw_atrous.hip).  Pure host code: no HIP call.  Demodulate, `levels` passes of atrous_pixel over two buffers, remodulate:
// the order of operations of each pixel is rtw_atrous.h's, which the kernels run too.
#include "rtw_atrous.h"

#include <chrono>
#include <cmath>
#include <cstddef>
#include <vector>

namespace rtw {

int atrous_check(const float *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx, const float *albedo,
                 const RtwAtrous *p, const float *out, AtrousPlan &pl) {
    if (!in || !out || !p) return RTW_E_INVALID;
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (w > RTW_ATROUS_MAX_SIDE || h > RTW_ATROUS_MAX_SIDE) return RTW_E_INVALID;          // pixel + 2 * step stays an int
    if (p->levels < 1 || p->levels > RTW_ATROUS_MAX_LEVELS) return RTW_E_INVALID;
    if (!(p->sigma_color >= 0.0f) || !std::isfinite(p->sigma_color)) return RTW_E_INVALID;
    if (!(p->sigma_depth >= 0.0f) || !std::isfinite(p->sigma_depth)) return RTW_E_INVALID;
    if (!(p->sigma_normal >= 0.0f) || !std::isfinite(p->sigma_normal)) return RTW_E_INVALID;
    if (p->same_object > 1) return RTW_E_INVALID;
    if (albedo && (!(p->albedo_floor > 0.0f) || !std::isfinite(p->albedo_floor))) return RTW_E_INVALID;
    pl = AtrousPlan();
    pl.levels = p->levels;
    pl.albedo_floor = p->albedo_floor;
    for (uint32_t i = 0; i < p->levels; i++) pl.depth_scale[i] = std::ldexp(1.0f, -(int)i);
    if (p->sigma_color > 0.0f) {
        for (uint32_t i = 0; i < p->levels; i++) {
            const float s = p->sigma_color * pl.depth_scale[i];
            pl.inv_color[i] = 0.5f / (s * s);
            if (!std::isfinite(pl.inv_color[i])) return RTW_E_INVALID;          // (a tiny sigma: inf * 0 for equal colours)
        }
        pl.terms |= ATROUS_COLOR;
    }
    if (p->sigma_depth > 0.0f) {
        pl.inv_depth = 0.5f / (p->sigma_depth * p->sigma_depth);
        if (!depth || !std::isfinite(pl.inv_depth)) return RTW_E_INVALID;
        pl.terms |= ATROUS_DEPTH;
    }
    if (p->sigma_normal > 0.0f) {
        pl.inv_normal = 0.5f / (p->sigma_normal * p->sigma_normal);
        if (!normal || !std::isfinite(pl.inv_normal)) return RTW_E_INVALID;
        pl.terms |= ATROUS_NORMAL;
    }
    if (p->same_object) {
        if (!idx) return RTW_E_INVALID;
        pl.terms |= ATROUS_IDX;
    }
    return RTW_OK;
}

uint64_t atrous_taps(uint32_t w, uint32_t h, uint32_t levels) {
    // the taps are a product of a column set and a row set: offset d * step stays inside for max(0, n - |d| step) pixels of a row of n
    uint64_t taps = 0;
    for (uint32_t i = 0; i < levels; i++) {
        uint64_t cols = 0, rows = 0;
        for (int d = -2; d <= 2; d++) {
            const uint64_t off = (uint64_t)(d < 0 ? -d : d) << i;
            cols += w > off ? w - off : 0;
            rows += h > off ? h - off : 0;
        }
        taps += cols * rows;
    }
    return taps;
}

} // namespace rtw

using namespace rtw;

static_assert(sizeof(RtwAtrous) == 24, "POD layout");

extern "C" int rtw_atrous_filter(const float *in, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                                 const float *albedo, const float *emitted, const RtwAtrous *params, float *out, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    AtrousPlan pl;
    const int rc = atrous_check(in, w, h, depth, normal, idx, albedo, params, out, pl);
    if (rc != RTW_OK) return rc;
    const size_t n = (size_t)w * h * 3;
    std::vector<float> a(n), b(n);
    for (size_t i = 0; i < n; i++) a[i] = atrous_demodulate(in, albedo, emitted, pl.albedo_floor, i);
    float *src = a.data(), *dst = b.data();
    for (uint32_t i = 0; i < pl.levels; i++) {
        const AtrousLevel lv = atrous_level(pl, i, w, h);
        const AtrousMemSrc ms = { src, depth, normal, idx, w, pl.terms };
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const AtrousColor c = atrous_pixel(lv, ms, (int)x, (int)y);
                float *o = dst + 3 * ((size_t)y * w + x);
                o[0] = c.r; o[1] = c.g; o[2] = c.b;
            }
        float *t = src; src = dst; dst = t;
    }
    for (size_t i = 0; i < n; i++) out[i] = atrous_remodulate(src[i], albedo, emitted, pl.albedo_floor, i);     // (out may be in: in was read above)
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, atrous_taps(w, h, pl.levels) };
    }
    return RTW_OK;
}
