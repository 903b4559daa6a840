// rtw_svgf.cpp -- the host forms of the variance estimate and of the variance-steered a-trous filter (rtw_variance_estimate,
// rtw_svgf_filter, include/rtw.h) and the argument checks they share with the device paths (rtw_svgf.hip).  Pure host code: no HIP call.
// The order of operations of each pixel is rtw_svgf.h's, which the kernels run too.
#include "rtw_svgf.h"

#include <chrono>
#include <cmath>
#include <cstddef>
#include <vector>

namespace rtw {

int variance_check(const float *moments, const float *len, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
                   const RtwVarianceEstimate *p, const float *out, VariancePlan &pl) {
    if (!moments || !len || !out || !p) return RTW_E_INVALID;
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (w > RTW_ATROUS_MAX_SIDE || h > RTW_ATROUS_MAX_SIDE) return RTW_E_INVALID;
    if (p->min_history < 1 || p->min_history > 65535) return RTW_E_INVALID;
    if (p->radius < 1 || p->radius > RTW_VARIANCE_MAX_RADIUS) return RTW_E_INVALID;
    if (!(p->sigma_depth >= 0.0f) || !std::isfinite(p->sigma_depth)) return RTW_E_INVALID;
    if (!(p->sigma_normal >= 0.0f) || !std::isfinite(p->sigma_normal)) return RTW_E_INVALID;
    if (p->same_object > 1) return RTW_E_INVALID;
    if (out == moments || out == len) return RTW_E_INVALID;                              // neighbours gather from both
    pl = VariancePlan();
    pl.min_history = (float)p->min_history;
    pl.radius = (int)p->radius;
    pl.lv = AtrousLevel{ 0, 1, w, h, 0.0f, 0.0f, 1.0f, 0.0f };
    if (p->sigma_depth > 0.0f) {
        pl.lv.inv_depth = 0.5f / (p->sigma_depth * p->sigma_depth);
        if (!depth || !std::isfinite(pl.lv.inv_depth)) return RTW_E_INVALID;
        pl.lv.terms |= ATROUS_DEPTH;
    }
    if (p->sigma_normal > 0.0f) {
        pl.lv.inv_normal = 0.5f / (p->sigma_normal * p->sigma_normal);
        if (!normal || !std::isfinite(pl.lv.inv_normal)) return RTW_E_INVALID;
        pl.lv.terms |= ATROUS_NORMAL;
    }
    if (p->same_object) {
        if (!idx) return RTW_E_INVALID;
        pl.lv.terms |= ATROUS_IDX;
    }
    return RTW_OK;
}

int svgf_check(const float *in, const float *variance, uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx,
               const float *albedo, const RtwAtrous *p, const RtwSvgf *vp, const float *out, const float *out_variance, SvgfPlan &pl) {
    if (!variance || !vp) return RTW_E_INVALID;
    pl = SvgfPlan();
    const int rc = atrous_check(in, w, h, depth, normal, idx, albedo, p, out, pl.at);
    if (rc != RTW_OK) return rc;
    if (!(vp->sigma_luminance >= 0.0f) || !std::isfinite(vp->sigma_luminance)) return RTW_E_INVALID;
    if (!(vp->epsilon > 0.0f) || !std::isfinite(vp->epsilon)) return RTW_E_INVALID;
    if (vp->prefilter > 1) return RTW_E_INVALID;
    if (out_variance && (out_variance == variance || out_variance == in || out_variance == out)) return RTW_E_INVALID;
    pl.sl2 = 2.0f * vp->sigma_luminance * vp->sigma_luminance;
    if (!std::isfinite(pl.sl2)) return RTW_E_INVALID;
    pl.lum_on = vp->sigma_luminance > 0.0f;
    pl.prefilter = (int)vp->prefilter;
    pl.epsilon = vp->epsilon;
    return RTW_OK;
}

uint64_t variance_taps(uint32_t w, uint32_t h, uint32_t radius) {
    uint64_t cols = 0, rows = 0;
    for (int d = -(int)radius; d <= (int)radius; d++) {
        const uint64_t off = (uint64_t)(d < 0 ? -d : d);
        cols += w > off ? w - off : 0;
        rows += h > off ? h - off : 0;
    }
    return cols * rows;
}

} // namespace rtw

using namespace rtw;

static_assert(sizeof(RtwVarianceEstimate) == 20 && sizeof(RtwSvgf) == 12, "POD layout");

extern "C" int rtw_variance_estimate(const float *moments, const float *len, uint32_t w, uint32_t h, const float *depth, const float *normal,
                                     const int32_t *idx, const RtwVarianceEstimate *params, float *out, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    VariancePlan pl;
    const int rc = variance_check(moments, len, w, h, depth, normal, idx, params, out, pl);
    if (rc != RTW_OK) return rc;
    const VarianceMemSrc src = { moments, len, AtrousMemSrc{ nullptr, depth, normal, idx, w, pl.lv.terms } };
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) out[(size_t)y * w + x] = variance_pixel(pl, src, (int)x, (int)y);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, variance_taps(w, h, params->radius) };
    }
    return RTW_OK;
}

extern "C" int rtw_svgf_filter(const float *in, const float *variance, uint32_t w, uint32_t h, const float *depth, const float *normal,
                               const int32_t *idx, const float *albedo, const float *emitted, const RtwAtrous *params, const RtwSvgf *vparams,
                               float *out, float *out_variance, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    SvgfPlan pl;
    const int rc = svgf_check(in, variance, w, h, depth, normal, idx, albedo, params, vparams, out, out_variance, pl);
    if (rc != RTW_OK) return rc;
    const size_t n_px = (size_t)w * h, n = n_px * 3;
    const float floor_ = pl.at.albedo_floor;
    std::vector<float> a(n), b(n), va(n_px), vb(n_px);
    for (size_t i = 0; i < n; i++) a[i] = atrous_demodulate(in, albedo, emitted, floor_, i);
    for (size_t p = 0; p < n_px; p++) va[p] = svgf_demodulate_variance(variance, albedo, floor_, p);
    float *src = a.data(), *dst = b.data(), *vsrc = va.data(), *vdst = vb.data();
    for (uint32_t i = 0; i < pl.at.levels; i++) {
        const SvgfLevel sv = svgf_level(pl, i, w, h);
        const SvgfMemSrc ms = { AtrousMemSrc{ src, depth, normal, idx, w, pl.at.terms }, vsrc };
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const SvgfPixel o = svgf_pixel(sv, ms, (int)x, (int)y);
                const size_t p = (size_t)y * w + x;
                dst[3 * p] = o.c.r; dst[3 * p + 1] = o.c.g; dst[3 * p + 2] = o.c.b;
                vdst[p] = o.v;
            }
        float *t = src; src = dst; dst = t;
        t = vsrc; vsrc = vdst; vdst = t;
    }
    for (size_t i = 0; i < n; i++) out[i] = atrous_remodulate(src[i], albedo, emitted, floor_, i);       // (out may be in: in was read above)
    if (out_variance)
        for (size_t p = 0; p < n_px; p++) out_variance[p] = svgf_remodulate_variance(vsrc[p], albedo, floor_, p);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, atrous_taps(w, h, pl.at.levels) };
    }
    return RTW_OK;
}
