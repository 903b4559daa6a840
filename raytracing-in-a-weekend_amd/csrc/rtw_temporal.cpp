// rtw_temporal.cpp -- the host forms of the temporal accumulation (rtw_temporal_accumulate, _motion, _points, include/rtw.h) and the argument checks and
// plan it shares with the device path (rtw_temporal.hip).  Pure host code: no HIP call.  One thread over the pixels, each running
// temporal_pixel (rtw_temporal.h), which the kernel runs too.
#include "rtw_temporal.h"

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>

namespace rtw {

int temporal_check(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal, const int32_t *idx,
                   const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments, const float *prev_len, const float *prev_depth,
                   const float *prev_normal, const int32_t *prev_idx, const RtwTemporal *p, const float *out_color, const float *out_moments,
                   const float *out_len, TemporalPlan &pl) {
    if (!cur || !cam || !depth || !p || !out_color || !out_moments || !out_len) return RTW_E_INVALID;
    if (w == 0 || h == 0 || w > RTW_TEMPORAL_MAX_SIDE || h > RTW_TEMPORAL_MAX_SIDE || (uint64_t)w * h > 0xFFFFFFFFull) return RTW_E_INVALID;
    const int n_prev = (prev_cam != nullptr) + (prev_color != nullptr) + (prev_moments != nullptr) + (prev_len != nullptr);
    if (n_prev != 0 && n_prev != 4) return RTW_E_INVALID;
    if (n_prev == 0 && (prev_depth || prev_normal || prev_idx)) return RTW_E_INVALID;     // (guides of a history that is not there)
    if (!(p->alpha >= 0.0f && p->alpha <= 1.0f) || !(p->alpha_moments >= 0.0f && p->alpha_moments <= 1.0f)) return RTW_E_INVALID;
    if (p->max_history < 1 || p->max_history > 65535) return RTW_E_INVALID;
    if (!(p->depth_tol >= 0.0f) || !std::isfinite(p->depth_tol)) return RTW_E_INVALID;
    if (!(p->normal_cos >= 0.0f && p->normal_cos <= 1.0f)) return RTW_E_INVALID;
    if (p->same_object > 1) return RTW_E_INVALID;
    if (!std::isfinite(p->offset[0]) || !std::isfinite(p->offset[1])) return RTW_E_INVALID;
    if (out_color == prev_color || out_moments == prev_moments || out_len == prev_len) return RTW_E_INVALID;     // neighbours gather from prev_*
    pl = TemporalPlan();
    pl.w = w; pl.h = h;
    pl.has_prev = n_prev == 4;
    pl.alpha = p->alpha; pl.alpha_moments = p->alpha_moments; pl.max_history = (float)p->max_history;
    pl.depth_tol = p->depth_tol; pl.normal_cos = p->normal_cos;
    pl.ox = p->offset[0]; pl.oy = p->offset[1];
    pl.cam = *cam;
    if (p->depth_tol > 0.0f) {
        if (pl.has_prev && !prev_depth) return RTW_E_INVALID;
        pl.terms |= TEMPORAL_DEPTH;
    }
    if (p->normal_cos > 0.0f) {
        if (!normal || (pl.has_prev && !prev_normal)) return RTW_E_INVALID;
        pl.terms |= TEMPORAL_NORMAL;
    }
    if (p->same_object) {
        if (!idx || (pl.has_prev && !prev_idx)) return RTW_E_INVALID;
        pl.terms |= TEMPORAL_IDX;
    }
    if (pl.has_prev) {
        const float *p00 = prev_cam->pixel00, *du = prev_cam->delta_u, *dv = prev_cam->delta_v;
        temporal_cross(du, dv, pl.n);
        temporal_cross(dv, pl.n, pl.a);
        temporal_cross(pl.n, du, pl.b);
        pl.pn = temporal_dot(p00, pl.n); pl.pa = temporal_dot(p00, pl.a); pl.pb = temporal_dot(p00, pl.b);
        pl.ua = temporal_dot(du, pl.a); pl.vb = temporal_dot(dv, pl.b);
        for (float v : { pl.pn, pl.ua, pl.vb })
            if (v == 0.0f || !std::isfinite(v)) return RTW_E_INVALID;
        for (int k = 0; k < 3; k++) pl.po[k] = prev_cam->origin[k];
        pl.is_static = !std::memcmp(cam->origin, prev_cam->origin, sizeof cam->origin) &&
                       !std::memcmp(cam->pixel00, prev_cam->pixel00, sizeof cam->pixel00) &&
                       !std::memcmp(cam->delta_u, prev_cam->delta_u, sizeof cam->delta_u) &&
                       !std::memcmp(cam->delta_v, prev_cam->delta_v, sizeof cam->delta_v);
    }
    return RTW_OK;
}

int temporal_check_motion(const int32_t *idx, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first, const float *out_color,
                          const float *out_moments, const float *out_len, const float *out_variance, const float *out_prev_xy) {
    if (rows && (!idx || n_rows == 0 || (uint64_t)first + n_rows > 0x80000000ull)) return RTW_E_INVALID;
    if (out_prev_xy && (out_prev_xy == out_color || out_prev_xy == out_moments || out_prev_xy == out_len || out_prev_xy == out_variance))
        return RTW_E_INVALID;
    return RTW_OK;
}

int temporal_check_points(const float *prev_point, const float *carried_normal, const float *out_color, const float *out_moments, const float *out_len,
                          const float *out_variance, const float *out_prev_xy) {
    if (carried_normal && !prev_point) return RTW_E_INVALID;
    for (const float *in : { prev_point, carried_normal })
        for (const float *out : { out_color, out_moments, out_len, out_variance, out_prev_xy })
            if (in && in == out) return RTW_E_INVALID;
    return RTW_OK;
}

int temporal_check_bounds(const float *hist_lo, const float *hist_hi, const float *out_clipped, const float *out_color, const float *out_moments,
                          const float *out_len, const float *out_variance, const float *out_prev_xy) {
    if ((hist_lo != nullptr) != (hist_hi != nullptr)) return RTW_E_INVALID;              // both or neither
    for (const float *b : { hist_lo, hist_hi, out_clipped })
        for (const float *out : { out_color, out_moments, out_len, out_variance, out_prev_xy })
            if (b && b == out) return RTW_E_INVALID;
    if (out_clipped && (out_clipped == hist_lo || out_clipped == hist_hi)) return RTW_E_INVALID;
    return RTW_OK;
}

} // namespace rtw

using namespace rtw;

static_assert(sizeof(RtwTemporal) == 32 && sizeof(RtwMotionRow) == 128, "POD layout");

extern "C" int rtw_temporal_accumulate(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                       const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                       const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                       const RtwTemporal *params, float *out_color, float *out_moments, float *out_len, float *out_variance,
                                       RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    TemporalPlan pl;
    const int rc = temporal_check(cur, w, h, cam, depth, normal, idx, prev_cam, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                                  params, out_color, out_moments, out_len, pl);
    if (rc != RTW_OK) return rc;
    const TemporalFrame f = { cur, depth, normal, idx };
    const TemporalHistory hs = { prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx };
    const TemporalOut o = { out_color, out_moments, out_len, out_variance };
    for (uint32_t j = 0; j < h; j++)
        for (uint32_t i = 0; i < w; i++) temporal_pixel(pl, f, hs, o, i, j);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, 4ull * w * h };
    }
    return RTW_OK;
}

extern "C" int rtw_temporal_accumulate_motion(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                              const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                              const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                              const RtwTemporal *params, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first, float *out_color,
                                              float *out_moments, float *out_len, float *out_variance, float *out_prev_xy, RtwFilterStats *stats) {
    if (!rows && !out_prev_xy)
        return rtw_temporal_accumulate(cur, w, h, cam, depth, normal, idx, prev_cam, prev_color, prev_moments, prev_len, prev_depth, prev_normal,
                                       prev_idx, params, out_color, out_moments, out_len, out_variance, stats);
    const auto t0 = std::chrono::steady_clock::now();
    TemporalPlan pl;
    int rc = temporal_check(cur, w, h, cam, depth, normal, idx, prev_cam, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                            params, out_color, out_moments, out_len, pl);
    if (rc == RTW_OK) rc = temporal_check_motion(idx, rows, n_rows, first, out_color, out_moments, out_len, out_variance, out_prev_xy);
    if (rc != RTW_OK) return rc;
    const TemporalFrame f = { cur, depth, normal, idx };
    const TemporalHistory hs = { prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx };
    const TemporalOut o = { out_color, out_moments, out_len, out_variance };
    const TemporalMotion mo = { rows, n_rows, first, out_prev_xy };
    for (uint32_t j = 0; j < h; j++)
        for (uint32_t i = 0; i < w; i++) temporal_pixel_t<true>(pl, f, hs, o, mo, TemporalPoints{ nullptr, nullptr }, i, j);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, 4ull * w * h };
    }
    return RTW_OK;
}

extern "C" int rtw_temporal_accumulate_points(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                              const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                              const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                              const RtwTemporal *params, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first,
                                              const float *prev_point, const float *carried_normal, float *out_color, float *out_moments,
                                              float *out_len, float *out_variance, float *out_prev_xy, RtwFilterStats *stats) {
    if (!prev_point && !carried_normal)
        return rtw_temporal_accumulate_motion(cur, w, h, cam, depth, normal, idx, prev_cam, prev_color, prev_moments, prev_len, prev_depth,
                                              prev_normal, prev_idx, params, rows, n_rows, first, out_color, out_moments, out_len, out_variance,
                                              out_prev_xy, stats);
    const auto t0 = std::chrono::steady_clock::now();
    TemporalPlan pl;
    int rc = temporal_check(cur, w, h, cam, depth, normal, idx, prev_cam, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                            params, out_color, out_moments, out_len, pl);
    if (rc == RTW_OK) rc = temporal_check_motion(idx, rows, n_rows, first, out_color, out_moments, out_len, out_variance, out_prev_xy);
    if (rc == RTW_OK) rc = temporal_check_points(prev_point, carried_normal, out_color, out_moments, out_len, out_variance, out_prev_xy);
    if (rc != RTW_OK) return rc;
    const TemporalFrame f = { cur, depth, normal, idx };
    const TemporalHistory hs = { prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx };
    const TemporalOut o = { out_color, out_moments, out_len, out_variance };
    const TemporalMotion mo = { rows, n_rows, first, out_prev_xy };
    const TemporalPoints pt = { prev_point, carried_normal };
    for (uint32_t j = 0; j < h; j++)
        for (uint32_t i = 0; i < w; i++) temporal_pixel_t<true, true>(pl, f, hs, o, mo, pt, i, j);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, 4ull * w * h };
    }
    return RTW_OK;
}

extern "C" int rtw_temporal_accumulate_bounded(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal,
                                               const int32_t *idx, const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments,
                                               const float *prev_len, const float *prev_depth, const float *prev_normal, const int32_t *prev_idx,
                                               const RtwTemporal *params, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first,
                                               const float *prev_point, const float *carried_normal, const float *hist_lo, const float *hist_hi,
                                               float *out_color, float *out_moments, float *out_len, float *out_variance, float *out_prev_xy,
                                               float *out_clipped, RtwFilterStats *stats) {
    if (!hist_lo && !hist_hi && !out_clipped)
        return rtw_temporal_accumulate_points(cur, w, h, cam, depth, normal, idx, prev_cam, prev_color, prev_moments, prev_len, prev_depth,
                                              prev_normal, prev_idx, params, rows, n_rows, first, prev_point, carried_normal, out_color,
                                              out_moments, out_len, out_variance, out_prev_xy, stats);
    const auto t0 = std::chrono::steady_clock::now();
    TemporalPlan pl;
    int rc = temporal_check(cur, w, h, cam, depth, normal, idx, prev_cam, prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx,
                            params, out_color, out_moments, out_len, pl);
    if (rc == RTW_OK) rc = temporal_check_motion(idx, rows, n_rows, first, out_color, out_moments, out_len, out_variance, out_prev_xy);
    if (rc == RTW_OK) rc = temporal_check_points(prev_point, carried_normal, out_color, out_moments, out_len, out_variance, out_prev_xy);
    if (rc == RTW_OK) rc = temporal_check_bounds(hist_lo, hist_hi, out_clipped, out_color, out_moments, out_len, out_variance, out_prev_xy);
    if (rc != RTW_OK) return rc;
    const TemporalFrame f = { cur, depth, normal, idx };
    const TemporalHistory hs = { prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx };
    const TemporalOut o = { out_color, out_moments, out_len, out_variance };
    const TemporalMotion mo = { rows, rows ? n_rows : 0u, rows ? first : 0u, out_prev_xy };
    const TemporalPoints pt = { prev_point, carried_normal };
    const TemporalBounds bd = { hist_lo, hist_hi, out_clipped };
    for (uint32_t j = 0; j < h; j++)
        for (uint32_t i = 0; i < w; i++) temporal_pixel_t<true, true, true>(pl, f, hs, o, mo, pt, i, j, bd);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, 4ull * w * h };
    }
    return RTW_OK;
}
