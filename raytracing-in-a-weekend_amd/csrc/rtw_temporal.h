// rtw_temporal.h -- temporal accumulation of frames by reprojection (include/rtw.h "temporal accumulation"): the rule of one
// pixel as ONE __host__ __device__ definition.  The host form (rtw_temporal.cpp) and the kernel (rtw_temporal.hip) run these with the same
// plan, formed once per call on the host by temporal_check, so the device writes the host form's bytes: f32, one rounding per written
// operation under -ffp-contract=off, dot products as (x*x' + y*y') + z*z', the four taps in the order (x0, y0), (x0+1, y0), (x0, y0+1),
// (x0+1, y0+1).
// With moving objects (rtw.h "temporal accumulation with moving objects") the same definition is instantiated a second time,
// temporal_pixel_t<true>: a pixel whose object has a row in the caller's table carries its world point into the previous frame first
// (temporal_row, temporal_project_row) and takes the four taps; every other pixel runs the code of temporal_pixel_t<false>.
// With per-pixel motion (rtw.h "temporal accumulation with per-pixel motion") a third time, temporal_pixel_t<true, true>: a pixel
// whose prev_point is not NaN projects that point (temporal_project_point) and takes the four taps; every other pixel runs the code above.
// With bounds on the history (rtw.h "bounded temporal accumulation") a fourth time, temporal_pixel_t<true, true, true>: the
// history's colour is clipped to the caller's box before it is blended; everything else is the code above.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw_pixel_ray.h"
#include "rtw.h"

namespace rtw {

constexpr int TEMPORAL_DEPTH = 1, TEMPORAL_NORMAL = 2, TEMPORAL_IDX = 4;               // the terms that are on

// What every pixel of a call shares: checked and derived once by temporal_check (rtw_temporal.cpp).
struct TemporalPlan {
    uint32_t w = 0, h = 0;
    int terms = 0;
    int has_prev = 0;                // 0: the first frame, every pixel is without a history
    int is_static = 0;               // cam and prev_cam agree byte for byte in origin, pixel00, delta_u, delta_v: fx = i, fy = j, s = depth[p]
    float alpha = 0.0f, alpha_moments = 0.0f, max_history = 1.0f, depth_tol = 0.0f, normal_cos = 0.0f, ox = 0.0f, oy = 0.0f;
    RtwCamera cam = {};              // the current camera: pixel_ray_dir reads it
    float po[3] = {};                // prev_cam.origin
    float n[3] = {}, a[3] = {}, b[3] = {};     // n = du x dv, a = dv x n, b = n x du of prev_cam
    float pn = 0.0f, pa = 0.0f, pb = 0.0f, ua = 0.0f, vb = 0.0f;     // p00.n, p00.a, p00.b, du.a, dv.b
};

// The buffers of a call (include/rtw.h): the current frame, the previous call's outputs and guides, this call's outputs.
struct TemporalFrame { const float *cur, *depth, *normal; const int32_t *idx; };
struct TemporalHistory { const float *color, *moments, *len, *depth, *normal; const int32_t *idx; };
struct TemporalOut { float *color, *moments, *len, *variance; };
// What the calls with motion add (include/rtw.h "temporal accumulation with moving objects"): the table (rows null: none) and prev_xy (may be null)
struct TemporalMotion { const RtwMotionRow *rows; uint32_t n_rows, first; float *prev_xy; };
// What the calls with per-pixel motion add: each pixel's previous world point (null: none) and the normal it had there (null: normal[p])
struct TemporalPoints { const float *point, *normal; };
// What the bounded calls add: the box each pixel's history colour is clipped to (both null: none) and how far it was moved (may be null)
struct TemporalBounds { const float *lo, *hi; float *clipped; };

// What the counted taps add up to.
struct TemporalSum { float w, c0, c1, c2, m1, m2, len; };

__host__ __device__ inline float temporal_dot(const float *x, const float *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
__host__ __device__ inline void temporal_cross(const float *x, const float *y, float *o) {
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}
__host__ __device__ inline bool temporal_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // (false for NaN)

// Where pixel (i, j) of the current view, at depth `depth`, lay in the previous view: the tap position (fx, fy) in pixel units and s, the t
// the previous depth buffer holds for a ray through (fx, fy) that meets the same world point.  false: no history (behind the previous
// camera, outside its frame by a pixel or more, or a NaN anywhere -- every comparison is false for NaN).
__host__ __device__ inline bool temporal_project(const TemporalPlan &pl, uint32_t i, uint32_t j, float depth, float &fx, float &fy, float &s) {
    if (pl.is_static) {
        fx = (float)i; fy = (float)j; s = depth;
    } else {
        float dir[3];
        pixel_ray_dir(pl.cam, i, j, pl.ox, pl.oy, dir[0], dir[1], dir[2]);
        float d[3];
        for (int k = 0; k < 3; k++) {
            const float P = pl.cam.origin[k] + dir[k] * depth;
            d[k] = P - pl.po[k];
        }
        s = temporal_dot(d, pl.n) / pl.pn;
        fx = ((temporal_dot(d, pl.a) / s - pl.pa) / pl.ua) - pl.ox;
        fy = ((temporal_dot(d, pl.b) / s - pl.pb) / pl.vb) - pl.oy;
    }
    return s > 0.0f && fx > -1.0f && fx < (float)pl.w && fy > -1.0f && fy < (float)pl.h;
}

// The row of the object `id`, or null: k = id - first without wrap-around, 0 <= k < n_rows, rows[k].moving != 0.  No address is formed
// from any other id.
__host__ __device__ inline const RtwMotionRow *temporal_row(const TemporalMotion &mo, int32_t id) {
    const int64_t k = (int64_t)id - (int64_t)mo.first;
    if (k < 0 || k >= (int64_t)mo.n_rows) return nullptr;
    const RtwMotionRow *r = mo.rows + k;
    return r->moving != 0u ? r : nullptr;
}

// temporal_project for a pixel of a moving object: its world point is carried into the previous frame by the row before it is projected,
// under a static camera too.  A NaN in the row ends as an s or fx that is NaN: false.
__host__ __device__ inline bool temporal_project_row(const TemporalPlan &pl, const RtwMotionRow &r, uint32_t i, uint32_t j, float depth, float &fx,
                                                     float &fy, float &s) {
    float dir[3];
    pixel_ray_dir(pl.cam, i, j, pl.ox, pl.oy, dir[0], dir[1], dir[2]);
    float e[3], d[3];
    for (int k = 0; k < 3; k++) {
        const float P = pl.cam.origin[k] + dir[k] * depth;
        e[k] = P - r.from[k];
    }
    for (int k = 0; k < 3; k++) {
        const float Pp = ((r.a[3 * k] * e[0] + r.a[3 * k + 1] * e[1]) + r.a[3 * k + 2] * e[2]) + r.to[k];
        d[k] = Pp - pl.po[k];
    }
    s = temporal_dot(d, pl.n) / pl.pn;
    fx = ((temporal_dot(d, pl.a) / s - pl.pa) / pl.ua) - pl.ox;
    fy = ((temporal_dot(d, pl.b) / s - pl.pb) / pl.vb) - pl.oy;
    return s > 0.0f && fx > -1.0f && fx < (float)pl.w && fy > -1.0f && fy < (float)pl.h;
}

// temporal_project for a pixel that brings its previous world point P' along: d = P' - prev_cam.origin, then s, fx, fy as for a row.  An
// infinity or a NaN in P' ends as an s or fx that is not finite or not in the box: false, never an index.
__host__ __device__ inline bool temporal_project_point(const TemporalPlan &pl, const float *Pp, float &fx, float &fy, float &s) {
    float d[3];
    for (int k = 0; k < 3; k++) d[k] = Pp[k] - pl.po[k];
    s = temporal_dot(d, pl.n) / pl.pn;
    fx = ((temporal_dot(d, pl.a) / s - pl.pa) / pl.ua) - pl.ox;
    fy = ((temporal_dot(d, pl.b) / s - pl.pb) / pl.vb) - pl.oy;
    return s > 0.0f && fx > -1.0f && fx < (float)pl.w && fy > -1.0f && fy < (float)pl.h;
}

// Does previous pixel q (inside the frame) count as history for a centre with normal `np`, object `id` and reprojected depth s?
__host__ __device__ inline bool temporal_tap_ok(const TemporalPlan &pl, const TemporalHistory &hs, size_t q, float s, const float *np, int32_t id) {
    if (!(hs.len[q] > 0.0f)) return false;                                               // (a hole: 0, or NaN)
    if (pl.terms & TEMPORAL_DEPTH) {
        if (!(__builtin_fabsf(hs.depth[q] - s) <= pl.depth_tol * s)) return false;
    }
    if (pl.terms & TEMPORAL_NORMAL) {
        if (!(temporal_dot(np, hs.normal + 3 * q) >= pl.normal_cos)) return false;
    }
    if ((pl.terms & TEMPORAL_IDX) && hs.idx[q] != id) return false;
    return true;
}

// One tap: skipped outside the frame, when it fails a term, and when its weight is not > 0 (the a-trous filter's rule, rtw_atrous.h: for
// finite values no bit changes, and a tap of weight 0 cannot enter as 0 * NaN).
__host__ __device__ inline void temporal_tap(const TemporalPlan &pl, const TemporalHistory &hs, int qx, int qy, float wt, float s, const float *np,
                                             int32_t id, TemporalSum &t) {
    if (qx < 0 || qy < 0 || qx >= (int)pl.w || qy >= (int)pl.h) return;
    const size_t q = (size_t)qy * pl.w + (size_t)qx;
    if (!temporal_tap_ok(pl, hs, q, s, np, id)) return;
    if (wt > 0.0f) {
        t.w = t.w + wt;
        t.c0 = t.c0 + wt * hs.color[3 * q];
        t.c1 = t.c1 + wt * hs.color[3 * q + 1];
        t.c2 = t.c2 + wt * hs.color[3 * q + 2];
        t.m1 = t.m1 + wt * hs.moments[2 * q];
        t.m2 = t.m2 + wt * hs.moments[2 * q + 1];
        t.len = t.len + wt * hs.len[q];
    }
}

// 1 / n_, raised to `floor_` when below it
__host__ __device__ inline float temporal_blend_factor(float n_, float floor_) {
    const float a_ = 1.0f / n_;
    return a_ < floor_ ? floor_ : a_;
}

// Pixel (i, j).  o.color may be f.cur: the pixel's own cur is read before anything is written.  MOTION: the calls with a table of rows or
// prev_xy; false compiles to the rule without them (`mo` is not read), which is what rtw_temporal_accumulate and its kernel run.  POINTS
// (only with MOTION): the calls with prev_point; false compiles to the rule without it (`pt` is not read).  BOUNDS (only with POINTS): the
// bounded calls; false compiles to the rule without them (`bd` is not read).
template <bool MOTION, bool POINTS = false, bool BOUNDS = false>
__host__ __device__ inline void temporal_pixel_t(const TemporalPlan &pl, const TemporalFrame &f, const TemporalHistory &hs, const TemporalOut &o,
                                                 const TemporalMotion &mo, const TemporalPoints &pt, uint32_t i, uint32_t j,
                                                 const TemporalBounds &bd = TemporalBounds{ nullptr, nullptr, nullptr }) {
    const size_t p = (size_t)j * pl.w + (size_t)i;
    const float r = f.cur[3 * p], g = f.cur[3 * p + 1], b = f.cur[3 * p + 2];
    const float L = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    const bool fin = temporal_finite(r) && temporal_finite(g) && temporal_finite(b);

    TemporalSum t = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    float fx, fy, s;
    const RtwMotionRow *row = nullptr;
    bool cand = false, has_pt = false;
    if (pl.has_prev) {
        float Pp[3] = { 0.0f, 0.0f, 0.0f };
        if (POINTS && pt.point) {
            Pp[0] = pt.point[3 * p]; Pp[1] = pt.point[3 * p + 1]; Pp[2] = pt.point[3 * p + 2];
            has_pt = Pp[0] == Pp[0];                                                     // (a NaN in x: the pixel has no point; its row, if any, counts)
        }
        if (POINTS && has_pt) cand = temporal_project_point(pl, Pp, fx, fy, s);
        else {
            if (MOTION && mo.rows) row = temporal_row(mo, f.idx[p]);
            cand = (MOTION && row) ? temporal_project_row(pl, *row, i, j, f.depth[p], fx, fy, s) : temporal_project(pl, i, j, f.depth[p], fx, fy, s);
        }
    }
    if (MOTION && mo.prev_xy) {
        mo.prev_xy[2 * p] = pl.has_prev ? fx : __builtin_nanf("");
        mo.prev_xy[2 * p + 1] = pl.has_prev ? fy : __builtin_nanf("");
    }
    if (cand) {
        float np[3] = { 0.0f, 0.0f, 0.0f };
        if (pl.terms & TEMPORAL_NORMAL) {
            const float *nr = (POINTS && has_pt && pt.normal) ? pt.normal : f.normal;
            np[0] = nr[3 * p]; np[1] = nr[3 * p + 1]; np[2] = nr[3 * p + 2];
            if (MOTION && row) {
                const float n0 = np[0], n1 = np[1], n2 = np[2];
                for (int k = 0; k < 3; k++) np[k] = (row->nrm[3 * k] * n0 + row->nrm[3 * k + 1] * n1) + row->nrm[3 * k + 2] * n2;
            }
        }
        const int32_t id = (pl.terms & TEMPORAL_IDX) ? f.idx[p] : 0;
        if (pl.is_static && !(MOTION && row) && !(POINTS && has_pt)) {
            temporal_tap(pl, hs, (int)i, (int)j, 1.0f, s, np, id, t);                  // wx = wy = 0: the other three weigh 0
        } else {
            const float xf = __builtin_floorf(fx), yf = __builtin_floorf(fy);
            const float wx = fx - xf, wy = fy - yf;
            const int x0 = (int)xf, y0 = (int)yf;                                      // -1 .. w - 1, -1 .. h - 1
            const float ux = 1.0f - wx, uy = 1.0f - wy;
            temporal_tap(pl, hs, x0, y0, ux * uy, s, np, id, t);
            temporal_tap(pl, hs, x0 + 1, y0, wx * uy, s, np, id, t);
            temporal_tap(pl, hs, x0, y0 + 1, ux * wy, s, np, id, t);
            temporal_tap(pl, hs, x0 + 1, y0 + 1, wx * wy, s, np, id, t);
        }
    }

    float c0 = r, c1 = g, c2 = b, m1, m2, len, clipped = 0.0f;
    if (t.w > 0.0f) {
        float h0 = t.c0 / t.w, h1 = t.c1 / t.w, h2 = t.c2 / t.w;
        const float hm1 = t.m1 / t.w, hm2 = t.m2 / t.w, hlen = t.len / t.w;
        if (BOUNDS && bd.lo) {                                                           // (a pixel without a history does not read its box)
            const float u0 = h0, u1 = h1, u2 = h2;
            const float *lo = bd.lo + 3 * p, *hi = bd.hi + 3 * p;
            h0 = h0 < lo[0] ? lo[0] : (h0 > hi[0] ? hi[0] : h0);
            h1 = h1 < lo[1] ? lo[1] : (h1 > hi[1] ? hi[1] : h1);
            h2 = h2 < lo[2] ? lo[2] : (h2 > hi[2] ? hi[2] : h2);
            clipped = (__builtin_fabsf(u0 - h0) + __builtin_fabsf(u1 - h1)) + __builtin_fabsf(u2 - h2);
        }
        if (fin) {
            const float n1 = hlen + 1.0f;
            const float n_ = n1 < pl.max_history ? n1 : pl.max_history;
            const float a_ = temporal_blend_factor(n_, pl.alpha), am_ = temporal_blend_factor(n_, pl.alpha_moments);
            c0 = h0 + (r - h0) * a_;
            c1 = h1 + (g - h1) * a_;
            c2 = h2 + (b - h2) * a_;
            m1 = hm1 + (L - hm1) * am_;
            m2 = hm2 + (L * L - hm2) * am_;
            len = n_;
        } else {                                                                         // one bad sample does not enter
            c0 = h0; c1 = h1; c2 = h2; m1 = hm1; m2 = hm2; len = hlen;
        }
    } else if (fin) {
        m1 = L; m2 = L * L; len = 1.0f;
    } else {                                                                             // len 0: no later frame reads this pixel as history
        m1 = 0.0f; m2 = 0.0f; len = 0.0f;
    }
    o.color[3 * p] = c0; o.color[3 * p + 1] = c1; o.color[3 * p + 2] = c2;
    o.moments[2 * p] = m1; o.moments[2 * p + 1] = m2;
    o.len[p] = len;
    if (BOUNDS && bd.clipped) bd.clipped[p] = clipped;
    if (o.variance) {
        const float v = m2 - m1 * m1;
        o.variance[p] = v > 0.0f ? v : 0.0f;
    }
}
__host__ __device__ inline void temporal_pixel(const TemporalPlan &pl, const TemporalFrame &f, const TemporalHistory &hs, const TemporalOut &o,
                                               uint32_t i, uint32_t j) {
    temporal_pixel_t<false>(pl, f, hs, o, TemporalMotion{ nullptr, 0u, 0u, nullptr }, TemporalPoints{ nullptr, nullptr }, i, j);
}

// Everything rtw_temporal_accumulate refuses (rtw.h); fills `pl`.  RTW_OK or RTW_E_INVALID.  (rtw_temporal.cpp)
int temporal_check(const float *cur, uint32_t w, uint32_t h, const RtwCamera *cam, const float *depth, const float *normal, const int32_t *idx,
                   const RtwCamera *prev_cam, const float *prev_color, const float *prev_moments, const float *prev_len, const float *prev_depth,
                   const float *prev_normal, const int32_t *prev_idx, const RtwTemporal *p, const float *out_color, const float *out_moments,
                   const float *out_len, TemporalPlan &pl);
// ... and what the calls with motion refuse besides (rtw.h "temporal accumulation with moving objects")
int temporal_check_motion(const int32_t *idx, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first, const float *out_color,
                          const float *out_moments, const float *out_len, const float *out_variance, const float *out_prev_xy);
// ... and the calls with per-pixel motion (rtw.h "temporal accumulation with per-pixel motion")
int temporal_check_points(const float *prev_point, const float *carried_normal, const float *out_color, const float *out_moments, const float *out_len,
                          const float *out_variance, const float *out_prev_xy);
// ... and the bounded calls (rtw.h "bounded temporal accumulation")
int temporal_check_bounds(const float *hist_lo, const float *hist_hi, const float *out_clipped, const float *out_color, const float *out_moments,
                          const float *out_len, const float *out_variance, const float *out_prev_xy);

} // namespace rtw
