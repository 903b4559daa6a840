// rtw_temporal.hip -- temporal accumulation by reprojection (rtw_temporal.h) on the GPU: the device path of
// rtw_ctx_temporal_accumulate, rtw_ctx_temporal_accumulate_motion, rtw_ctx_temporal_accumulate_points (8g) and
// rtw_ctx_temporal_accumulate_bounded (8h).
//
// One launch, one thread per pixel running temporal_pixel -- the host form's definition with the host form's plan, so its bytes.
// Workgroup b covers the 32 x 8 pixels of tile (b % tiles_x, b / tiles_x): a wave is two rows of 32 pixels, so its loads of cur and of the
// guides, and under a small camera move its four taps, fall on a few consecutive cache lines.  The taps are plain global loads: each
// previous pixel is read by about four threads, all of them neighbours, and the reuse is the caches'.  With a static camera
// (TemporalPlan.is_static, a launch-uniform branch) a thread reads the one tap under it.  Results go straight into the caller's buffers
// when those are device memory; host buffers are staged.
#include "rtw_temporal_dev.h"
#include "rtw_temporal.h"
#include "rtw_devmem.h"

#include <chrono>
#include <new>

namespace rtw {
namespace {

constexpr uint32_t TBX = 32, TBY = 8;                    // workgroup: 32 x 8 pixels, a wave covers two rows of 32

// (f.cur and o.color may be the same buffer: no __restrict__ here)
__global__ void __launch_bounds__(TBX * TBY) temporal_kernel(TemporalPlan pl, uint32_t tiles_x, TemporalFrame f, TemporalHistory hs, TemporalOut o) {
    const uint32_t x = (blockIdx.x % tiles_x) * TBX + threadIdx.x % TBX;
    const uint32_t y = (blockIdx.x / tiles_x) * TBY + threadIdx.x / TBX;
    if (x < pl.w && y < pl.h) temporal_pixel(pl, f, hs, o, x, y);
}

// The same with a table of motion rows and / or prev_xy (rtw_ctx_temporal_accumulate_motion): a second instantiation, chosen on the host, so
// that the kernel above stays what it is.  A pixel of a moving object loads its row (128 bytes, the same for every lane on the object) and
// takes the four taps; the others run the code above.
__global__ void __launch_bounds__(TBX * TBY) temporal_motion_kernel(TemporalPlan pl, uint32_t tiles_x, TemporalFrame f, TemporalHistory hs, TemporalOut o,
                                                                    TemporalMotion mo) {
    const uint32_t x = (blockIdx.x % tiles_x) * TBX + threadIdx.x % TBX;
    const uint32_t y = (blockIdx.x / tiles_x) * TBY + threadIdx.x / TBX;
    if (x < pl.w && y < pl.h) temporal_pixel_t<true>(pl, f, hs, o, mo, TemporalPoints{ nullptr, nullptr }, x, y);
}

// ... and with per-pixel previous points (rtw_ctx_temporal_accumulate_points): a third instantiation, chosen on the host likewise.  A pixel
// with a point loads its 12 bytes (and the 12 of its carried normal) beside cur and takes the four taps; the others run the code above.
__global__ void __launch_bounds__(TBX * TBY) temporal_points_kernel(TemporalPlan pl, uint32_t tiles_x, TemporalFrame f, TemporalHistory hs, TemporalOut o,
                                                                    TemporalMotion mo, TemporalPoints pt) {
    const uint32_t x = (blockIdx.x % tiles_x) * TBX + threadIdx.x % TBX;
    const uint32_t y = (blockIdx.x / tiles_x) * TBY + threadIdx.x / TBX;
    if (x < pl.w && y < pl.h) temporal_pixel_t<true, true>(pl, f, hs, o, mo, pt, x, y);
}

// ... and with bounds on the history's colour (rtw_ctx_temporal_accumulate_bounded): a fourth instantiation, chosen on the host likewise.  A
// pixel with a history loads its box (24 bytes) beside cur and writes how far the box moved its history (4 bytes); the others run the code
// above.
__global__ void __launch_bounds__(TBX * TBY) temporal_bounded_kernel(TemporalPlan pl, uint32_t tiles_x, TemporalFrame f, TemporalHistory hs, TemporalOut o,
                                                                     TemporalMotion mo, TemporalPoints pt, TemporalBounds bd) {
    const uint32_t x = (blockIdx.x % tiles_x) * TBX + threadIdx.x % TBX;
    const uint32_t y = (blockIdx.x / tiles_x) * TBY + threadIdx.x / TBX;
    if (x < pl.w && y < pl.h) temporal_pixel_t<true, true, true>(pl, f, hs, o, mo, pt, x, y, bd);
}

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

} // namespace

struct TemporalScratch {
    DevMem cur, depth, normal, idx;                                      // the caller's host buffers, staged
    DevMem prev_color, prev_moments, prev_len, prev_depth, prev_normal, prev_idx;
    DevMem out_color, out_moments, out_len, out_variance;                // a result whose buffer is host memory
    DevMem rows, out_prev_xy;                                            // (the calls with motion)
    DevMem point, carried;                                               // (the calls with per-pixel motion)
    DevMem hist_lo, hist_hi, out_clipped;                                // (the bounded calls)
    hipEvent_t ev[2] = { nullptr, nullptr };
};

void temporal_scratch_free(TemporalScratch *s) {
    if (!s) return;
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;                                      // (the buffers free themselves)
}

#define TEMPORAL_TRY(expr)                                                                                                        \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; } \
    } while (0)

int temporal_accumulate_device(int device, hipStream_t stream, TemporalScratch **scratch, uint32_t w, uint32_t h, const RtwCamera *cam,
                               const RtwCamera *prev_cam, const TemporalBuffers &b, const RtwTemporal *p, const TemporalMotion *m, const TemporalPoints *pts,
                               const TemporalBounds *bds, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    TemporalPlan pl;
    const int rc = temporal_check(b.cur, w, h, cam, b.depth, b.normal, b.idx, prev_cam, b.prev_color, b.prev_moments, b.prev_len, b.prev_depth,
                                  b.prev_normal, b.prev_idx, p, b.out_color, b.out_moments, b.out_len, pl);
    if (rc != RTW_OK) return rc;
    TemporalMotion mo = { nullptr, 0u, 0u, nullptr };
    if (m && (m->rows || m->prev_xy)) {
        const int rm = temporal_check_motion(b.idx, m->rows, m->n_rows, m->first, b.out_color, b.out_moments, b.out_len, b.out_variance, m->prev_xy);
        if (rm != RTW_OK) return rm;
        mo = *m;
        if (!mo.rows) mo.n_rows = mo.first = 0u;
    }
    TemporalPoints pt = { nullptr, nullptr };
    if (pts && (pts->point || pts->normal)) {
        const int rp = temporal_check_points(pts->point, pts->normal, b.out_color, b.out_moments, b.out_len, b.out_variance, mo.prev_xy);
        if (rp != RTW_OK) return rp;
        pt = *pts;
        if (!(pl.terms & TEMPORAL_NORMAL)) pt.normal = nullptr;                          // (read by the normal test only)
    }
    TemporalBounds bd = { nullptr, nullptr, nullptr };
    if (bds && (bds->lo || bds->hi || bds->clipped)) {
        const int rb = temporal_check_bounds(bds->lo, bds->hi, bds->clipped, b.out_color, b.out_moments, b.out_len, b.out_variance, mo.prev_xy);
        if (rb != RTW_OK) return rb;
        bd = *bds;
    }
    const bool motion = mo.rows || mo.prev_xy, bounded = bd.lo || bd.clipped;
    TEMPORAL_TRY(hipSetDevice(device));
    if (!*scratch) {
        TemporalScratch *s = new (std::nothrow) TemporalScratch();
        if (!s) return RTW_E_NOMEM;
        *scratch = s;
        for (hipEvent_t &e : s->ev) TEMPORAL_TRY(hipEventCreate(&e));
    }
    TemporalScratch *s = *scratch;
    const size_t n_px = (size_t)w * h, f1 = n_px * sizeof(float), f2 = 2 * f1, f3 = 3 * f1;

    // the caller's buffers on the device: a host one is staged; a guide whose term is off is not touched
    TemporalFrame f = { b.cur, b.depth, (pl.terms & TEMPORAL_NORMAL) ? b.normal : nullptr, ((pl.terms & TEMPORAL_IDX) || mo.rows) ? b.idx : nullptr };
    TemporalHistory hs = { b.prev_color, b.prev_moments, b.prev_len, (pl.terms & TEMPORAL_DEPTH) ? b.prev_depth : nullptr,
                           (pl.terms & TEMPORAL_NORMAL) ? b.prev_normal : nullptr, (pl.terms & TEMPORAL_IDX) ? b.prev_idx : nullptr };
    struct Stage { const void **p; DevMem *m; size_t bytes; };
    const Stage stages[15] = { { (const void **)&f.cur, &s->cur, f3 },
                               { (const void **)&f.depth, &s->depth, f1 },
                               { (const void **)&f.normal, &s->normal, f3 },
                               { (const void **)&f.idx, &s->idx, n_px * sizeof(int32_t) },
                               { (const void **)&hs.color, &s->prev_color, f3 },
                               { (const void **)&hs.moments, &s->prev_moments, f2 },
                               { (const void **)&hs.len, &s->prev_len, f1 },
                               { (const void **)&hs.depth, &s->prev_depth, f1 },
                               { (const void **)&hs.normal, &s->prev_normal, f3 },
                               { (const void **)&hs.idx, &s->prev_idx, n_px * sizeof(int32_t) },
                               { (const void **)&mo.rows, &s->rows, (size_t)mo.n_rows * sizeof(RtwMotionRow) },
                               { (const void **)&pt.point, &s->point, f3 },
                               { (const void **)&pt.normal, &s->carried, f3 },
                               { (const void **)&bd.lo, &s->hist_lo, f3 },
                               { (const void **)&bd.hi, &s->hist_hi, f3 } };
    for (const Stage &st : stages) {
        if (!*st.p || on_device(*st.p, device)) continue;
        TEMPORAL_TRY(st.m->reserve(st.bytes));
        TEMPORAL_TRY(hipMemcpyAsync(st.m->ptr, *st.p, st.bytes, hipMemcpyDefault, stream));
        *st.p = st.m->ptr;
    }
    TemporalOut o = { b.out_color, b.out_moments, b.out_len, b.out_variance };
    struct Result { float **p; float *host; DevMem *m; size_t bytes; };
    Result results[6] = { { &o.color, nullptr, &s->out_color, f3 },
                          { &o.moments, nullptr, &s->out_moments, f2 },
                          { &o.len, nullptr, &s->out_len, f1 },
                          { &o.variance, nullptr, &s->out_variance, f1 },
                          { &mo.prev_xy, nullptr, &s->out_prev_xy, f2 },
                          { &bd.clipped, nullptr, &s->out_clipped, f1 } };
    for (Result &r : results) {
        if (!*r.p || on_device(*r.p, device)) continue;
        TEMPORAL_TRY(r.m->reserve(r.bytes));
        r.host = *r.p;
        *r.p = r.m->as<float>();
    }

    const uint32_t tiles_x = (w + TBX - 1) / TBX, tiles_y = (h + TBY - 1) / TBY;
    TEMPORAL_TRY(hipEventRecord(s->ev[0], stream));
    const dim3 grid((unsigned)((uint64_t)tiles_x * tiles_y));
    if (bounded) hipLaunchKernelGGL(temporal_bounded_kernel, grid, dim3(TBX * TBY), 0, stream, pl, tiles_x, f, hs, o, mo, pt, bd);
    else if (pt.point) hipLaunchKernelGGL(temporal_points_kernel, grid, dim3(TBX * TBY), 0, stream, pl, tiles_x, f, hs, o, mo, pt);
    else if (motion) hipLaunchKernelGGL(temporal_motion_kernel, grid, dim3(TBX * TBY), 0, stream, pl, tiles_x, f, hs, o, mo);
    else hipLaunchKernelGGL(temporal_kernel, grid, dim3(TBX * TBY), 0, stream, pl, tiles_x, f, hs, o);
    TEMPORAL_TRY(hipGetLastError());
    TEMPORAL_TRY(hipEventRecord(s->ev[1], stream));
    for (const Result &r : results)
        if (r.host) TEMPORAL_TRY(hipMemcpyAsync(r.host, *r.p, r.bytes, hipMemcpyDefault, stream));
    TEMPORAL_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, 4ull * w * h };
    }
    return RTW_OK;
}
#undef TEMPORAL_TRY

} // namespace rtw
