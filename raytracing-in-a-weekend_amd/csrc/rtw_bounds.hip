// rtw_bounds.hip -- the neighbourhood colour bounds (rtw_bounds.h) on the GPU: the device path of rtw_ctx_colour_bounds.
//
// One launch, one thread per pixel running bounds_write -- the host form's definition with the host form's plan, so its bytes.  The
// workgroup is the a-trous levels' 32 x 16 pixels, and as there the window comes from one of two places:
//   * tile (RTW_OPT_ATROUS_LAYOUT 1): the workgroup's pixels plus a halo of `radius` as one LDS plane per component, r | g | b | id, the id
//     plane absent without same_object (at radius 3: 38 x 22 x 16 bytes = 13.4 KB).  Both sweeps read the tile.
//   * direct (2): every tap is a global load; the reuse between taps, and between the sweeps, is the caches'.
// 0 takes what was measured (BOUNDS_TILE; profiles/history_clamp.log).
// A tile entry outside the frame is not a tap.  What keeps it out is the inside test of bounds_tap, which the host form and the direct
// kernel need anyway and which costs four integer compares a tap; the fill of such an entry is a NaN colour besides, which the rule's
// finite test would refuse by itself, so that no entry of the tile is ever a colour the frame does not hold.
#include "rtw_bounds_dev.h"
#include "rtw_bounds.h"
#include "rtw_atrous_dev.h"
#include "rtw_svgf.h"

#include <chrono>
#include <new>

namespace rtw {
namespace {

// RTW_OPT_ATROUS_LAYOUT 0: the window is read from a tile.  profiles/history_clamp.log lines 20 .. 31, 1920 x 1080: tile 0.050 / 0.105 / 0.181 ms
// at radius 1 / 2 / 3 against direct 0.051 / 0.111 / 0.193 ms, and 0.056 / 0.112 / 0.198 against 0.068 / 0.147 / 0.259 ms with same_object and
// out_clamped: the tile is ahead in every row.
constexpr bool BOUNDS_TILE = true;

// The workgroup's tile as bounds_pixel's source: plane k starts at k * tn; (ox, oy) is the frame pixel of tile entry 0.
struct BoundsTileSrc {
    const float *p;                                // r | g | b | id
    int ox, oy, tw, tn;
    __device__ int at(int x, int y) const { return (y - oy) * tw + (x - ox); }
    __device__ BoundsColor color(int x, int y) const {
        const int i = at(x, y);
        return BoundsColor{ p[i], p[tn + i], p[2 * tn + i] };
    }
    __device__ int32_t id(int x, int y) const { return ((const int32_t *)(p + 3 * tn))[at(x, y)]; }
};

// Workgroup b covers the 32 x 16 pixels of tile (b % tiles_x, b / tiles_x).  (idx is null without same_object.)
template <bool TILE>
__global__ void __launch_bounds__(ABX * ABY) bounds_kernel(BoundsPlan pl, uint32_t tiles_x, const float *__restrict__ in,
                                                           const int32_t *__restrict__ idx, float *__restrict__ lo, float *__restrict__ hi,
                                                           float *__restrict__ clamped) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tx = (int)(threadIdx.x % ABX), ty = (int)(threadIdx.x / ABX);
    const int x0 = (int)((blockIdx.x % tiles_x) * ABX), y0 = (int)((blockIdx.x / tiles_x) * ABY);
    const int x = x0 + tx, y = y0 + ty;
    const int w = (int)pl.w, h = (int)pl.h;
    const bool inside = x < w && y < h;
    const BoundsMemSrc ms = { in, idx, pl.w };
    if (TILE) {
        const int halo = pl.radius, tw = (int)ABX + 2 * halo, th = (int)ABY + 2 * halo, tn = tw * th;
        int32_t *ids = (int32_t *)(smem + 3 * tn);
        for (int i = (int)threadIdx.x; i < tn; i += (int)(ABX * ABY)) {
            const int ix = x0 - halo + i % tw, iy = y0 - halo + i / tw;
            BoundsColor c = { __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("") };
            int32_t id = 0;
            if (ix >= 0 && iy >= 0 && ix < w && iy < h) {
                c = ms.color(ix, iy);
                if (pl.same_object) id = ms.id(ix, iy);
            }
            smem[i] = c.r; smem[tn + i] = c.g; smem[2 * tn + i] = c.b;
            if (pl.same_object) ids[i] = id;
        }
        __syncthreads();
        const BoundsTileSrc ts = { smem, x0 - halo, y0 - halo, tw, tn };
        if (inside) bounds_write(pl, ts, x, y, lo, hi, clamped);
    } else {
        if (inside) bounds_write(pl, ms, x, y, lo, hi, clamped);
    }
}

size_t bounds_tile_bytes(uint32_t radius, int same_object) {
    return (size_t)(ABX + 2 * radius) * (ABY + 2 * radius) * (same_object ? 4u : 3u) * sizeof(float);
}

// Does the pass read its window from an LDS tile?  layout: RTW_OPT_ATROUS_LAYOUT.
bool bounds_tile(uint32_t layout) { return layout == 1 || (layout == 0 && BOUNDS_TILE); }

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

} // namespace

struct BoundsScratch {
    DevMem in, idx;                                // the caller's host buffers, staged
    DevMem out_lo, out_hi, out_clamped;            // a result whose buffer is host memory
    hipEvent_t ev[2] = { nullptr, nullptr };
};

void bounds_scratch_free(BoundsScratch *s) {
    if (!s) return;
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;                                      // (the buffers free themselves)
}

#define BOUNDS_TRY(expr)                                                                                                          \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; } \
    } while (0)

int colour_bounds_device(int device, hipStream_t stream, BoundsScratch **scratch, uint32_t layout, const float *in, uint32_t w, uint32_t h,
                         const int32_t *idx, const RtwColourBounds *p, float *out_lo, float *out_hi, float *out_clamped, RtwFilterStats *stats,
                         int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    BoundsPlan pl;
    const int rc = bounds_check(in, w, h, idx, p, out_lo, out_hi, out_clamped, pl);
    if (rc != RTW_OK) return rc;
    BOUNDS_TRY(hipSetDevice(device));
    if (!*scratch) {
        BoundsScratch *s = new (std::nothrow) BoundsScratch();
        if (!s) return RTW_E_NOMEM;
        *scratch = s;                              // (owned by the context from here on, whatever follows)
        for (hipEvent_t &e : s->ev) BOUNDS_TRY(hipEventCreate(&e));
    }
    BoundsScratch *s = *scratch;
    const size_t n_px = (size_t)w * h, f3 = 3 * n_px * sizeof(float);

    // the caller's buffers on the device: a host one is staged; idx is not touched without same_object
    if (!pl.same_object) idx = nullptr;
    struct Stage { const void **p; DevMem *m; size_t bytes; };
    const Stage stages[2] = { { (const void **)&in, &s->in, f3 }, { (const void **)&idx, &s->idx, n_px * sizeof(int32_t) } };
    for (const Stage &st : stages) {
        if (!*st.p || on_device(*st.p, device)) continue;
        BOUNDS_TRY(st.m->reserve(st.bytes));
        BOUNDS_TRY(hipMemcpyAsync(st.m->ptr, *st.p, st.bytes, hipMemcpyDefault, stream));
        *st.p = st.m->ptr;
    }
    float *lo = out_lo, *hi = out_hi, *clamped = out_clamped;
    struct Result { float **p; float *host; DevMem *m; };
    Result results[3] = { { &lo, nullptr, &s->out_lo }, { &hi, nullptr, &s->out_hi }, { &clamped, nullptr, &s->out_clamped } };
    for (Result &r : results) {
        if (!*r.p || on_device(*r.p, device)) continue;
        BOUNDS_TRY(r.m->reserve(f3));
        r.host = *r.p;
        *r.p = r.m->as<float>();
    }

    const uint32_t tiles_x = (w + ABX - 1) / ABX, tiles_y = (h + ABY - 1) / ABY;
    const dim3 grid((unsigned)((uint64_t)tiles_x * tiles_y));
    BOUNDS_TRY(hipEventRecord(s->ev[0], stream));
    if (bounds_tile(layout))
        hipLaunchKernelGGL(bounds_kernel<true>, grid, dim3(ABX * ABY), bounds_tile_bytes(p->radius, pl.same_object), stream, pl, tiles_x, in, idx,
                           lo, hi, clamped);
    else
        hipLaunchKernelGGL(bounds_kernel<false>, grid, dim3(ABX * ABY), 0, stream, pl, tiles_x, in, idx, lo, hi, clamped);
    BOUNDS_TRY(hipGetLastError());
    BOUNDS_TRY(hipEventRecord(s->ev[1], stream));
    for (const Result &r : results)
        if (r.host) BOUNDS_TRY(hipMemcpyAsync(r.host, *r.p, f3, hipMemcpyDefault, stream));
    BOUNDS_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, variance_taps(w, h, p->radius) };
    }
    return RTW_OK;
}
#undef BOUNDS_TRY

} // namespace rtw
