// rtw_upsample.hip -- the guide-steered upsampling (rtw_upsample.h) on the GPU: the device path of rtw_ctx_upsample_filter.
//
// One launch, one thread per OUTPUT pixel running upsample_write -- the host form's definition with the host form's plan, so its bytes.  The
// workgroup is the a-trous levels' 32 x 16 pixels, and as there the low-resolution window comes from one of two places:
//   * tile (RTW_OPT_ATROUS_LAYOUT 1): the low pixels the workgroup's footprints can reach, as one LDS plane per component: demodulated
//     r | g | b, then depth, normal x | y | z and id, each only when its term is on.  The window starts at I0 of the workgroup's first column
//     minus (radius - 1) and is ceil(31 / scale) + 2 radius entries wide (rows likewise, from 15): I0 is monotone in the column and
//     floor(x + y) - floor(x) <= ceil(y), so the last column's I0 + radius is its last entry.  At scale 1 and radius 2 that is
//     35 x 19 x 8 planes x 4 bytes = 21.3 KB; at scale 2 and radius 1, 18 x 10 x 32 bytes = 5.8 KB.
//     The tile holds L = (lo - e) / a already: the same operations on the same operands as a tap's own demodulation, so the same bits, three
//     divides an entry in place of three a tap.
//   * direct (2): every tap is demodulated from global memory; the reuse between the scale^2 output pixels of a low pixel is the caches'.
// 0 takes what was measured (UPSAMPLE_TILE; profiles/upsample.log).
// The fallback pixel (i / s, j / s) lies inside the window: with i = s a + b, I0(i) is a - 1 or a (upsample_foot), so a is I0 or I0 + 1, both
// among the taps -(radius - 1) .. radius of that very pixel for every radius >= 1; and a <= (w - 1) / s < w_lo, so it is a pixel of the frame.
// A tile entry outside the low frame is not a tap.  What keeps it out is the inside test of upsample_pixel, which the host form and the
// direct kernel need anyway; the fill of such an entry is a NaN colour besides, which the rule's finite test would refuse by itself.
// Neighbouring lanes of a row read the same entry of a plane or the next one (scale > 1: the same for `scale` lanes), so LDS reads broadcast
// or run at stride 1.
#include "rtw_upsample_dev.h"
#include "rtw_upsample.h"
#include "rtw_atrous_dev.h"

#include <chrono>
#include <new>

namespace rtw {
namespace {

// RTW_OPT_ATROUS_LAYOUT 0: the window is read from a tile.  profiles/upsample.log lines 3 .. 15, output 1920 x 1080, every term on: tile
// 0.050 / 0.048 / 0.047 ms at scale 2 / 3 / 4 and radius 1 against direct 0.063 / 0.051 / 0.050 ms, and 0.083 / 0.082 / 0.081 against
// 0.187 / 0.135 / 0.133 ms at radius 2; with every term off 0.032 against 0.034 and 0.064 against 0.091 ms: the tile is ahead in every row.
constexpr bool UPSAMPLE_TILE = true;

// Entries of the workgroup's window along a side of n output pixels.
__host__ __device__ inline int upsample_tile_dim(int n, int scale, int radius) { return (n - 1 + scale - 1) / scale + 2 * radius; }
__host__ __device__ inline int upsample_planes(int terms) {
    return 3 + ((terms & UPSAMPLE_DEPTH) ? 1 : 0) + ((terms & UPSAMPLE_NORMAL) ? 3 : 0) + ((terms & UPSAMPLE_IDX) ? 1 : 0);
}

// The workgroup's tile as upsample_pixel's source: plane k starts at k * tn; (ox, oy) is the low pixel of tile entry 0.
struct UpsampleTileSrc {
    const float *p;                                // r | g | b | depth | nx | ny | nz | id, the off ones absent
    int ox, oy, tw, tn, terms;
    __device__ int at(int x, int y) const { return (y - oy) * tw + (x - ox); }
    __device__ UpsampleColor color(int x, int y) const {
        const int i = at(x, y);
        return UpsampleColor{ p[i], p[tn + i], p[2 * tn + i] };
    }
    __device__ UpsampleGuide guide(int x, int y) const {
        const float *q = p + 3 * tn + at(x, y);
        UpsampleGuide g = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
        if (terms & UPSAMPLE_DEPTH) { g.z = *q; q += tn; }
        if (terms & UPSAMPLE_NORMAL) { g.nx = q[0]; g.ny = q[tn]; g.nz = q[2 * tn]; q += 3 * tn; }
        if (terms & UPSAMPLE_IDX) g.id = *(const int32_t *)q;
        return g;
    }
};

// Workgroup b covers the 32 x 16 output pixels of tile (b % tiles_x, b / tiles_x).
template <bool TILE>
__global__ void __launch_bounds__(ABX * ABY) upsample_kernel(UpsamplePlan pl, uint32_t tiles_x, UpsampleBufs b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tx = (int)(threadIdx.x % ABX), ty = (int)(threadIdx.x / ABX);
    const int x0 = (int)((blockIdx.x % tiles_x) * ABX), y0 = (int)((blockIdx.x / tiles_x) * ABY);
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < (int)pl.w && y < (int)pl.h;
    const UpsampleMemSrc ms = { b.lo, b.g_lo, pl.w_lo, pl.terms, pl.albedo_floor };
    if (TILE) {
        const int tw = upsample_tile_dim((int)ABX, pl.scale, pl.radius), th = upsample_tile_dim((int)ABY, pl.scale, pl.radius), tn = tw * th;
        float t_;
        const int ox = upsample_foot(x0, pl.scale, t_) - (pl.radius - 1), oy = upsample_foot(y0, pl.scale, t_) - (pl.radius - 1);
        for (int i = (int)threadIdx.x; i < tn; i += (int)(ABX * ABY)) {
            const int ix = ox + i % tw, iy = oy + i / tw;
            UpsampleColor c = { __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("") };
            UpsampleGuide g = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
            if (ix >= 0 && iy >= 0 && ix < (int)pl.w_lo && iy < (int)pl.h_lo) {
                c = ms.color(ix, iy);
                g = ms.guide(ix, iy);
            }
            smem[i] = c.r; smem[tn + i] = c.g; smem[2 * tn + i] = c.b;
            float *q = smem + 3 * tn + i;
            if (pl.terms & UPSAMPLE_DEPTH) { *q = g.z; q += tn; }
            if (pl.terms & UPSAMPLE_NORMAL) { q[0] = g.nx; q[tn] = g.ny; q[2 * tn] = g.nz; q += 3 * tn; }
            if (pl.terms & UPSAMPLE_IDX) *(int32_t *)q = g.id;
        }
        __syncthreads();
        const UpsampleTileSrc ts = { smem, ox, oy, tw, tn, pl.terms };
        if (inside) upsample_write(pl, ts, b, x, y);
    } else {
        if (inside) upsample_write(pl, ms, b, x, y);
    }
}

size_t upsample_tile_bytes(const UpsamplePlan &pl) {
    return (size_t)upsample_tile_dim((int)ABX, pl.scale, pl.radius) * (size_t)upsample_tile_dim((int)ABY, pl.scale, pl.radius) *
           (size_t)upsample_planes(pl.terms) * sizeof(float);
}

// Does the pass read its window from an LDS tile?  layout: RTW_OPT_ATROUS_LAYOUT.
bool upsample_tile(uint32_t layout) { return layout == 1 || (layout == 0 && UPSAMPLE_TILE); }

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

} // namespace

struct UpsampleScratch {
    DevMem in[11];                                 // the caller's host buffers, staged: lo, then the five guides of each side
    DevMem out, wsum;                              // a result whose buffer is host memory
    hipEvent_t ev[2] = { nullptr, nullptr };
};

void upsample_scratch_free(UpsampleScratch *s) {
    if (!s) return;
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;                                      // (the buffers free themselves)
}

#define UPSAMPLE_TRY(expr)                                                                                                        \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; } \
    } while (0)

int upsample_filter_device(int device, hipStream_t stream, UpsampleScratch **scratch, uint32_t layout, const float *lo, uint32_t w_lo,
                           uint32_t h_lo, const RtwGuides *g_lo, uint32_t w, uint32_t h, const RtwGuides *g_hi, const RtwUpsample *p, float *out,
                           float *wsum_out, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    UpsamplePlan pl;
    UpsampleBufs b;
    const int rc = upsample_check(lo, w_lo, h_lo, g_lo, w, h, g_hi, p, out, wsum_out, pl, b);
    if (rc != RTW_OK) return rc;
    UPSAMPLE_TRY(hipSetDevice(device));
    if (!*scratch) {
        UpsampleScratch *s = new (std::nothrow) UpsampleScratch();
        if (!s) return RTW_E_NOMEM;
        *scratch = s;                              // (owned by the context from here on, whatever follows)
        for (hipEvent_t &e : s->ev) UPSAMPLE_TRY(hipEventCreate(&e));
    }
    UpsampleScratch *s = *scratch;
    const size_t n_lo = (size_t)w_lo * h_lo, n_hi = (size_t)w * h;

    // the caller's buffers on the device: a host one is staged; `b` holds no guide whose term is off
    struct Stage { const void **p; size_t bytes; };
    const Stage stages[11] = {
        { (const void **)&b.lo, 3 * n_lo * sizeof(float) },
        { (const void **)&b.g_lo.depth, n_lo * sizeof(float) }, { (const void **)&b.g_lo.normal, 3 * n_lo * sizeof(float) },
        { (const void **)&b.g_lo.idx, n_lo * sizeof(int32_t) }, { (const void **)&b.g_lo.albedo, 3 * n_lo * sizeof(float) },
        { (const void **)&b.g_lo.emitted, 3 * n_lo * sizeof(float) },
        { (const void **)&b.g_hi.depth, n_hi * sizeof(float) }, { (const void **)&b.g_hi.normal, 3 * n_hi * sizeof(float) },
        { (const void **)&b.g_hi.idx, n_hi * sizeof(int32_t) }, { (const void **)&b.g_hi.albedo, 3 * n_hi * sizeof(float) },
        { (const void **)&b.g_hi.emitted, 3 * n_hi * sizeof(float) },
    };
    for (int k = 0; k < 11; k++) {
        const Stage &st = stages[k];
        if (!*st.p || on_device(*st.p, device)) continue;
        UPSAMPLE_TRY(s->in[k].reserve(st.bytes));
        UPSAMPLE_TRY(hipMemcpyAsync(s->in[k].ptr, *st.p, st.bytes, hipMemcpyDefault, stream));
        *st.p = s->in[k].ptr;
    }
    struct Result { float **p; float *host; DevMem *m; size_t bytes; };
    Result results[2] = { { &b.out, nullptr, &s->out, 3 * n_hi * sizeof(float) }, { &b.wsum, nullptr, &s->wsum, n_hi * sizeof(float) } };
    for (Result &r : results) {
        if (!*r.p || on_device(*r.p, device)) continue;
        UPSAMPLE_TRY(r.m->reserve(r.bytes));
        r.host = *r.p;
        *r.p = r.m->as<float>();
    }

    const uint32_t tiles_x = (w + ABX - 1) / ABX, tiles_y = (h + ABY - 1) / ABY;
    const dim3 grid((unsigned)((uint64_t)tiles_x * tiles_y));
    UPSAMPLE_TRY(hipEventRecord(s->ev[0], stream));
    if (upsample_tile(layout))
        hipLaunchKernelGGL(upsample_kernel<true>, grid, dim3(ABX * ABY), upsample_tile_bytes(pl), stream, pl, tiles_x, b);
    else
        hipLaunchKernelGGL(upsample_kernel<false>, grid, dim3(ABX * ABY), 0, stream, pl, tiles_x, b);
    UPSAMPLE_TRY(hipGetLastError());
    UPSAMPLE_TRY(hipEventRecord(s->ev[1], stream));
    for (const Result &r : results)
        if (r.host) UPSAMPLE_TRY(hipMemcpyAsync(r.host, *r.p, r.bytes, hipMemcpyDefault, stream));
    UPSAMPLE_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, upsample_taps(pl) };
    }
    return RTW_OK;
}
#undef UPSAMPLE_TRY

} // namespace rtw
