// rtw_atrous.hip -- the a-trous filter (rtw_atrous.h) on the GPU: rtw_ctx_atrous_filter's device path.
//
// One launch demodulates into the first of two ping-pong buffers of the context, then one launch per level, one thread per pixel, each
// running atrous_pixel -- the host form's definition, so its bytes.  The last level remodulates as it writes, straight into the caller's
// buffer when that is device memory.  A level's 25 taps come from one of two places:
//   * tile (RTW_OPT_ATROUS_LAYOUT 1): the workgroup's 32 x 16 pixels plus a halo of 2 * step, as one LDS plane per component (r | g | b |
//     z | nx | ny | nz | id, an absent guide takes no room).  A wave reads two rows of 32 consecutive dwords of a plane: conflict-free.
//     Taken while the tile fits in ATROUS_TILE_LDS_MAX; a level whose tile does not fit runs the other kernel.
//   * direct (2): every tap is a global load; neighbouring lanes read neighbouring pixels and the reuse between taps is the caches'.
// 0 takes what was measured per level (atrous_tile_level, profiles/atrous.log).
#include "rtw_atrous_dev.h"
#include "rtw_atrous.h"
#include "rtw_devmem.h"

#include <chrono>
#include <new>

namespace rtw {
namespace {

constexpr uint32_t ATROUS_TILE_LEVELS = 3;               // RTW_OPT_ATROUS_LAYOUT 0: levels below this (steps 1, 2, 4) read a tile where it fits:
                                                         // measured faster there, and no faster from step 8 on (profiles/atrous.log)

__global__ void __launch_bounds__(256) atrous_demodulate_kernel(const float *__restrict__ in, const float *__restrict__ albedo,
                                                                const float *__restrict__ emitted, float floor_, size_t n,
                                                                float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = atrous_demodulate(in, albedo, emitted, floor_, i);
}

constexpr uint32_t atrous_planes(int terms) {
    return 3u + (terms & ATROUS_DEPTH ? 1u : 0u) + (terms & ATROUS_NORMAL ? 3u : 0u) + (terms & ATROUS_IDX ? 1u : 0u);
}

// The workgroup's tile as atrous_pixel's source: plane k of the tile starts at k * tn; (ox, oy) is the frame pixel of tile entry 0.
struct AtrousTileSrc {
    const float *c, *gz, *gn;
    const int32_t *gi;
    int ox, oy, tw, tn, terms;
    __device__ int at(int x, int y) const { return (y - oy) * tw + (x - ox); }
    __device__ AtrousColor color(int x, int y) const {
        const int i = at(x, y);
        return AtrousColor{ c[i], c[tn + i], c[2 * tn + i] };
    }
    __device__ AtrousGuide guide(int x, int y) const {
        const int i = at(x, y);
        AtrousGuide g = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
        if (terms & ATROUS_DEPTH) g.z = gz[i];
        if (terms & ATROUS_NORMAL) { g.nx = gn[i]; g.ny = gn[tn + i]; g.nz = gn[2 * tn + i]; }
        if (terms & ATROUS_IDX) g.id = gi[i];
        return g;
    }
};

// One level.  Workgroup b covers the 32 x 16 pixels of tile (b % tiles_x, b / tiles_x).  last: the result is remodulated as it is written.
template <bool TILE>
__global__ void __launch_bounds__(ABX * ABY) atrous_level_kernel(AtrousLevel lv, uint32_t tiles_x, const float *__restrict__ src,
                                                                 const float *__restrict__ depth, const float *__restrict__ normal,
                                                                 const int32_t *__restrict__ idx, const float *albedo, const float *emitted,
                                                                 float floor_, int last, float *dst) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tx = (int)(threadIdx.x % ABX), ty = (int)(threadIdx.x / ABX);
    const int x0 = (int)((blockIdx.x % tiles_x) * ABX), y0 = (int)((blockIdx.x / tiles_x) * ABY);
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < (int)lv.w && y < (int)lv.h;
    const AtrousMemSrc ms = { src, depth, normal, idx, lv.w, lv.terms };
    AtrousColor o = { 0.0f, 0.0f, 0.0f };
    if (TILE) {
        const int halo = 2 * lv.step, tw = (int)ABX + 2 * halo, th = (int)ABY + 2 * halo, tn = tw * th;
        float *c = smem, *gz = c + 3 * tn, *gn = gz + ((lv.terms & ATROUS_DEPTH) ? tn : 0);
        int32_t *gi = (int32_t *)(gn + ((lv.terms & ATROUS_NORMAL) ? 3 * tn : 0));
        for (int i = (int)threadIdx.x; i < tn; i += (int)(ABX * ABY)) {
            const int ix = x0 - halo + i % tw, iy = y0 - halo + i / tw;
            AtrousColor cq = { 0.0f, 0.0f, 0.0f };
            AtrousGuide gq = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
            if (ix >= 0 && iy >= 0 && ix < (int)lv.w && iy < (int)lv.h) { cq = ms.color(ix, iy); gq = ms.guide(ix, iy); }
            c[i] = cq.r; c[tn + i] = cq.g; c[2 * tn + i] = cq.b;
            if (lv.terms & ATROUS_DEPTH) gz[i] = gq.z;
            if (lv.terms & ATROUS_NORMAL) { gn[i] = gq.nx; gn[tn + i] = gq.ny; gn[2 * tn + i] = gq.nz; }
            if (lv.terms & ATROUS_IDX) gi[i] = gq.id;
        }
        __syncthreads();
        const AtrousTileSrc ts = { c, gz, gn, gi, x0 - halo, y0 - halo, tw, tn, lv.terms };
        if (inside) o = atrous_pixel(lv, ts, x, y);
    } else {
        if (inside) o = atrous_pixel(lv, ms, x, y);
    }
    if (!inside) return;
    const size_t p = 3 * ((size_t)y * lv.w + (size_t)x);
    if (last) {
        o.r = atrous_remodulate(o.r, albedo, emitted, floor_, p);
        o.g = atrous_remodulate(o.g, albedo, emitted, floor_, p + 1);
        o.b = atrous_remodulate(o.b, albedo, emitted, floor_, p + 2);
    }
    dst[p] = o.r; dst[p + 1] = o.g; dst[p + 2] = o.b;
}

size_t atrous_tile_bytes(int terms, uint32_t level) {
    const size_t halo = (size_t)2 << level;
    return (ABX + 2 * halo) * (ABY + 2 * halo) * atrous_planes(terms) * sizeof(float);
}

// Does level `level` read its taps from an LDS tile?  layout: RTW_OPT_ATROUS_LAYOUT.
bool atrous_tile_level(uint32_t layout, int terms, uint32_t level) {
    if (atrous_tile_bytes(terms, level) > ATROUS_TILE_LDS_MAX) return false;
    if (layout == 1) return true;
    if (layout == 2) return false;
    return level < ATROUS_TILE_LEVELS;
}

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

} // namespace

void atrous_scratch_free(AtrousScratch *s) {
    if (!s) return;
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;                                      // (the buffers free themselves)
}

hipError_t atrous_scratch_get(AtrousScratch **scratch) {
    if (*scratch) return hipSuccess;
    AtrousScratch *s = new (std::nothrow) AtrousScratch();
    if (!s) return hipErrorOutOfMemory;
    *scratch = s;                                  // (owned by the context from here on, whatever follows)
    for (hipEvent_t &e : s->ev) {
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
    }
    return hipSuccess;
}

#define ATROUS_TRY(expr)                                                                                                          \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; } \
    } while (0)

int atrous_filter_device(int device, hipStream_t stream, AtrousScratch **scratch, uint32_t layout, const float *in, uint32_t w, uint32_t h,
                         const float *depth, const float *normal, const int32_t *idx, const float *albedo, const float *emitted,
                         const RtwAtrous *p, float *out, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    AtrousPlan pl;
    const int rc = atrous_check(in, w, h, depth, normal, idx, albedo, p, out, pl);
    if (rc != RTW_OK) return rc;
    ATROUS_TRY(hipSetDevice(device));
    ATROUS_TRY(atrous_scratch_get(scratch));
    AtrousScratch *s = *scratch;
    const size_t n_px = (size_t)w * h, n = 3 * n_px;

    // the caller's buffers on the device: a host one is staged; a guide whose term is off is not touched
    if (!(pl.terms & ATROUS_DEPTH)) depth = nullptr;
    if (!(pl.terms & ATROUS_NORMAL)) normal = nullptr;
    if (!(pl.terms & ATROUS_IDX)) idx = nullptr;
    struct Stage { const void **p; DevMem *m; size_t bytes; };
    const Stage stages[6] = { { (const void **)&in, &s->in, n * sizeof(float) },
                              { (const void **)&depth, &s->depth, n_px * sizeof(float) },
                              { (const void **)&normal, &s->normal, n * sizeof(float) },
                              { (const void **)&idx, &s->idx, n_px * sizeof(int32_t) },
                              { (const void **)&albedo, &s->albedo, n * sizeof(float) },
                              { (const void **)&emitted, &s->emitted, n * sizeof(float) } };
    for (const Stage &st : stages) {
        if (!*st.p || on_device(*st.p, device)) continue;
        ATROUS_TRY(st.m->reserve(st.bytes));
        ATROUS_TRY(hipMemcpyAsync(st.m->ptr, *st.p, st.bytes, hipMemcpyDefault, stream));
        *st.p = st.m->ptr;
    }
    float *dst = out;
    const bool direct = on_device(out, device);
    if (!direct) { ATROUS_TRY(s->out.reserve(n * sizeof(float))); dst = s->out.as<float>(); }
    ATROUS_TRY(s->ping.reserve(n * sizeof(float)));
    ATROUS_TRY(s->pong.reserve(n * sizeof(float)));

    ATROUS_TRY(hipEventRecord(s->ev[0], stream));
    hipLaunchKernelGGL(atrous_demodulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, albedo, emitted, pl.albedo_floor,
                       n, s->ping.as<float>());
    const uint32_t tiles_x = (w + ABX - 1) / ABX, tiles_y = (h + ABY - 1) / ABY;
    const dim3 grid((unsigned)((uint64_t)tiles_x * tiles_y));
    float *src = s->ping.as<float>(), *tmp = s->pong.as<float>();
    for (uint32_t i = 0; i < pl.levels; i++) {
        const AtrousLevel lv = atrous_level(pl, i, w, h);
        const int last = i + 1 == pl.levels;
        float *to = last ? dst : tmp;
        if (atrous_tile_level(layout, pl.terms, i))
            hipLaunchKernelGGL(atrous_level_kernel<true>, grid, dim3(ABX * ABY), atrous_tile_bytes(pl.terms, i), stream, lv, tiles_x, src, depth,
                               normal, idx, albedo, emitted, pl.albedo_floor, last, to);
        else
            hipLaunchKernelGGL(atrous_level_kernel<false>, grid, dim3(ABX * ABY), 0, stream, lv, tiles_x, src, depth, normal, idx, albedo, emitted,
                               pl.albedo_floor, last, to);
        tmp = src;
        src = to;
    }
    ATROUS_TRY(hipGetLastError());
    ATROUS_TRY(hipEventRecord(s->ev[1], stream));
    if (!direct) ATROUS_TRY(hipMemcpyAsync(out, dst, n * sizeof(float), hipMemcpyDefault, stream));
    ATROUS_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, atrous_taps(w, h, pl.levels) };
    }
    return RTW_OK;
}
#undef ATROUS_TRY

} // namespace rtw
