// rtw_svgf.hip -- the variance estimate and the variance-steered a-trous filter (rtw_svgf.h) on the GPU: the device paths of
// rtw_ctx_variance_estimate and rtw_ctx_svgf_filter.
//
// The variance estimate is one launch, one thread per pixel running variance_pixel; the filter is one launch that demodulates colour and
// variance into the first of two ping-pong pairs of the context, then one launch per level, one thread per pixel running svgf_pixel --
// the host forms' definitions, so their bytes.  The last level remodulates as it writes, straight into the caller's buffers when those are
// device memory.  The workgroup is the a-trous levels' 32 x 16 pixels, and as there the taps come from one of two places:
//   * tile (RTW_OPT_ATROUS_LAYOUT 1): the workgroup's pixels plus a halo (2 * step for a level, `radius` for the estimate) as one LDS plane
//     per component (a level: r | g | b | v | z | nx | ny | nz | id; the estimate: m1 | m2 | len | z | nx | ny | nz | id; an absent guide
//     takes no room).  A level whose tile is beyond ATROUS_TILE_LDS_MAX runs the other kernel.  The estimate's workgroup fills its tile only
//     when one of its pixels has a history short enough to need the window.
//   * direct (2): every tap is a global load; the reuse between taps is the caches'.
// 0 takes what was measured (svgf_tile_level, variance_tile; profiles/svgf.log).
#include "rtw_svgf_dev.h"
#include "rtw_svgf.h"

#include <chrono>

namespace rtw {
namespace {

constexpr uint32_t SVGF_TILE_LEVELS = 3;                 // RTW_OPT_ATROUS_LAYOUT 0: levels below this read a tile where it fits (profiles/svgf.log)
constexpr bool VARIANCE_TILE = true;                     // RTW_OPT_ATROUS_LAYOUT 0: the estimate reads its window from a tile (profiles/svgf.log)

constexpr uint32_t guide_planes(int terms) {
    return (terms & ATROUS_DEPTH ? 1u : 0u) + (terms & ATROUS_NORMAL ? 3u : 0u) + (terms & ATROUS_IDX ? 1u : 0u);
}

// The guide planes of a tile, behind its `first` leading planes of tn entries each.
struct TileGuides {
    float *gz, *gn;
    int32_t *gi;
    __device__ TileGuides(float *smem, int first, int tn, int terms) {
        gz = smem + first * tn;
        gn = gz + ((terms & ATROUS_DEPTH) ? tn : 0);
        gi = (int32_t *)(gn + ((terms & ATROUS_NORMAL) ? 3 * tn : 0));
    }
    __device__ void store(int i, int tn, int terms, const AtrousGuide &g) const {
        if (terms & ATROUS_DEPTH) gz[i] = g.z;
        if (terms & ATROUS_NORMAL) { gn[i] = g.nx; gn[tn + i] = g.ny; gn[2 * tn + i] = g.nz; }
        if (terms & ATROUS_IDX) gi[i] = g.id;
    }
    __device__ AtrousGuide load(int i, int tn, int terms) const {
        AtrousGuide g = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
        if (terms & ATROUS_DEPTH) g.z = gz[i];
        if (terms & ATROUS_NORMAL) { g.nx = gn[i]; g.ny = gn[tn + i]; g.nz = gn[2 * tn + i]; }
        if (terms & ATROUS_IDX) g.id = gi[i];
        return g;
    }
};

// ---- the variance estimate -------------------------------------------------------------------------------------------------------------
// The workgroup's tile as variance_pixel's source: plane k starts at k * tn; (ox, oy) is the frame pixel of tile entry 0.
struct VarianceTileSrc {
    const float *p;                                // m1 | m2 | len
    TileGuides gd;
    int ox, oy, tw, tn, terms;
    __device__ int at(int x, int y) const { return (y - oy) * tw + (x - ox); }
    __device__ float m1(int x, int y) const { return p[at(x, y)]; }
    __device__ float m2(int x, int y) const { return p[tn + at(x, y)]; }
    __device__ float len(int x, int y) const { return p[2 * tn + at(x, y)]; }
    __device__ AtrousGuide guide(int x, int y) const { return gd.load(at(x, y), tn, terms); }
};

// Workgroup b covers the 32 x 16 pixels of tile (b % tiles_x, b / tiles_x).
template <bool TILE>
__global__ void __launch_bounds__(ABX * ABY) variance_kernel(VariancePlan pl, uint32_t tiles_x, const float *__restrict__ moments,
                                                             const float *__restrict__ len, const float *__restrict__ depth,
                                                             const float *__restrict__ normal, const int32_t *__restrict__ idx,
                                                             float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tx = (int)(threadIdx.x % ABX), ty = (int)(threadIdx.x / ABX);
    const int x0 = (int)((blockIdx.x % tiles_x) * ABX), y0 = (int)((blockIdx.x / tiles_x) * ABY);
    const int x = x0 + tx, y = y0 + ty;
    const int w = (int)pl.lv.w, h = (int)pl.lv.h, terms = pl.lv.terms;
    const bool inside = x < w && y < h;
    const VarianceMemSrc ms = { moments, len, AtrousMemSrc{ nullptr, depth, normal, idx, pl.lv.w, terms } };
    float v = 0.0f;
    bool tile = false;
    if (TILE) tile = __syncthreads_or(inside && !(ms.len(x, y) >= pl.min_history)) != 0;      // does any pixel here read its window?
    if (tile) {
        const int halo = pl.radius, tw = (int)ABX + 2 * halo, th = (int)ABY + 2 * halo, tn = tw * th;
        const TileGuides gd(smem, 3, tn, terms);
        for (int i = (int)threadIdx.x; i < tn; i += (int)(ABX * ABY)) {
            const int ix = x0 - halo + i % tw, iy = y0 - halo + i / tw;
            float m1 = 0.0f, m2 = 0.0f, n = 0.0f;
            AtrousGuide gq = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
            if (ix >= 0 && iy >= 0 && ix < w && iy < h) { m1 = ms.m1(ix, iy); m2 = ms.m2(ix, iy); n = ms.len(ix, iy); gq = ms.guide(ix, iy); }
            smem[i] = m1; smem[tn + i] = m2; smem[2 * tn + i] = n;
            gd.store(i, tn, terms, gq);
        }
        __syncthreads();
        const VarianceTileSrc ts = { smem, gd, x0 - halo, y0 - halo, tw, tn, terms };
        if (inside) v = variance_pixel(pl, ts, x, y);
    } else {
        if (inside) v = variance_pixel(pl, ms, x, y);
    }
    if (inside) out[(size_t)y * pl.lv.w + (size_t)x] = v;
}

size_t variance_tile_bytes(int terms, uint32_t radius) {
    return (size_t)(ABX + 2 * radius) * (ABY + 2 * radius) * (3u + guide_planes(terms)) * sizeof(float);
}

// Does the estimate read its window from an LDS tile?  layout: RTW_OPT_ATROUS_LAYOUT.
bool variance_tile(uint32_t layout) { return layout == 1 || (layout == 0 && VARIANCE_TILE); }

// ---- the variance-steered a-trous filter -----------------------------------------------------------------------------------------------
// One thread per pixel: C0 into `c`, V0 into `v`.
__global__ void __launch_bounds__(256) svgf_demodulate_kernel(const float *__restrict__ in, const float *__restrict__ variance,
                                                              const float *__restrict__ albedo, const float *__restrict__ emitted, float floor_,
                                                              size_t n_px, float *__restrict__ c, float *__restrict__ v) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_px) return;
    for (size_t i = 3 * p; i < 3 * p + 3; i++) c[i] = atrous_demodulate(in, albedo, emitted, floor_, i);
    v[p] = svgf_demodulate_variance(variance, albedo, floor_, p);
}

// The workgroup's tile as svgf_pixel's source.
struct SvgfTileSrc {
    const float *c;                                // r | g | b | v
    TileGuides gd;
    int ox, oy, tw, tn, terms;
    __device__ int at(int x, int y) const { return (y - oy) * tw + (x - ox); }
    __device__ AtrousColor color(int x, int y) const {
        const int i = at(x, y);
        return AtrousColor{ c[i], c[tn + i], c[2 * tn + i] };
    }
    __device__ float var(int x, int y) const { return c[3 * tn + at(x, y)]; }
    __device__ AtrousGuide guide(int x, int y) const { return gd.load(at(x, y), tn, terms); }
};

// One level.  last: colour and variance are remodulated as they are written (vdst may then be NULL: the caller wants no variance).
template <bool TILE>
__global__ void __launch_bounds__(ABX * ABY) svgf_level_kernel(SvgfLevel sv, uint32_t tiles_x, const float *__restrict__ src,
                                                               const float *__restrict__ vsrc, const float *__restrict__ depth,
                                                               const float *__restrict__ normal, const int32_t *__restrict__ idx,
                                                               const float *albedo, const float *emitted, float floor_, int last, float *dst,
                                                               float *vdst) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AtrousLevel &lv = sv.lv;
    const int tx = (int)(threadIdx.x % ABX), ty = (int)(threadIdx.x / ABX);
    const int x0 = (int)((blockIdx.x % tiles_x) * ABX), y0 = (int)((blockIdx.x / tiles_x) * ABY);
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < (int)lv.w && y < (int)lv.h;
    const SvgfMemSrc ms = { AtrousMemSrc{ src, depth, normal, idx, lv.w, lv.terms }, vsrc };
    SvgfPixel o = { { 0.0f, 0.0f, 0.0f }, 0.0f };
    if (TILE) {
        const int halo = 2 * lv.step, tw = (int)ABX + 2 * halo, th = (int)ABY + 2 * halo, tn = tw * th;
        const TileGuides gd(smem, 4, tn, lv.terms);
        for (int i = (int)threadIdx.x; i < tn; i += (int)(ABX * ABY)) {
            const int ix = x0 - halo + i % tw, iy = y0 - halo + i / tw;
            AtrousColor cq = { 0.0f, 0.0f, 0.0f };
            AtrousGuide gq = { 0.0f, 0.0f, 0.0f, 0.0f, 0 };
            float vq = 0.0f;
            if (ix >= 0 && iy >= 0 && ix < (int)lv.w && iy < (int)lv.h) { cq = ms.color(ix, iy); gq = ms.guide(ix, iy); vq = ms.var(ix, iy); }
            smem[i] = cq.r; smem[tn + i] = cq.g; smem[2 * tn + i] = cq.b; smem[3 * tn + i] = vq;
            gd.store(i, tn, lv.terms, gq);
        }
        __syncthreads();
        const SvgfTileSrc ts = { smem, gd, x0 - halo, y0 - halo, tw, tn, lv.terms };
        if (inside) o = svgf_pixel(sv, ts, x, y);
    } else {
        if (inside) o = svgf_pixel(sv, ms, x, y);
    }
    if (!inside) return;
    const size_t q = (size_t)y * lv.w + (size_t)x, p = 3 * q;
    if (last) {
        o.c.r = atrous_remodulate(o.c.r, albedo, emitted, floor_, p);
        o.c.g = atrous_remodulate(o.c.g, albedo, emitted, floor_, p + 1);
        o.c.b = atrous_remodulate(o.c.b, albedo, emitted, floor_, p + 2);
        o.v = svgf_remodulate_variance(o.v, albedo, floor_, q);
    }
    dst[p] = o.c.r; dst[p + 1] = o.c.g; dst[p + 2] = o.c.b;
    if (vdst) vdst[q] = o.v;
}

size_t svgf_tile_bytes(int terms, uint32_t level) {
    const size_t halo = (size_t)2 << level;
    return (ABX + 2 * halo) * (ABY + 2 * halo) * (4u + guide_planes(terms)) * sizeof(float);
}

// Does level `level` read its taps from an LDS tile?  layout: RTW_OPT_ATROUS_LAYOUT.
bool svgf_tile_level(uint32_t layout, int terms, uint32_t level) {
    if (svgf_tile_bytes(terms, level) > ATROUS_TILE_LDS_MAX) return false;
    if (layout == 1) return true;
    if (layout == 2) return false;
    return level < SVGF_TILE_LEVELS;
}

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

struct Stage { const void **p; DevMem *m; size_t bytes; };

} // namespace

#define SVGF_TRY(expr)                                                                                                            \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; } \
    } while (0)

int variance_estimate_device(int device, hipStream_t stream, AtrousScratch **scratch, uint32_t layout, const float *moments, const float *len,
                             uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx, const RtwVarianceEstimate *p,
                             float *out, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    VariancePlan pl;
    const int rc = variance_check(moments, len, w, h, depth, normal, idx, p, out, pl);
    if (rc != RTW_OK) return rc;
    SVGF_TRY(hipSetDevice(device));
    SVGF_TRY(atrous_scratch_get(scratch));
    AtrousScratch *s = *scratch;
    const size_t n_px = (size_t)w * h, f1 = n_px * sizeof(float);
    const int terms = pl.lv.terms;

    // the caller's buffers on the device: a host one is staged; a guide whose term is off is not touched
    if (!(terms & ATROUS_DEPTH)) depth = nullptr;
    if (!(terms & ATROUS_NORMAL)) normal = nullptr;
    if (!(terms & ATROUS_IDX)) idx = nullptr;
    const Stage stages[5] = { { (const void **)&moments, &s->moments, 2 * f1 },
                              { (const void **)&len, &s->len, f1 },
                              { (const void **)&depth, &s->depth, f1 },
                              { (const void **)&normal, &s->normal, 3 * f1 },
                              { (const void **)&idx, &s->idx, n_px * sizeof(int32_t) } };
    for (const Stage &st : stages) {
        if (!*st.p || on_device(*st.p, device)) continue;
        SVGF_TRY(st.m->reserve(st.bytes));
        SVGF_TRY(hipMemcpyAsync(st.m->ptr, *st.p, st.bytes, hipMemcpyDefault, stream));
        *st.p = st.m->ptr;
    }
    float *dst = out;
    const bool direct = on_device(out, device);
    if (!direct) { SVGF_TRY(s->out_variance.reserve(f1)); dst = s->out_variance.as<float>(); }

    const uint32_t tiles_x = (w + ABX - 1) / ABX, tiles_y = (h + ABY - 1) / ABY;
    const dim3 grid((unsigned)((uint64_t)tiles_x * tiles_y));
    SVGF_TRY(hipEventRecord(s->ev[0], stream));
    if (variance_tile(layout))
        hipLaunchKernelGGL(variance_kernel<true>, grid, dim3(ABX * ABY), variance_tile_bytes(terms, p->radius), stream, pl, tiles_x, moments, len,
                           depth, normal, idx, dst);
    else
        hipLaunchKernelGGL(variance_kernel<false>, grid, dim3(ABX * ABY), 0, stream, pl, tiles_x, moments, len, depth, normal, idx, dst);
    SVGF_TRY(hipGetLastError());
    SVGF_TRY(hipEventRecord(s->ev[1], stream));
    if (!direct) SVGF_TRY(hipMemcpyAsync(out, dst, f1, hipMemcpyDefault, stream));
    SVGF_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, variance_taps(w, h, p->radius) };
    }
    return RTW_OK;
}

int svgf_filter_device(int device, hipStream_t stream, AtrousScratch **scratch, uint32_t layout, const float *in, const float *variance, uint32_t w,
                       uint32_t h, const float *depth, const float *normal, const int32_t *idx, const float *albedo, const float *emitted,
                       const RtwAtrous *p, const RtwSvgf *vp, float *out, float *out_variance, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    SvgfPlan pl;
    const int rc = svgf_check(in, variance, w, h, depth, normal, idx, albedo, p, vp, out, out_variance, pl);
    if (rc != RTW_OK) return rc;
    SVGF_TRY(hipSetDevice(device));
    SVGF_TRY(atrous_scratch_get(scratch));
    AtrousScratch *s = *scratch;
    const size_t n_px = (size_t)w * h, f1 = n_px * sizeof(float);
    const int terms = pl.at.terms;

    if (!(terms & ATROUS_DEPTH)) depth = nullptr;
    if (!(terms & ATROUS_NORMAL)) normal = nullptr;
    if (!(terms & ATROUS_IDX)) idx = nullptr;
    const Stage stages[7] = { { (const void **)&in, &s->in, 3 * f1 },
                              { (const void **)&variance, &s->variance, f1 },
                              { (const void **)&depth, &s->depth, f1 },
                              { (const void **)&normal, &s->normal, 3 * f1 },
                              { (const void **)&idx, &s->idx, n_px * sizeof(int32_t) },
                              { (const void **)&albedo, &s->albedo, 3 * f1 },
                              { (const void **)&emitted, &s->emitted, 3 * f1 } };
    for (const Stage &st : stages) {
        if (!*st.p || on_device(*st.p, device)) continue;
        SVGF_TRY(st.m->reserve(st.bytes));
        SVGF_TRY(hipMemcpyAsync(st.m->ptr, *st.p, st.bytes, hipMemcpyDefault, stream));
        *st.p = st.m->ptr;
    }
    float *dst = out, *vout = out_variance;
    const bool direct = on_device(out, device), vdirect = !out_variance || on_device(out_variance, device);
    if (!direct) { SVGF_TRY(s->out.reserve(3 * f1)); dst = s->out.as<float>(); }
    if (!vdirect) { SVGF_TRY(s->out_variance.reserve(f1)); vout = s->out_variance.as<float>(); }
    SVGF_TRY(s->ping.reserve(3 * f1));
    SVGF_TRY(s->pong.reserve(3 * f1));
    SVGF_TRY(s->vping.reserve(f1));
    SVGF_TRY(s->vpong.reserve(f1));

    SVGF_TRY(hipEventRecord(s->ev[0], stream));
    hipLaunchKernelGGL(svgf_demodulate_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream, in, variance, albedo, emitted,
                       pl.at.albedo_floor, n_px, s->ping.as<float>(), s->vping.as<float>());
    const uint32_t tiles_x = (w + ABX - 1) / ABX, tiles_y = (h + ABY - 1) / ABY;
    const dim3 grid((unsigned)((uint64_t)tiles_x * tiles_y));
    float *src = s->ping.as<float>(), *tmp = s->pong.as<float>(), *vsrc = s->vping.as<float>(), *vtmp = s->vpong.as<float>();
    for (uint32_t i = 0; i < pl.at.levels; i++) {
        const SvgfLevel sv = svgf_level(pl, i, w, h);
        const int last = i + 1 == pl.at.levels;
        float *to = last ? dst : tmp, *vto = last ? vout : vtmp;
        if (svgf_tile_level(layout, terms, i))
            hipLaunchKernelGGL(svgf_level_kernel<true>, grid, dim3(ABX * ABY), svgf_tile_bytes(terms, i), stream, sv, tiles_x, src, vsrc, depth, normal,
                               idx, albedo, emitted, pl.at.albedo_floor, last, to, vto);
        else
            hipLaunchKernelGGL(svgf_level_kernel<false>, grid, dim3(ABX * ABY), 0, stream, sv, tiles_x, src, vsrc, depth, normal, idx, albedo, emitted,
                               pl.at.albedo_floor, last, to, vto);
        tmp = src; src = to;
        vtmp = vsrc; vsrc = vto;
    }
    SVGF_TRY(hipGetLastError());
    SVGF_TRY(hipEventRecord(s->ev[1], stream));
    if (!direct) SVGF_TRY(hipMemcpyAsync(out, dst, 3 * f1, hipMemcpyDefault, stream));
    if (!vdirect) SVGF_TRY(hipMemcpyAsync(out_variance, vout, f1, hipMemcpyDefault, stream));
    SVGF_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, atrous_taps(w, h, pl.at.levels) };
    }
    return RTW_OK;
}
#undef SVGF_TRY

} // namespace rtw
