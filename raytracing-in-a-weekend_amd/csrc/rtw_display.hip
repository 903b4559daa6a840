// rtw_display.hip -- the display stage (rtw_display.h) on the GPU: the device paths of rtw_ctx_luminance_histogram and
// rtw_ctx_display.  Both kernels run the host forms' definitions (histogram_slot, display_value / display_byte / display_write) with the host
// forms' plan, so they give the host forms' counts and bytes.
//
// Both take four consecutive pixels of the flat frame a thread -- 48 bytes, three 16-byte loads -- when `in` is 16-byte aligned (and, for the
// display transform, `out` is aligned for one wide store: 4 bytes for RGB8's 12, 16 bytes for RGBA8's 16 and F32's 48), and one pixel a thread
// otherwise and for the last w * h % 4 pixels.  A buffer of hipMalloc or a whole torch tensor is aligned; a numpy view or a torch slice that
// starts at pixel 1 is 12 bytes off.
//
// The histogram: a grid-stride loop of at most RTW_HISTOGRAM_BLOCKS_PER_CU workgroups of 256 threads a compute unit.  A workgroup counts into
// LDS (258 slots: the bins, black, non-finite) with LDS integer atomics and, at its end, adds every non-empty slot to the context's 258
// counters with one global atomicAdd; the counters are zeroed by a hipMemsetAsync enqueued on the same stream in front of the launch, and
// copied to `hist` and `counts` behind it.  RTW_OPT_HISTOGRAM_COUNT chooses how the LDS counts are kept:
//   1 plain:    one histogram, one LDS atomic a pixel.  On a frame of one luminance all 64 lanes of a wave hit one address.
//   2 per wave: one histogram a wave (4 x 258 x 4 bytes), summed by the flush: a quarter of the lanes meet at an address.
//   3 ballot:   one histogram; the lanes that share the first active lane's slot are counted with a ballot and added by that lane as one
//               atomic, the others add 1 each: one atomic a wave on a constant frame, one more than plain on noise.
// 0 takes what was measured (HIST_COUNT below; profiles/display.log).
#include "rtw_display_dev.h"
#include "rtw_display.h"
#include "rtw_devmem.h"

#include <chrono>
#include <new>

namespace rtw {
namespace {

constexpr uint32_t DISPLAY_THREADS = 256;                                  // both kernels; RTW_HISTOGRAM_BLOCK_PIXELS = 4 x this
constexpr uint32_t WAVE = 64;
static_assert(RTW_HISTOGRAM_BLOCK_PIXELS == 4 * DISPLAY_THREADS, "four pixels a thread");

enum { COUNT_PLAIN = 1, COUNT_PER_WAVE = 2, COUNT_BALLOT = 3 };
// RTW_OPT_HISTOGRAM_COUNT 0.  profiles/display.log section (a), 1920 x 1080, plain / per wave / ballot: white noise 0.0247 / 0.0248 /
// 0.0253 ms, a constant frame 0.0188 / 0.0190 / 0.0175 ms, the Book-1 4-spp frame 0.0252 / 0.0253 / 0.0251 ms.  The three are within 2 % of
// each other but on the constant frame, where the ballot is 7 % ahead: it is the choice.  A histogram a wave buys nothing anywhere.
constexpr int HIST_COUNT = COUNT_BALLOT;

template <int COUNT>
__device__ __forceinline__ void histogram_add(uint32_t *lds, int slot) {
    if (COUNT == COUNT_BALLOT) {
        const int first = __builtin_amdgcn_readfirstlane(slot);            // the first active lane's slot
        const bool same = slot == first;
        const unsigned long long m = __ballot(same);
        if (same) {
            if ((int)__lane_id() == __ffsll(m) - 1) atomicAdd(&lds[first], (uint32_t)__popcll(m));
        } else {
            atomicAdd(&lds[slot], 1u);
        }
    } else {
        atomicAdd(&lds[slot], 1u);
    }
}

// n_quads: the groups of four pixels read 16 bytes at a time (0 when `in` is not 16-byte aligned); the pixels from 4 * n_quads on are read
// one a thread.  g: the 258 counters, zeroed on the stream in front of the launch.
template <int COUNT>
__global__ void __launch_bounds__(DISPLAY_THREADS) histogram_kernel(const float *in, uint64_t n_pixels, uint64_t n_quads, uint32_t *g) {
    constexpr int SUBS = COUNT == COUNT_PER_WAVE ? (int)(DISPLAY_THREADS / WAVE) : 1;
    __shared__ uint32_t lds[SUBS * HIST_SLOTS];
    for (int k = (int)threadIdx.x; k < SUBS * HIST_SLOTS; k += (int)DISPLAY_THREADS) lds[k] = 0u;
    __syncthreads();
    uint32_t *mine = lds + (COUNT == COUNT_PER_WAVE ? (threadIdx.x / WAVE) * HIST_SLOTS : 0u);
    const uint64_t stride = (uint64_t)gridDim.x * DISPLAY_THREADS, t = (uint64_t)blockIdx.x * DISPLAY_THREADS + threadIdx.x;
    for (uint64_t q = t; q < n_quads; q += stride) {
        const float4 *p = (const float4 *)(in + 12 * q);
        const float4 a = p[0], b = p[1], c = p[2];
        histogram_add<COUNT>(mine, histogram_slot(a.x, a.y, a.z));
        histogram_add<COUNT>(mine, histogram_slot(a.w, b.x, b.y));
        histogram_add<COUNT>(mine, histogram_slot(b.z, b.w, c.x));
        histogram_add<COUNT>(mine, histogram_slot(c.y, c.z, c.w));
    }
    for (uint64_t p = 4 * n_quads + t; p < n_pixels; p += stride)
        histogram_add<COUNT>(mine, histogram_slot(in[3 * p], in[3 * p + 1], in[3 * p + 2]));
    __syncthreads();
    for (int k = (int)threadIdx.x; k < HIST_SLOTS; k += (int)DISPLAY_THREADS) {
        uint32_t v = 0;
        for (int s = 0; s < SUBS; s++) v += lds[s * HIST_SLOTS + k];
        if (v) atomicAdd(&g[k], v);
    }
}

struct __attribute__((aligned(4))) Bytes12 { uint32_t a, b, c; };

// Thread t < n_quads takes pixels 4 t .. 4 t + 3 (n_quads is 0 when a pointer is not aligned for it); thread n_quads + k takes pixel
// 4 * n_quads + k by display_write, the host form's own loop body.
__global__ void __launch_bounds__(DISPLAY_THREADS) display_kernel(DisplayPlan pl, const float *in, void *out, uint64_t n_pixels, uint64_t n_quads) {
    const uint64_t t = (uint64_t)blockIdx.x * DISPLAY_THREADS + threadIdx.x;
    if (t >= n_quads) {
        const uint64_t p = 4 * n_quads + (t - n_quads);
        if (p < n_pixels) display_write(pl, in, out, (size_t)p);
        return;
    }
    const float4 *src = (const float4 *)(in + 12 * t);
    const float4 a = src[0], b = src[1], c = src[2];
    const float f[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
    float v[12];
#pragma unroll
    for (int k = 0; k < 4; k++) display_value(pl, f + 3 * k, v + 3 * k);
    if (pl.format == RTW_DISPLAY_F32) {
        float4 *dst = (float4 *)((float *)out + 12 * t);
        dst[0] = make_float4(v[0], v[1], v[2], v[3]);
        dst[1] = make_float4(v[4], v[5], v[6], v[7]);
        dst[2] = make_float4(v[8], v[9], v[10], v[11]);
        return;
    }
    uint32_t q[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float d = 0.0f;
        if (pl.dither) {                                                   // (i, j) only here
            const uint32_t p = 4u * (uint32_t)t + (uint32_t)k;             // (w * h fits 32 bits)
            d = display_dither(p % pl.w, p / pl.w);
        }
        for (int ch = 0; ch < 3; ch++) q[3 * k + ch] = display_byte(pl, v[3 * k + ch], d);
    }
    if (pl.format == RTW_DISPLAY_RGBA8) {
        uint4 o;
        o.x = q[0] | (q[1] << 8) | (q[2] << 16) | 0xFF000000u;
        o.y = q[3] | (q[4] << 8) | (q[5] << 16) | 0xFF000000u;
        o.z = q[6] | (q[7] << 8) | (q[8] << 16) | 0xFF000000u;
        o.w = q[9] | (q[10] << 8) | (q[11] << 16) | 0xFF000000u;
        *(uint4 *)((uint8_t *)out + 16 * t) = o;
    } else {
        Bytes12 o;
        o.a = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        o.b = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
        o.c = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
        *(Bytes12 *)((uint8_t *)out + 12 * t) = o;
    }
}

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

} // namespace

struct DisplayScratch {
    DevMem in, out;                                // a frame or a result whose buffer is host memory, staged
    DevMem slots;                                  // the histogram's HIST_SLOTS counters
    hipEvent_t ev[2] = { nullptr, nullptr };
    uint32_t cus = 0;                              // compute units of the context's GPU
};

void display_scratch_free(DisplayScratch *s) {
    if (!s) return;
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;                                      // (the buffers free themselves)
}

#define DISPLAY_TRY(expr)                                                                                                         \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; }                \
    } while (0)

namespace {

int scratch_get(int device, DisplayScratch **scratch, int *last_hip) {
    DISPLAY_TRY(hipSetDevice(device));
    if (*scratch) return RTW_OK;
    DisplayScratch *s = new (std::nothrow) DisplayScratch();
    if (!s) return RTW_E_NOMEM;
    *scratch = s;                                  // (owned by the context from here on, whatever follows)
    for (hipEvent_t &e : s->ev) DISPLAY_TRY(hipEventCreate(&e));
    int cus = 0;
    DISPLAY_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    s->cus = cus > 0 ? (uint32_t)cus : 1u;
    DISPLAY_TRY(s->slots.reserve(HIST_SLOTS * sizeof(uint32_t)));
    return RTW_OK;
}

} // namespace

int luminance_histogram_device(int device, hipStream_t stream, DisplayScratch **scratch, uint32_t count, const float *in, uint32_t w, uint32_t h,
                               uint32_t *hist, uint32_t *counts, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = histogram_check(in, w, h, hist, counts);
    if (rc != RTW_OK) return rc;
    if ((rc = scratch_get(device, scratch, last_hip)) != RTW_OK) return rc;
    DisplayScratch *s = *scratch;
    if (!s->slots.ptr || !s->ev[1] || !s->cus) return RTW_E_HIP;           // (a first call that failed half way)
    const uint64_t n = (uint64_t)w * h;
    if (!on_device(in, device)) {
        DISPLAY_TRY(s->in.reserve(n * 3 * sizeof(float)));
        DISPLAY_TRY(hipMemcpyAsync(s->in.ptr, in, n * 3 * sizeof(float), hipMemcpyDefault, stream));
        in = s->in.as<float>();
    }
    uint32_t *g = s->slots.as<uint32_t>();
    const uint64_t n_quads = aligned_to(in, 16) ? n / 4 : 0, items = n_quads + (n - 4 * n_quads);
    const uint64_t want = (items + DISPLAY_THREADS - 1) / DISPLAY_THREADS, cap = (uint64_t)s->cus * RTW_HISTOGRAM_BLOCKS_PER_CU;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    DISPLAY_TRY(hipMemsetAsync(g, 0, HIST_SLOTS * sizeof(uint32_t), stream));
    DISPLAY_TRY(hipEventRecord(s->ev[0], stream));
    switch (count ? (int)count : HIST_COUNT) {
    case COUNT_PLAIN:    hipLaunchKernelGGL(histogram_kernel<COUNT_PLAIN>, grid, dim3(DISPLAY_THREADS), 0, stream, in, n, n_quads, g); break;
    case COUNT_PER_WAVE: hipLaunchKernelGGL(histogram_kernel<COUNT_PER_WAVE>, grid, dim3(DISPLAY_THREADS), 0, stream, in, n, n_quads, g); break;
    default:             hipLaunchKernelGGL(histogram_kernel<COUNT_BALLOT>, grid, dim3(DISPLAY_THREADS), 0, stream, in, n, n_quads, g); break;
    }
    DISPLAY_TRY(hipGetLastError());
    DISPLAY_TRY(hipEventRecord(s->ev[1], stream));
    DISPLAY_TRY(hipMemcpyAsync(hist, g, HIST_BINS * sizeof(uint32_t), hipMemcpyDefault, stream));
    DISPLAY_TRY(hipMemcpyAsync(counts, g + HIST_BLACK, 2 * sizeof(uint32_t), hipMemcpyDefault, stream));
    DISPLAY_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, n };
    }
    return RTW_OK;
}

int display_device(int device, hipStream_t stream, DisplayScratch **scratch, const float *in, uint32_t w, uint32_t h, const RtwDisplay *p,
                   void *out, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    DisplayPlan pl;
    int rc = display_check(in, w, h, p, out, pl);
    if (rc != RTW_OK) return rc;
    if ((rc = scratch_get(device, scratch, last_hip)) != RTW_OK) return rc;
    DisplayScratch *s = *scratch;
    if (!s->ev[1]) return RTW_E_HIP;
    const uint64_t n = (uint64_t)w * h;
    const size_t in_bytes = n * 3 * sizeof(float), out_bytes = n * display_pixel_bytes(pl.format);
    if (!on_device(in, device)) {
        DISPLAY_TRY(s->in.reserve(in_bytes));
        DISPLAY_TRY(hipMemcpyAsync(s->in.ptr, in, in_bytes, hipMemcpyDefault, stream));
        in = s->in.as<float>();
    }
    void *host_out = nullptr;
    if (!on_device(out, device)) {
        DISPLAY_TRY(s->out.reserve(out_bytes));
        host_out = out;
        out = s->out.ptr;
    }
    const bool wide = aligned_to(in, 16) && aligned_to(out, pl.format == RTW_DISPLAY_RGB8 ? 4 : 16);
    const uint64_t n_quads = wide ? n / 4 : 0, threads = n_quads + (n - 4 * n_quads);
    const dim3 grid((unsigned)((threads + DISPLAY_THREADS - 1) / DISPLAY_THREADS));
    DISPLAY_TRY(hipEventRecord(s->ev[0], stream));
    hipLaunchKernelGGL(display_kernel, grid, dim3(DISPLAY_THREADS), 0, stream, pl, in, out, n, n_quads);
    DISPLAY_TRY(hipGetLastError());
    DISPLAY_TRY(hipEventRecord(s->ev[1], stream));
    if (host_out) DISPLAY_TRY(hipMemcpyAsync(host_out, out, out_bytes, hipMemcpyDefault, stream));
    DISPLAY_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, n };
    }
    return RTW_OK;
}
#undef DISPLAY_TRY

} // namespace rtw
