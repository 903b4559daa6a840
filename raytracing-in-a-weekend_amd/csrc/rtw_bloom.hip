// rtw_bloom.hip -- bloom (rtw_bloom.h) on the GPU: the device path of rtw_ctx_bloom.
//
// 2 n launches for n levels used: n down steps (the first reads the frame through the bright pass), n - 1 up steps in place over the down
// chain, and the composite.  Every kernel is one thread per OUTPUT pixel in workgroups of 16 x 16 pixels, each running bloom_down_pixel /
// bloom_up_value -- the host form's definitions on the host form's plan, so its bytes.  As in the other window passes the source window comes
// from one of two places:
//   * tile (RTW_OPT_ATROUS_LAYOUT 1): the workgroup's window of the source level in LDS, loaded cooperatively, one plane per channel.
//     Down: 36 x 36 entries from (2 I0 - 2, 2 J0 - 2).  A lane's taps are at columns 2 tx + a, so a row of 16 lanes strides by two entries: the
//     even and the odd columns of a tile row are kept apart (18 entries each, the odd ones 20 floats behind the even ones) and a tile row is
//     40 floats, so that for each tap the 16 lanes of a row read 16 consecutive floats and the next row of lanes (two tile rows on: 80 floats,
//     16 banks of the 32 a ds_read_b32 sees) the other 16: by that bank rule no bank is read twice by the 32 lanes that share a cycle (by
//     construction; no conflict counter was collected, and the split was not measured against a plain padded tile).  The first step keeps the
//     bright pass's result, b and kw (4 planes, 23 040 bytes; the other steps 3 planes, 17 280 bytes): the same operations on the same
//     operands as a tap's own bright pass, so the same bits, one bright pass an entry in place of nine a pixel of the frame.
//     Up and composite: 12 x 12 entries from the footprint of the workgroup's first pixel (1728 bytes); neighbouring lanes read the same
//     entry or the next one.
//   * direct (2): every tap is read from global memory (the first step runs the bright pass for each tap); the reuse is the caches'.
// 0 takes what was measured: the tile, which was ahead in every kernel at every level size (bloom_tile below; profiles/bloom.log).
// An entry of a tile outside its level is not a tap: what keeps it out is the inside test of the step, which the host form and the direct
// kernels need anyway; such an entry is filled with zeros and, in the first step, flagged not usable besides.
#include "rtw_bloom_dev.h"
#include "rtw_bloom.h"
#include "rtw_devmem.h"

#include <chrono>
#include <new>

namespace rtw {
namespace {

constexpr int BB = 16;                             // a workgroup is BB x BB output pixels
constexpr int DOWN_TILE = 2 * BB + 4;              // 36: entries of a down window along a side
constexpr int DOWN_ODD = 20, DOWN_PITCH = 40;      // floats from a tile row's even columns to its odd ones, and to the next row
constexpr int DOWN_PLANE = DOWN_TILE * DOWN_PITCH;
constexpr int UP_TILE = 12;                        // 16 fine pixels reach 8 m - 2 .. 8 m + 9
constexpr int UP_PLANE = UP_TILE * UP_TILE;
static_assert(DOWN_TILE / 2 <= DOWN_ODD && DOWN_ODD + DOWN_TILE / 2 <= DOWN_PITCH && (2 * DOWN_PITCH) % 32 == 16, "the down tile's banks");

struct BloomDownArgs {
    const float *src;                              // level l (the frame when FIRST)
    float *dst;                                    // level l + 1
    int sw, sh, dw, dh;
    uint32_t tiles_x;
    float threshold, knee;
    uint32_t karis;
};

template <bool FIRST>
struct BloomDownTileSrc {
    const float *p;
    int ox, oy, w, h;
    __device__ bool inside(int x, int y) const { return x >= 0 && y >= 0 && x < w && y < h; }
    __device__ static int at(int ex, int ey) { return ey * DOWN_PITCH + (ex & 1) * DOWN_ODD + (ex >> 1); }
    __device__ BloomTap tap(int x, int y) const {
        const int e = at(x - ox, y - oy);
        return BloomTap{ { p[e], p[DOWN_PLANE + e], p[2 * DOWN_PLANE + e] }, FIRST ? p[3 * DOWN_PLANE + e] : 1.0f };
    }
};

// Workgroup b covers the 16 x 16 pixels of level l + 1 of tile (b % tiles_x, b / tiles_x).
template <bool FIRST, bool TILE>
__global__ void __launch_bounds__(BB * BB) bloom_down_kernel(BloomDownArgs a) {
    __shared__ float smem[TILE ? (FIRST ? 4 : 3) * DOWN_PLANE : 1];
    const int tx = (int)(threadIdx.x % BB), ty = (int)(threadIdx.x / BB);
    const int I0 = (int)(blockIdx.x % a.tiles_x) * BB, J0 = (int)(blockIdx.x / a.tiles_x) * BB;
    const int I = I0 + tx, J = J0 + ty;
    const bool mine = I < a.dw && J < a.dh;
    const BloomFrameSrc fs = { a.src, a.sw, a.sh, a.threshold, a.knee, a.karis };
    const BloomMemSrc ms = { a.src, a.sw, a.sh };
    float o[3];
    if (TILE) {
        const int ox = 2 * I0 - 2, oy = 2 * J0 - 2;
        for (int i = (int)threadIdx.x; i < DOWN_TILE * DOWN_TILE; i += BB * BB) {
            const int ex = i % DOWN_TILE, ey = i / DOWN_TILE;
            BloomTap t = { { 0.0f, 0.0f, 0.0f }, -1.0f };
            if (ms.inside(ox + ex, oy + ey)) t = FIRST ? fs.tap(ox + ex, oy + ey) : ms.tap(ox + ex, oy + ey);
            const int e = BloomDownTileSrc<FIRST>::at(ex, ey);
            smem[e] = t.v[0]; smem[DOWN_PLANE + e] = t.v[1]; smem[2 * DOWN_PLANE + e] = t.v[2];
            if (FIRST) smem[3 * DOWN_PLANE + e] = t.kw;
        }
        __syncthreads();
        if (!mine) return;
        const BloomDownTileSrc<FIRST> ts = { smem, ox, oy, a.sw, a.sh };
        (void)bloom_down_pixel(ts, I, J, o);
    } else {
        if (!mine) return;
        if (FIRST) (void)bloom_down_pixel(fs, I, J, o); else (void)bloom_down_pixel(ms, I, J, o);
    }
    float *q = a.dst + 3 * ((size_t)J * (size_t)a.dw + (size_t)I);
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
}

struct BloomUpArgs {
    const float *coarse;                           // level l + 1
    int cw, ch;
    float *fine;                                   // an up step: level l, in place
    const float *in;                               // the composite: the frame, the result and the layer (may be NULL)
    float *out, *layer;
    int fw, fh;
    uint32_t tiles_x;
    float k;                                       // spread, or the composite's intensity
};

struct BloomUpTileSrc {
    const float *p;
    int ox, oy, w, h;
    __device__ bool inside(int x, int y) const { return x >= 0 && y >= 0 && x < w && y < h; }
    __device__ BloomTap tap(int x, int y) const {
        const int e = (y - oy) * UP_TILE + (x - ox);
        return BloomTap{ { p[e], p[UP_PLANE + e], p[2 * UP_PLANE + e] }, 1.0f };
    }
};

// Workgroup b covers the 16 x 16 pixels of the finer level of tile (b % tiles_x, b / tiles_x).
template <bool COMPOSITE, bool TILE>
__global__ void __launch_bounds__(BB * BB) bloom_up_kernel(BloomUpArgs a) {
    __shared__ float smem[TILE ? 3 * UP_PLANE : 1];
    const int tx = (int)(threadIdx.x % BB), ty = (int)(threadIdx.x / BB);
    const int x0 = (int)(blockIdx.x % a.tiles_x) * BB, y0 = (int)(blockIdx.x / a.tiles_x) * BB;
    const int i = x0 + tx, j = y0 + ty;
    const bool mine = i < a.fw && j < a.fh;
    const BloomMemSrc ms = { a.coarse, a.cw, a.ch };
    float u[3];
    if (TILE) {
        int wt_[4];
        const int ox = bloom_up_foot(x0, wt_), oy = bloom_up_foot(y0, wt_);
        if ((int)threadIdx.x < UP_PLANE) {
            const int ex = (int)threadIdx.x % UP_TILE, ey = (int)threadIdx.x / UP_TILE;
            BloomTap t = { { 0.0f, 0.0f, 0.0f }, 1.0f };
            if (ms.inside(ox + ex, oy + ey)) t = ms.tap(ox + ex, oy + ey);
            smem[threadIdx.x] = t.v[0]; smem[UP_PLANE + threadIdx.x] = t.v[1]; smem[2 * UP_PLANE + threadIdx.x] = t.v[2];
        }
        __syncthreads();
        if (!mine) return;
        const BloomUpTileSrc ts = { smem, ox, oy, a.cw, a.ch };
        (void)bloom_up_value(ts, i, j, u);
    } else {
        if (!mine) return;
        (void)bloom_up_value(ms, i, j, u);
    }
    const size_t p = 3 * ((size_t)j * (size_t)a.fw + (size_t)i);
    if (COMPOSITE) {
        for (int c = 0; c < 3; c++) a.out[p + c] = a.in[p + c] + a.k * u[c];
        if (a.layer) for (int c = 0; c < 3; c++) a.layer[p + c] = u[c];
    } else {
        for (int c = 0; c < 3; c++) a.fine[p + c] = a.fine[p + c] + a.k * u[c];
    }
}

// Does a launch read its window from an LDS tile?  RTW_OPT_ATROUS_LAYOUT 0: the tile, in every kernel at every level size.
// profiles/bloom.log section (d), 1920 x 1080, 8 levels, kernel times of a trace, tile against global memory: the first down step 0.022
// against 0.043 ms, the composite 0.019 against 0.030 ms, the other down steps ahead by 8 .. 33 % from 480 x 270 to 8 x 5, the up steps by
// 0 .. 25 % (the smallest within 0.0001 ms of global memory, level from run to run).  The tile loses nowhere, so neither the kernel nor
// the size enters the choice.
bool bloom_tile(uint32_t layout) { return layout != 2; }

float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

uint32_t tiles(uint32_t n) { return (n + BB - 1) / BB; }

} // namespace

struct BloomScratch {
    DevMem in, out, layer;                         // a frame or a result whose buffer is host memory, staged
    DevMem pyr;                                    // levels 1 .. n of the call, one behind the other
    hipEvent_t ev[2] = { nullptr, nullptr };
};

void bloom_scratch_free(BloomScratch *s) {
    if (!s) return;
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;                                      // (the buffers free themselves)
}

#define BLOOM_TRY(expr)                                                                                                           \
    do {                                                                                                                          \
        hipError_t e_ = (expr);                                                                                                   \
        if (e_ != hipSuccess) { *last_hip = (int)e_; return e_ == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP; }                \
    } while (0)

int bloom_device(int device, hipStream_t stream, BloomScratch **scratch, uint32_t layout, const float *in, uint32_t w, uint32_t h,
                 const RtwBloom *p, float *out, float *layer_out, RtwFilterStats *stats, int *last_hip) {
    const auto t0 = std::chrono::steady_clock::now();
    BloomPlan pl;
    const int rc = bloom_check(in, w, h, p, out, layer_out, pl);
    if (rc != RTW_OK) return rc;
    BLOOM_TRY(hipSetDevice(device));
    if (!*scratch) {
        BloomScratch *s = new (std::nothrow) BloomScratch();
        if (!s) return RTW_E_NOMEM;
        *scratch = s;                              // (owned by the context from here on, whatever follows)
        for (hipEvent_t &e : s->ev) BLOOM_TRY(hipEventCreate(&e));
    }
    BloomScratch *s = *scratch;
    if (!s->ev[1]) return RTW_E_HIP;               // (a first call that failed half way)
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    if (!on_device(in, device)) {
        BLOOM_TRY(s->in.reserve(bytes));
        BLOOM_TRY(hipMemcpyAsync(s->in.ptr, in, bytes, hipMemcpyDefault, stream));
        in = s->in.as<float>();
    }
    float *host_out = nullptr, *host_layer = nullptr;
    if (!on_device(out, device)) {
        BLOOM_TRY(s->out.reserve(bytes));
        host_out = out;
        out = s->out.as<float>();
    }
    if (layer_out && !on_device(layer_out, device)) {
        BLOOM_TRY(s->layer.reserve(bytes));
        host_layer = layer_out;
        layer_out = s->layer.as<float>();
    }
    BLOOM_TRY(s->pyr.reserve(pl.off[pl.n + 1] * sizeof(float)));
    float *pyr = s->pyr.as<float>();

    const bool tile = bloom_tile(layout);
    BLOOM_TRY(hipEventRecord(s->ev[0], stream));
    for (uint32_t l = 0; l < pl.n; l++) {
        const BloomDownArgs a = { l ? pyr + pl.off[l] : in, pyr + pl.off[l + 1], (int)pl.lw[l], (int)pl.lh[l], (int)pl.lw[l + 1], (int)pl.lh[l + 1],
                                  tiles(pl.lw[l + 1]), pl.threshold, pl.knee, pl.karis };
        const dim3 grid((unsigned)((uint64_t)a.tiles_x * tiles(pl.lh[l + 1])));
        if (l == 0) {
            if (tile) hipLaunchKernelGGL((bloom_down_kernel<true, true>), grid, dim3(BB * BB), 0, stream, a);
            else      hipLaunchKernelGGL((bloom_down_kernel<true, false>), grid, dim3(BB * BB), 0, stream, a);
        } else {
            if (tile) hipLaunchKernelGGL((bloom_down_kernel<false, true>), grid, dim3(BB * BB), 0, stream, a);
            else      hipLaunchKernelGGL((bloom_down_kernel<false, false>), grid, dim3(BB * BB), 0, stream, a);
        }
        BLOOM_TRY(hipGetLastError());
    }
    for (uint32_t l = pl.n - 1; l >= 1; l--) {
        const BloomUpArgs a = { pyr + pl.off[l + 1], (int)pl.lw[l + 1], (int)pl.lh[l + 1], pyr + pl.off[l], nullptr, nullptr, nullptr,
                                (int)pl.lw[l], (int)pl.lh[l], tiles(pl.lw[l]), pl.spread };
        const dim3 grid((unsigned)((uint64_t)a.tiles_x * tiles(pl.lh[l])));
        if (tile)
            hipLaunchKernelGGL((bloom_up_kernel<false, true>), grid, dim3(BB * BB), 0, stream, a);
        else
            hipLaunchKernelGGL((bloom_up_kernel<false, false>), grid, dim3(BB * BB), 0, stream, a);
        BLOOM_TRY(hipGetLastError());
    }
    {
        const BloomUpArgs a = { pyr + pl.off[1], (int)pl.lw[1], (int)pl.lh[1], nullptr, in, out, layer_out, (int)w, (int)h, tiles(w), pl.intensity };
        const dim3 grid((unsigned)((uint64_t)a.tiles_x * tiles(h)));
        if (tile)
            hipLaunchKernelGGL((bloom_up_kernel<true, true>), grid, dim3(BB * BB), 0, stream, a);
        else
            hipLaunchKernelGGL((bloom_up_kernel<true, false>), grid, dim3(BB * BB), 0, stream, a);
        BLOOM_TRY(hipGetLastError());
    }
    BLOOM_TRY(hipEventRecord(s->ev[1], stream));
    if (host_out) BLOOM_TRY(hipMemcpyAsync(host_out, out, bytes, hipMemcpyDefault, stream));
    if (host_layer) BLOOM_TRY(hipMemcpyAsync(host_layer, layer_out, bytes, hipMemcpyDefault, stream));
    BLOOM_TRY(hipStreamSynchronize(stream));
    if (stats) {
        const float total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, event_ms(s->ev[0], s->ev[1]), total, bloom_taps(pl) };
    }
    return RTW_OK;
}
#undef BLOOM_TRY

} // namespace rtw
