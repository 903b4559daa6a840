// rtw_bloom.h -- bloom (include/rtw.h "bloom"): the bright pass, the 36-weight down step, the 16-weight up step and the
// composite, written once as __host__ __device__ for the host form (rtw_bloom.cpp) and the kernels (rtw_bloom.hip).  f32, one rounding per
// written operation under -ffp-contract=off, correctly rounded divides, no elementary function.  A step reads its source level through a
// `Src` (inside / tap): global memory on the host and in the direct kernels, the workgroup's LDS tile in the tile kernels.
#pragma once
#include "rtw.h"
#include "rtw_display.h"

namespace rtw {

// RtwBloom as the steps want it: bloom_check (rtw_bloom.cpp) fills it on the host, once, for both forms.
struct BloomPlan {
    uint32_t w = 0, h = 0;
    uint32_t n = 0;                                  // levels used, 1 .. RTW_BLOOM_MAX_LEVELS
    uint32_t lw[RTW_BLOOM_MAX_LEVELS + 1] = { 0 };   // lw[l] x lh[l]: level l, 0 .. n (level 0 is the frame)
    uint32_t lh[RTW_BLOOM_MAX_LEVELS + 1] = { 0 };
    size_t off[RTW_BLOOM_MAX_LEVELS + 2] = { 0 };    // level l = 1 .. n starts at float off[l] of the pyramid; off[n + 1]: its floats
    float threshold = 0.0f, knee = 0.0f;
    uint32_t karis = 0;
    float spread = 0.0f, intensity = 0.0f;
};

// The sizes of the chain: level l + 1 is the ceiling of half of level l; it stops at `levels` or at the first 1 x 1 level.
__host__ __device__ inline uint32_t bloom_chain(uint32_t w, uint32_t h, uint32_t levels, uint32_t *lw, uint32_t *lh) {
    uint32_t n = 0;
    lw[0] = w; lh[0] = h;
    while (n < levels) {
        lw[n + 1] = (lw[n] + 1u) / 2u;
        lh[n + 1] = (lh[n] + 1u) / 2u;
        n++;
        if (lw[n] == 1u && lh[n] == 1u) break;
    }
    return n;
}

// One tap of a down step: the value and the factor on its table weight.  kw < 0: not a tap (a pixel of the frame that is not usable).
struct BloomTap { float v[3]; float kw; };

// The knee: the quadratic between s = -knee and s = knee, max(s, 0) outside.
__host__ __device__ __forceinline__ float bloom_knee(float s, float knee) {
    return (knee > 0.0f && s > -knee && s < knee) ? ((s + knee) * (s + knee)) / (4.0f * knee) : (s > 0.0f ? s : 0.0f);
}

// The bright pass of one pixel of the frame.
__host__ __device__ __forceinline__ BloomTap bloom_bright(float threshold, float knee, uint32_t karis, float r, float g, float b) {
    BloomTap t = { { 0.0f, 0.0f, 0.0f }, -1.0f };
    if (!(display_finite(r) && display_finite(g) && display_finite(b))) return t;
    const float x[3] = { r < 0.0f ? 0.0f : r, g < 0.0f ? 0.0f : g, b < 0.0f ? 0.0f : b };
    const float y = display_luma(x[0], x[1], x[2]);
    const float c = bloom_knee(y - threshold, knee);
    if (y > 0.0f) {
        const float k = c / y;
        for (int ch = 0; ch < 3; ch++) t.v[ch] = x[ch] * k;
    }
    t.kw = karis ? 1.0f / (1.0f + display_luma(t.v[0], t.v[1], t.v[2])) : 1.0f;
    return t;
}

// D[b + 2][a + 2]: Jimenez' 13 bilinear taps (a centre box at 1/2, four corner boxes at 1/8) as the 36 pixel weights they amount to, in 1/128.
__host__ __device__ __forceinline__ float bloom_down_weight(int a, int b) {
    constexpr uint8_t D[36] = { 1, 1, 2, 2, 1, 1,
                                1, 5, 6, 6, 5, 1,
                                2, 6, 8, 8, 6, 2,
                                2, 6, 8, 8, 6, 2,
                                1, 5, 6, 6, 5, 1,
                                1, 1, 2, 2, 1, 1 };
    return (float)D[(b + 2) * 6 + (a + 2)] / 128.0f;
}

// Pixel (I, J) of level l + 1 from level l behind `src`.  Returns the taps inside level l.
template <class Src>
__host__ __device__ __forceinline__ uint32_t bloom_down_pixel(const Src &src, int I, int J, float out[3]) {
    float sum[3] = { 0.0f, 0.0f, 0.0f }, wsum = 0.0f;
    uint32_t taps = 0;
#pragma unroll
    for (int b = -2; b <= 3; b++) {
#pragma unroll
        for (int a = -2; a <= 3; a++) {
            const int x = 2 * I + a, y = 2 * J + b;
            if (!src.inside(x, y)) continue;
            taps++;
            const BloomTap t = src.tap(x, y);
            if (t.kw < 0.0f) continue;
            const float wt = bloom_down_weight(a, b) * t.kw;
            for (int c = 0; c < 3; c++) sum[c] = sum[c] + t.v[c] * wt;
            wsum = wsum + wt;
        }
    }
    for (int c = 0; c < 3; c++) out[c] = wsum > 0.0f ? sum[c] / wsum : 0.0f;
    return taps;
}

// The footprint of fine coordinate i on the coarser level: its first column (of four) and the four weights, in 1/16.  The rule's
// N = 2i - 1, I0 = floor(N / 4), r = N - 4 I0 without forming N, which does not fit an int beyond i = 2^30: i = 2m gives N = 4m - 1, so
// I0 = m - 1 and r = 3; i = 2m + 1 gives N = 4m + 1, so I0 = m and r = 1.
__host__ __device__ __forceinline__ int bloom_up_foot(int i, int wt[4]) {
    const int odd = i & 1, i0 = (i >> 1) - 1 + odd;                        // -1 at i = 0
    if (odd) { wt[0] = 3; wt[1] = 7; wt[2] = 5; wt[3] = 1; }               // r == 1
    else     { wt[0] = 1; wt[1] = 5; wt[2] = 7; wt[3] = 3; }               // r == 3
    return i0 - 1;
}

// U(coarse, (i, j)): a 3 x 3 tent on the coarse level, then the bilinear fetch at the fine pixel's centre, multiplied out.
template <class Src>
__host__ __device__ __forceinline__ uint32_t bloom_up_value(const Src &src, int i, int j, float u[3]) {
    int wx[4], wy[4];
    const int x0 = bloom_up_foot(i, wx), y0 = bloom_up_foot(j, wy);
    float sum[3] = { 0.0f, 0.0f, 0.0f }, wsum = 0.0f;
    uint32_t taps = 0;
#pragma unroll
    for (int ky = 0; ky < 4; ky++) {
#pragma unroll
        for (int kx = 0; kx < 4; kx++) {
            const int x = x0 + kx, y = y0 + ky;
            if (!src.inside(x, y)) continue;
            taps++;
            const BloomTap t = src.tap(x, y);
            const float wt = (float)(wx[kx] * wy[ky]) / 256.0f;
            for (int c = 0; c < 3; c++) sum[c] = sum[c] + t.v[c] * wt;
            wsum = wsum + wt;
        }
    }
    for (int c = 0; c < 3; c++) u[c] = sum[c] / wsum;                       // wsum > 0: the covering coarse pixel is tap 1 or 2
    return taps;
}

// A level in memory, [h][w][3].
struct BloomMemSrc {
    const float *p;
    int w, h;
    __host__ __device__ bool inside(int x, int y) const { return x >= 0 && y >= 0 && x < w && y < h; }
    __host__ __device__ BloomTap tap(int x, int y) const {
        const float *q = p + 3 * ((size_t)y * (size_t)w + (size_t)x);
        return BloomTap{ { q[0], q[1], q[2] }, 1.0f };
    }
};

// The frame in memory, as the first down step reads it: every tap through the bright pass.
struct BloomFrameSrc {
    const float *p;
    int w, h;
    float threshold, knee;
    uint32_t karis;
    __host__ __device__ bool inside(int x, int y) const { return x >= 0 && y >= 0 && x < w && y < h; }
    __host__ __device__ BloomTap tap(int x, int y) const {
        const float *q = p + 3 * ((size_t)y * (size_t)w + (size_t)x);
        return bloom_bright(threshold, knee, karis, q[0], q[1], q[2]);
    }
};

// The taps inside their level over all the steps of a call, in closed form: a step's count factors into columns x rows.
// bloom_side_taps: the sum over the output coordinates 0 .. n_out - 1 of a side of their taps inside [0, n_src).  A down coordinate k reads
// 2k - 2 .. 2k + 3 of n_src = 2 n_out or 2 n_out - 1, an up coordinate k the four from floor((2k - 1) / 4) - 1 of n_src = ceil(n_out / 2):
// from k = 4 on neither reaches below 0, and up to k = n_out - 5 neither reaches n_src (2k + 3 <= 2 n_out - 7; floor((2k - 1) / 4) + 2 <=
// n_out / 2 - 3 / 4).  So only the first and the last BLOOM_EDGE = 4 coordinates are counted tap by tap; the ones between have all.
constexpr uint32_t BLOOM_EDGE = 4;
inline uint64_t bloom_side_taps(uint32_t n_out, uint32_t n_src, bool down) {
    const uint32_t all = down ? 6u : 4u;
    const auto inside = [&](uint32_t k) {
        int wt[4];
        const int64_t lo = down ? 2 * (int64_t)k - 2 : (int64_t)bloom_up_foot((int)k, wt);
        uint64_t n = 0;
        for (uint32_t t = 0; t < all; t++) n += (lo + t >= 0 && lo + t < (int64_t)n_src) ? 1u : 0u;
        return n;
    };
    uint64_t total = 0;
    if (n_out <= 2 * BLOOM_EDGE) {
        for (uint32_t k = 0; k < n_out; k++) total += inside(k);
        return total;
    }
    for (uint32_t k = 0; k < BLOOM_EDGE; k++) total += inside(k) + inside(n_out - 1 - k);
    return total + (uint64_t)(n_out - 2 * BLOOM_EDGE) * all;
}
inline uint64_t bloom_taps(const BloomPlan &pl) {
    uint64_t taps = 0;
    for (uint32_t l = 0; l < pl.n; l++) {
        taps += bloom_side_taps(pl.lw[l + 1], pl.lw[l], true) * bloom_side_taps(pl.lh[l + 1], pl.lh[l], true);   // down l -> l + 1
        taps += bloom_side_taps(pl.lw[l], pl.lw[l + 1], false) * bloom_side_taps(pl.lh[l], pl.lh[l + 1], false); // up / composite l + 1 -> l
    }
    return taps;
}

// The argument checks both forms share (rtw_bloom.cpp).
int bloom_check(const float *in, uint32_t w, uint32_t h, const RtwBloom *p, const float *out, const float *layer_out, BloomPlan &pl);

} // namespace rtw
