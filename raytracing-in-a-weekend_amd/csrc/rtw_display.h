// rtw_display.h -- the display stage (include/rtw.h "display stage"): the luminance histogram's bin rule and the display
// transform's per-pixel rule, written once as __host__ __device__ for the host forms (rtw_display.cpp) and the kernels (rtw_display.hip).
// f32, one rounding per written operation under -ffp-contract=off, correctly rounded divides, pow_plain (rtw_mixed.h) the only elementary
// function, no ocml call: the rounding to a byte is written out too (display_round below), since what std::round becomes differs per side.
#pragma once
#include "rtw.h"
#include "rtw_mixed.h"

namespace rtw {

// ---- the luminance histogram -----------------------------------------------------------------------------------------------------------
constexpr int HIST_BINS = 256;
constexpr int HIST_BLACK = 256, HIST_NON_FINITE = 257;     // the two counts, as slots behind the bins
constexpr int HIST_SLOTS = 258;

__host__ __device__ __forceinline__ bool display_finite(float x) { return (mx_float_to_bits(x) & 0x7F800000u) != 0x7F800000u; }

__host__ __device__ __forceinline__ float display_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The slot of one pixel: its bin 0 .. 255, HIST_BLACK or HIST_NON_FINITE.  With finite channels every product is finite (the weights are
// below 1) and so is the first sum, so Y is never NaN; it can overflow to +inf (non-finite) or to -inf (<= 0: black).
__host__ __device__ __forceinline__ int histogram_slot(float r, float g, float b) {
    if (!(display_finite(r) && display_finite(g) && display_finite(b))) return HIST_NON_FINITE;
    const float y = display_luma(r, g, b);
    if (y != y || y == __builtin_inff()) return HIST_NON_FINITE;
    if (y <= 0.0f) return HIST_BLACK;
    const int bin = (int)(mx_float_to_bits(y) >> 20) - 888;                // exponent and three mantissa bits; 888 = 8 * (127 - 16)
    return bin < 0 ? 0 : (bin > 255 ? 255 : bin);
}

// ---- the display transform ---------------------------------------------------------------------------------------------------------------
// RtwDisplay as the per-pixel rule wants it: display_check (rtw_display.cpp) fills it on the host, once, for both forms.
struct DisplayPlan {
    uint32_t w = 0, h = 0;
    float exposure = 1.0f;
    uint32_t tone = RTW_TONE_NONE;
    float ww = 1.0f;                 // white * white
    uint32_t transfer = RTW_TRANSFER_GAMMA;
    float inv_gamma = 1.0f;          // 1.0f / gamma
    float scale = 255.0f;            // 255.0f (RUST) or 255.99f (RUST2)
    uint32_t dither = 0;
    uint32_t format = RTW_DISPLAY_RGB8;
};

constexpr float SRGB_KNEE = 0.0031308f;
constexpr float SRGB_EXP = 0.4166666567325592f;                            // 1.0f / 2.4f, the nearest f32 to 1 / 2.4

// B[j & 7][i & 7], the 8 x 8 Bayer matrix (include/rtw.h writes it out).
__host__ __device__ __forceinline__ float display_dither(uint32_t i, uint32_t j) {
    constexpr uint8_t B[64] = {  0, 32,  8, 40,  2, 34, 10, 42,
                                48, 16, 56, 24, 50, 18, 58, 26,
                                12, 44,  4, 36, 14, 46,  6, 38,
                                60, 28, 52, 20, 62, 30, 54, 22,
                                 3, 35, 11, 43,  1, 33,  9, 41,
                                51, 19, 59, 27, 49, 17, 57, 25,
                                15, 47,  7, 39, 13, 45,  5, 37,
                                63, 31, 55, 23, 61, 29, 53, 21 };
    return ((float)B[(j & 7u) * 8u + (i & 7u)] + 0.5f) * 0.015625f;
}

__host__ __device__ __forceinline__ float display_reinhard(float x, float ww) { return (x * (1.0f + x / ww)) / (1.0f + x); }

__host__ __device__ __forceinline__ float display_clamp(float v, float hi) { return v != v ? v : (v < 0.0f ? 0.0f : (v > hi ? hi : v)); }

// Steps 3 and 4 of one channel: clamp to [0, 1], then the transfer function.
__host__ __device__ __forceinline__ float display_transfer(const DisplayPlan &pl, float v) {
    v = display_clamp(v, 1.0f);
    if (pl.transfer == RTW_TRANSFER_SRGB) return v <= SRGB_KNEE ? 12.92f * v : 1.055f * pow_plain(v, SRGB_EXP) - 0.055f;
    return pl.inv_gamma == 1.0f ? v : pow_plain(v, pl.inv_gamma);
}

// Steps 1 to 4 of one pixel: in[3] -> v[3].
__host__ __device__ __forceinline__ void display_value(const DisplayPlan &pl, const float in[3], float v[3]) {
    float x[3];
    for (int c = 0; c < 3; c++) x[c] = in[c] * pl.exposure;
    if (pl.tone == RTW_TONE_REINHARD) {
        for (int c = 0; c < 3; c++) v[c] = display_reinhard(x[c], pl.ww);
    } else if (pl.tone == RTW_TONE_REINHARD_LUMA) {
        const float y = display_luma(x[0], x[1], x[2]);
        if (y > 0.0f) {
            const float k = display_reinhard(y, pl.ww) / y;
            for (int c = 0; c < 3; c++) v[c] = x[c] * k;
        } else {
            for (int c = 0; c < 3; c++) v[c] = x[c];
        }
    } else if (pl.tone == RTW_TONE_ACES_FIT) {
        for (int c = 0; c < 3; c++) v[c] = (x[c] * (2.51f * x[c] + 0.03f)) / (x[c] * (2.43f * x[c] + 0.59f) + 0.14f);
    } else {
        for (int c = 0; c < 3; c++) v[c] = x[c];
    }
    for (int c = 0; c < 3; c++) v[c] = display_transfer(pl, v[c]);
}

// Step 5 for a byte.  Without dither the rule of rtw_quantize_u8 / rtw_quantize_u8_rust2: scale, clamp to [0, 255] (a NaN propagates), round
// half away from zero, NaN -> 0.  t is in [0, 255], so t - (float)(int)t is exact and the comparison is f32::round's.  With dither d in
// (0, 1):  floor(t + d), at most 255.
__host__ __device__ __forceinline__ uint32_t display_byte(const DisplayPlan &pl, float v, float d) {
    const float t = display_clamp(v * pl.scale, 255.0f);
    if (t != t) return 0u;
    if (pl.dither) {
        const uint32_t b = (uint32_t)(int)(t + d);                         // t + d >= 0: the conversion's truncation is floorf
        return b > 255u ? 255u : b;
    }
    const float f = (float)(int)t;
    return (uint32_t)(int)(t - f >= 0.5f ? f + 1.0f : f);
}

// One pixel, p = j * w + i, into `out` in the plan's format: what the host form runs for every pixel and the kernel on its scalar path.
__host__ __device__ __forceinline__ void display_write(const DisplayPlan &pl, const float *in, void *out, size_t p) {
    float v[3];
    display_value(pl, in + 3 * p, v);
    if (pl.format == RTW_DISPLAY_F32) {
        float *o = (float *)out + 3 * p;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
        return;
    }
    const float d = pl.dither ? display_dither((uint32_t)p % pl.w, (uint32_t)p / pl.w) : 0.0f;         // (w * h fits 32 bits)
    const int stride = pl.format == RTW_DISPLAY_RGBA8 ? 4 : 3;
    uint8_t *o = (uint8_t *)out + (size_t)stride * p;
    for (int c = 0; c < 3; c++) o[c] = (uint8_t)display_byte(pl, v[c], d);
    if (stride == 4) o[3] = 255;
}

__host__ __device__ inline size_t display_pixel_bytes(uint32_t format) {
    return format == RTW_DISPLAY_F32 ? 12u : (format == RTW_DISPLAY_RGBA8 ? 4u : 3u);
}

// The argument checks both forms share (rtw_display.cpp).
int histogram_check(const float *in, uint32_t w, uint32_t h, const uint32_t *hist, const uint32_t *counts);
int display_check(const float *in, uint32_t w, uint32_t h, const RtwDisplay *p, const void *out, DisplayPlan &pl);

} // namespace rtw
