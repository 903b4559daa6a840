// rtw_display.cpp -- the host forms of the display stage (rtw_luminance_histogram, rtw_exposure_from_histogram, rtw_display; include/rtw.h)
// and the argument checks they share with the device path (rtw_display.hip).  Pure host code: no HIP call.  One thread over the pixels, each
// running histogram_slot / display_write (rtw_display.h), which the kernels run too.
#include "rtw_display.h"

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>

namespace rtw {

namespace {

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

int size_check(uint32_t w, uint32_t h) {
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (w > RTW_ATROUS_MAX_SIDE || h > RTW_ATROUS_MAX_SIDE) return RTW_E_INVALID;
    return RTW_OK;
}

} // namespace

int histogram_check(const float *in, uint32_t w, uint32_t h, const uint32_t *hist, const uint32_t *counts) {
    if (!in || !hist || !counts) return RTW_E_INVALID;
    if (size_check(w, h) != RTW_OK) return RTW_E_INVALID;
    const size_t in_bytes = (size_t)w * h * 3 * sizeof(float), hist_bytes = HIST_BINS * sizeof(uint32_t), counts_bytes = 2 * sizeof(uint32_t);
    if (overlap(hist, hist_bytes, in, in_bytes) || overlap(counts, counts_bytes, in, in_bytes) || overlap(hist, hist_bytes, counts, counts_bytes))
        return RTW_E_INVALID;
    return RTW_OK;
}

int display_check(const float *in, uint32_t w, uint32_t h, const RtwDisplay *p, const void *out, DisplayPlan &pl) {
    if (!in || !p || !out) return RTW_E_INVALID;
    if (size_check(w, h) != RTW_OK) return RTW_E_INVALID;
    if (!(p->exposure >= 0.0f) || !std::isfinite(p->exposure)) return RTW_E_INVALID;
    if (!(p->gamma > 0.0f) || !std::isfinite(p->gamma)) return RTW_E_INVALID;
    if (p->tone > RTW_TONE_ACES_FIT || p->transfer > RTW_TRANSFER_SRGB || p->quantise > RTW_QUANTISE_RUST2 || p->out_format > RTW_DISPLAY_F32)
        return RTW_E_INVALID;
    if (p->dither > 1) return RTW_E_INVALID;
    const bool reinhard = p->tone == RTW_TONE_REINHARD || p->tone == RTW_TONE_REINHARD_LUMA;
    if (reinhard && (!(p->white > 0.0f) || !std::isfinite(p->white))) return RTW_E_INVALID;
    pl = DisplayPlan();
    pl.w = w; pl.h = h;
    pl.exposure = p->exposure;
    pl.tone = p->tone;
    pl.ww = reinhard ? p->white * p->white : 1.0f;
    pl.transfer = p->transfer;
    pl.inv_gamma = 1.0f / p->gamma;
    if (!std::isfinite(pl.inv_gamma)) return RTW_E_INVALID;
    pl.scale = p->quantise == RTW_QUANTISE_RUST2 ? 255.99f : 255.0f;
    pl.dither = p->dither;
    pl.format = p->out_format;
    const size_t n = (size_t)w * h;
    if (overlap(out, n * display_pixel_bytes(pl.format), in, n * 3 * sizeof(float))) return RTW_E_INVALID;
    return RTW_OK;
}

} // namespace rtw

using namespace rtw;

static_assert(sizeof(RtwMetering) == 24, "POD layout");
static_assert(sizeof(RtwDisplay) == 32, "POD layout");

extern "C" int rtw_luminance_histogram(const float *in, uint32_t w, uint32_t h, uint32_t *hist, uint32_t *counts, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = histogram_check(in, w, h, hist, counts);
    if (rc != RTW_OK) return rc;
    uint32_t slots[HIST_SLOTS] = { 0 };
    const size_t n = (size_t)w * h;
    for (size_t p = 0; p < n; p++) slots[histogram_slot(in[3 * p], in[3 * p + 1], in[3 * p + 2])]++;
    std::memcpy(hist, slots, HIST_BINS * sizeof(uint32_t));
    counts[0] = slots[HIST_BLACK];
    counts[1] = slots[HIST_NON_FINITE];
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, (uint64_t)n };
    }
    return RTW_OK;
}

extern "C" int rtw_exposure_from_histogram(const uint32_t *hist, const RtwMetering *mt, double prev_level, float prev_exposure,
                                           double *level_out, float *exposure_out) {
    if (!hist || !mt || !level_out || !exposure_out) return RTW_E_INVALID;
    if ((uint64_t)mt->low_permille + mt->high_permille >= 1000) return RTW_E_INVALID;
    if (!(mt->key > 0.0f) || !std::isfinite(mt->key)) return RTW_E_INVALID;
    if (!(mt->rate >= 0.0f && mt->rate <= 1.0f)) return RTW_E_INVALID;
    if (!(mt->min_level >= 0.0f && mt->max_level <= 256.0f && mt->min_level <= mt->max_level)) return RTW_E_INVALID;
    const bool first = prev_level != prev_level;
    if (!first && !(prev_level >= 0.0 && prev_level <= 256.0)) return RTW_E_INVALID;
    uint64_t c[HIST_BINS], total = 0;
    for (int i = 0; i < HIST_BINS; i++) { c[i] = hist[i]; total += c[i]; }
    uint64_t drop_lo = total * mt->low_permille / 1000, drop_hi = total * mt->high_permille / 1000;
    const uint64_t n = total - drop_lo - drop_hi;                          // > 0 when total > 0: low + high < 1000
    if (n == 0) {
        *level_out = prev_level;
        *exposure_out = first ? 1.0f : prev_exposure;
        return RTW_OK;
    }
    for (int i = 0; i < HIST_BINS && drop_lo; i++) { const uint64_t k = c[i] < drop_lo ? c[i] : drop_lo; c[i] -= k; drop_lo -= k; }
    for (int i = HIST_BINS - 1; i >= 0 && drop_hi; i--) { const uint64_t k = c[i] < drop_hi ? c[i] : drop_hi; c[i] -= k; drop_hi -= k; }
    uint64_t S = 0;
    for (int i = 0; i < HIST_BINS; i++) S += c[i] * (uint64_t)(2 * i + 1);
    double m = (double)S / (2.0 * (double)n);
    m = m < (double)mt->min_level ? (double)mt->min_level : (m > (double)mt->max_level ? (double)mt->max_level : m);
    const double level = first ? m : prev_level + (double)mt->rate * (m - prev_level);
    const double x = level / 8.0;
    int64_t s = (int64_t)x;                                                // floor, without libm
    if ((double)s > x) s -= 1;
    const double f = x - (double)s;
    const uint64_t pbits = (uint64_t)(1023 + s - 16) << 52;                // 2^(s - 16); level is within an ulp of [0, 256], so s is in -1 .. 32
    double p2;
    std::memcpy(&p2, &pbits, sizeof p2);
    const double y_meter = (1.0 + f) * p2;
    *level_out = level;
    *exposure_out = (float)((double)mt->key / y_meter);
    return RTW_OK;
}

extern "C" int rtw_display(const float *in, uint32_t w, uint32_t h, const RtwDisplay *params, void *out, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    DisplayPlan pl;
    const int rc = display_check(in, w, h, params, out, pl);
    if (rc != RTW_OK) return rc;
    const size_t n = (size_t)w * h;
    for (size_t p = 0; p < n; p++) display_write(pl, in, out, p);
    if (stats) {
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms, ms, (uint64_t)n };
    }
    return RTW_OK;
}
