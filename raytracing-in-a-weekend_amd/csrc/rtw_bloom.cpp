// rtw_bloom.cpp -- the host form of bloom (rtw_bloom, rtw_bloom_levels; include/rtw.h) and the argument check it shares with the device path
// (rtw_bloom.hip).  Pure host code: no HIP call.  One thread; every pixel of every step runs bloom_down_pixel / bloom_up_value (rtw_bloom.h),
// which the kernels run too.
#include "rtw_bloom.h"

#include <chrono>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

namespace rtw {

namespace {

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

bool plain(float v) { return v >= 0.0f && std::isfinite(v); }             // neither negative nor NaN nor infinite

} // namespace

int bloom_check(const float *in, uint32_t w, uint32_t h, const RtwBloom *p, const float *out, const float *layer_out, BloomPlan &pl) {
    if (!in || !out || !p) return RTW_E_INVALID;
    if (w == 0 || h == 0 || (uint64_t)w * h > 0xFFFFFFFFull) return RTW_E_INVALID;
    if (w > RTW_ATROUS_MAX_SIDE || h > RTW_ATROUS_MAX_SIDE) return RTW_E_INVALID;
    if (p->levels < 1 || p->levels > RTW_BLOOM_MAX_LEVELS) return RTW_E_INVALID;
    if (!plain(p->threshold) || !plain(p->knee) || !plain(p->spread) || !plain(p->intensity)) return RTW_E_INVALID;
    if (p->knee > p->threshold) return RTW_E_INVALID;
    if (p->karis > 1) return RTW_E_INVALID;
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    if (layer_out && (overlap(layer_out, bytes, in, bytes) || overlap(layer_out, bytes, out, bytes))) return RTW_E_INVALID;
    if (out != in && overlap(out, bytes, in, bytes)) return RTW_E_INVALID;
    pl = BloomPlan();
    pl.w = w; pl.h = h;
    pl.n = bloom_chain(w, h, p->levels, pl.lw, pl.lh);
    pl.off[1] = 0;
    for (uint32_t l = 1; l <= pl.n; l++) pl.off[l + 1] = pl.off[l] + (size_t)pl.lw[l] * pl.lh[l] * 3;
    pl.threshold = p->threshold; pl.knee = p->knee;
    pl.karis = p->karis;
    pl.spread = p->spread; pl.intensity = p->intensity;
    return RTW_OK;
}

} // namespace rtw

using namespace rtw;

static_assert(sizeof(RtwBloom) == 24, "POD layout");

extern "C" uint32_t rtw_bloom_levels(uint32_t w, uint32_t h, uint32_t levels, uint32_t *sizes) {
    if (w == 0 || h == 0 || levels < 1 || levels > RTW_BLOOM_MAX_LEVELS) return 0;
    uint32_t lw[RTW_BLOOM_MAX_LEVELS + 1], lh[RTW_BLOOM_MAX_LEVELS + 1];
    const uint32_t n = bloom_chain(w, h, levels, lw, lh);
    if (sizes)
        for (uint32_t l = 1; l <= n; l++) { sizes[2 * (l - 1)] = lw[l]; sizes[2 * (l - 1) + 1] = lh[l]; }
    return n;
}

extern "C" int rtw_bloom(const float *in, uint32_t w, uint32_t h, const RtwBloom *params, float *out, float *layer_out, RtwFilterStats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    BloomPlan pl;
    const int rc = bloom_check(in, w, h, params, out, layer_out, pl);
    if (rc != RTW_OK) return rc;
    std::vector<float> pyr;
    try { pyr.resize(pl.off[pl.n + 1]); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    uint64_t taps = 0;
    // down: the frame through the bright pass to level 1, then level to level
    for (uint32_t l = 0; l < pl.n; l++) {
        float *dst = pyr.data() + pl.off[l + 1];
        const int dw = (int)pl.lw[l + 1], dh = (int)pl.lh[l + 1];
        const BloomFrameSrc fs = { in, (int)w, (int)h, pl.threshold, pl.knee, pl.karis };
        const BloomMemSrc ms = { l ? pyr.data() + pl.off[l] : nullptr, (int)pl.lw[l], (int)pl.lh[l] };
        for (int J = 0; J < dh; J++)
            for (int I = 0; I < dw; I++) {
                float *o = dst + 3 * ((size_t)J * dw + I);
                taps += l == 0 ? bloom_down_pixel(fs, I, J, o) : bloom_down_pixel(ms, I, J, o);
            }
    }
    // up, in place: a pixel of level l reads itself and a window of level l + 1 only
    for (uint32_t l = pl.n - 1; l >= 1; l--) {
        float *dst = pyr.data() + pl.off[l];
        const BloomMemSrc ms = { pyr.data() + pl.off[l + 1], (int)pl.lw[l + 1], (int)pl.lh[l + 1] };
        const int dw = (int)pl.lw[l], dh = (int)pl.lh[l];
        for (int j = 0; j < dh; j++)
            for (int i = 0; i < dw; i++) {
                float u[3], *o = dst + 3 * ((size_t)j * dw + i);
                taps += bloom_up_value(ms, i, j, u);
                for (int c = 0; c < 3; c++) o[c] = o[c] + pl.spread * u[c];
            }
    }
    // composite
    const BloomMemSrc ms = { pyr.data() + pl.off[1], (int)pl.lw[1], (int)pl.lh[1] };
    for (int j = 0; j < (int)h; j++)
        for (int i = 0; i < (int)w; i++) {
            float u[3];
            const size_t p = 3 * ((size_t)j * w + i);
            taps += bloom_up_value(ms, i, j, u);
            for (int c = 0; c < 3; c++) out[p + c] = in[p + c] + pl.intensity * u[c];
            if (layer_out) for (int c = 0; c < 3; c++) layer_out[p + c] = u[c];
        }
    if (stats) {
        const float ms_ = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *stats = RtwFilterStats{ 0.0f, 0.0f, 0.0f, 0.0f, ms_, ms_, taps };
    }
    return RTW_OK;
}
