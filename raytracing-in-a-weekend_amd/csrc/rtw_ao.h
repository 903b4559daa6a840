// rtw_ao.h -- the sampling rule of ambient occlusion (rtw_ao_rays / rtw_ctx_ambient_occlusion / rtw_ctx_ao_map): which
// ray is sample k of point i under a seed.  Everything here is __host__ __device__: one definition for ambient_occlusion_kernel
// (rtw_occluded.hip) and for the host form rtw_ao_rays (rtw_ao.cpp), so the kernel's rays are rtw_ao_rays' rays bit for bit.
//
// The direction is mixed_dir(exp = 1, ...) of rtw_mixed.h, unchanged: gen_exp = 1/2, and pow(1 - xi, 1/2) is the inverse CDF of the
// cosine lobe, so the samples are cosine-weighted about the normal and the mean of "not occluded" is the ambient term with no weights.
#pragma once
#include "rtw_mixed.h"

namespace rtw {

#define RTW_AO_STREAM 0x414F5241u      /* "AORA": keeps the stream of a point apart from the render's stream of the pixel with the same index */
#define RTW_AO_MAX_SAMPLES 1024u

// rtw_device.h's mix32 / rng_pixel_base / rng_start / rng_f32 are __device__ only; these four are their __host__ __device__ TWINS (as
// probe_mix32 of rtw_probe.h is mix32's).  Change them together.
__host__ __device__ __forceinline__ uint32_t ao_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// rng_pixel_base(seed, RTW_AO_STREAM, i): the (seed, point) prefix of the chain
__host__ __device__ __forceinline__ uint32_t ao_point_base(uint32_t seed, uint32_t i) {
    uint32_t h = ao_mix32(seed + 0x9E3779B9U);
    h = ao_mix32(h ^ RTW_AO_STREAM);
    return ao_mix32(h ^ i);
}
// rng_start(base, k), then two rng_f32 draws: xi_phi first, xi_cos second
__host__ __device__ __forceinline__ void ao_draws(uint32_t base, uint32_t k, float &xi_phi, float &xi_cos) {
    uint32_t state = ao_mix32(base ^ k);
    const uint32_t inc = ao_mix32(state ^ 0x85EBCA6BU) | 1U;
    xi_phi = (float)(state >> 8) * (1.0f / 16777216.0f);
    state = state * 747796405U + inc;
    xi_cos = (float)(state >> 8) * (1.0f / 16777216.0f);
}

// A point with this normal casts no rays and answers 1.0 (the normal rtw_ctx_depth_map writes for a miss); a NaN is not zero
__host__ __device__ __forceinline__ bool ao_skipped(lv3 n) { return n.x == 0.0f && n.y == 0.0f && n.z == 0.0f; }

// The direction of sample k of the point with stream prefix `base` and normal n (not skipped)
__host__ __device__ __forceinline__ lv3 ao_dir(uint32_t base, uint32_t k, lv3 n) {
    float xi_phi, xi_cos;
    ao_draws(base, k, xi_phi, xi_cos);
    return mixed_dir(1.0f, xi_phi, xi_cos, n);
}

// samples: a power of two in 1 .. 1024, so that (samples - c) * (1 / samples) is exact
__host__ __device__ __forceinline__ bool ao_samples_ok(uint32_t samples) {
    return samples >= 1u && samples <= RTW_AO_MAX_SAMPLES && (samples & (samples - 1u)) == 0u;
}

} // namespace rtw
