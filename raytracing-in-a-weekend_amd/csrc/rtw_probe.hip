// rtw_probe.hip -- the device-math probe (rtw.h "device math, for tests"): the arithmetic sequences of rtw_device.h, rtw_mixed.h and rtw_exp.h
// evaluated on the GPU one element per thread, and in-kernel sweeps that judge sqrt_plain and div_plain against the exact integer predicates
// of rtw_probe.h.  The functions are CALLED, never restated: what runs here is the text the render, query and filter kernels compile, built
// with the same flags.  No render kernel includes or calls anything of this file.
#include "rtw_device.h"
#include "rtw_mixed.h"
#include "rtw_exp.h"
#include "rtw_probe.h"
#include "rtw_devmem.h"

#include <cstring>

namespace rtw {

#define PROBE_BLOCK 256u
#define PROBE_SWEEP_ITEMS 8u          // arguments per thread of a sweep: consecutive indices stay in consecutive lanes

// ---- element-wise -------------------------------------------------------------------------------------------------------------------------
template <uint32_t FN>
__global__ __launch_bounds__(PROBE_BLOCK) void device_math_kernel(const float *in, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;                              // (the last wave's ballots then cover its live lanes only, as a render's exec mask would)
    if (FN == RTW_MATH_SQRT_PLAIN) out[i] = sqrt_plain(in[i]);
    if (FN == RTW_MATH_SQRT_IEEE) out[i] = sqrt_ieee(in[i]);
    if (FN == RTW_MATH_DIV) {
        const float nn = in[2 * (size_t)i], d = in[2 * (size_t)i + 1];
        out[i] = div_plain(nn, d, rcp_refined(d));
    }
    if (FN == RTW_MATH_UNIT) {
        const v3 r = unit(ld3(in + 3 * (size_t)i));
        out[3 * (size_t)i] = r.x; out[3 * (size_t)i + 1] = r.y; out[3 * (size_t)i + 2] = r.z;
    }
    if (FN == RTW_MATH_UNIT_BALL) {
        const v3 r = unit_of_ball_point(ld3(in + 4 * (size_t)i), in[4 * (size_t)i + 3]);
        out[3 * (size_t)i] = r.x; out[3 * (size_t)i + 1] = r.y; out[3 * (size_t)i + 2] = r.z;
    }
    if (FN == RTW_MATH_SPHERE_ROOT) {
        const float b = in[4 * (size_t)i], disc = in[4 * (size_t)i + 1], a = in[4 * (size_t)i + 2], mint = in[4 * (size_t)i + 3];
        const float ra = rcp_refined(a);
        const bool a_plain = ballot64(!in_range(a, 0x1p-20f, 0x1p20f)) == 0ull;      // as closest_brute (rtw_kernels.hip) and rtw_query.hip form it
        float x = __builtin_nanf("");
        if (!(disc < 0.0f)) x = sphere_root(b, disc, a, ra, a_plain, mint);
        out[i] = x;
    }
    if (FN == RTW_MATH_ATAN2) out[i] = atan2_plain(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
    if (FN == RTW_MATH_ACOS) out[i] = acos_plain(in[i]);
    if (FN == RTW_MATH_SPHERE_UV) {
        float u, v;
        sphere_uv(ld3(in + 3 * (size_t)i), u, v);
        out[2 * (size_t)i] = u; out[2 * (size_t)i + 1] = v;
    }
    if (FN == RTW_MATH_LN) out[i] = ln_f32(in[i]);
    if (FN == RTW_MATH_POW) out[i] = pow_plain(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
    if (FN == RTW_MATH_SINCOS) {
        float s, c;
        sincos_plain(in[i], s, c);
        out[2 * (size_t)i] = s; out[2 * (size_t)i + 1] = c;
    }
    if (FN == RTW_MATH_EXP) out[i] = exp_plain(in[i]);
}

void device_math_cols(uint32_t fn, uint32_t &in_cols, uint32_t &out_cols) {
    static const unsigned char cols[RTW_MATH_COUNT][2] = { { 1, 1 }, { 1, 1 }, { 2, 1 }, { 3, 3 }, { 4, 3 }, { 4, 1 }, { 2, 1 }, { 1, 1 }, { 3, 2 },
                                                           { 1, 1 }, { 2, 1 }, { 1, 2 }, { 1, 1 } };
    in_cols = fn < RTW_MATH_COUNT ? cols[fn][0] : 0u;
    out_cols = fn < RTW_MATH_COUNT ? cols[fn][1] : 0u;
}

template <uint32_t FN>
static void launch_math(const float *in, uint32_t n, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(device_math_kernel<FN>, dim3((n + PROBE_BLOCK - 1u) / PROBE_BLOCK), dim3(PROBE_BLOCK), 0, stream, in, n, out);
}

// as call_status (rtw_shim.hip): after a failure the stream is waited for before the temporaries go
static int probe_status(hipStream_t stream, hipError_t e, int *last_hip) {
    if (e == hipSuccess) return RTW_OK;
    (void)hipStreamSynchronize(stream);
    (void)hipGetLastError();
    if (last_hip) *last_hip = (int)e;
    return e == hipErrorOutOfMemory ? RTW_E_NOMEM : RTW_E_HIP;
}

int device_math_device(int device, hipStream_t stream, uint32_t fn, const float *in, uint32_t n_cols, uint32_t n, float *out, uint32_t out_cols,
                       int *last_hip) {
    uint32_t ic, oc;
    device_math_cols(fn, ic, oc);
    if (!in || !out || n == 0 || ic == 0 || n_cols != ic || out_cols != oc) return RTW_E_INVALID;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { if (last_hip) *last_hip = (int)e; return RTW_E_HIP; }
    const size_t in_bytes = sizeof(float) * (size_t)ic * n, out_bytes = sizeof(float) * (size_t)oc * n;
    DevMem d_i, d_o;
    e = d_i.reserve(in_bytes);
    if (e == hipSuccess) e = d_o.reserve(out_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_i.ptr, in, in_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const float *di = d_i.as<const float>();
        float *dout = d_o.as<float>();
        switch (fn) {
        case RTW_MATH_SQRT_PLAIN:  launch_math<RTW_MATH_SQRT_PLAIN>(di, n, dout, stream); break;
        case RTW_MATH_SQRT_IEEE:   launch_math<RTW_MATH_SQRT_IEEE>(di, n, dout, stream); break;
        case RTW_MATH_DIV:         launch_math<RTW_MATH_DIV>(di, n, dout, stream); break;
        case RTW_MATH_UNIT:        launch_math<RTW_MATH_UNIT>(di, n, dout, stream); break;
        case RTW_MATH_UNIT_BALL:   launch_math<RTW_MATH_UNIT_BALL>(di, n, dout, stream); break;
        case RTW_MATH_SPHERE_ROOT: launch_math<RTW_MATH_SPHERE_ROOT>(di, n, dout, stream); break;
        case RTW_MATH_ATAN2:       launch_math<RTW_MATH_ATAN2>(di, n, dout, stream); break;
        case RTW_MATH_ACOS:        launch_math<RTW_MATH_ACOS>(di, n, dout, stream); break;
        case RTW_MATH_SPHERE_UV:   launch_math<RTW_MATH_SPHERE_UV>(di, n, dout, stream); break;
        case RTW_MATH_LN:          launch_math<RTW_MATH_LN>(di, n, dout, stream); break;
        case RTW_MATH_POW:         launch_math<RTW_MATH_POW>(di, n, dout, stream); break;
        case RTW_MATH_SINCOS:      launch_math<RTW_MATH_SINCOS>(di, n, dout, stream); break;
        default:                   launch_math<RTW_MATH_EXP>(di, n, dout, stream); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_o.ptr, out_bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return probe_status(stream, e, last_hip);
}

// ---- sweeps ---------------------------------------------------------------------------------------------------------------------------------
struct SweepOut {
    unsigned long long wrong;
    uint32_t records[RTW_SWEEP_RECORDS][4];
};

template <uint32_t WHICH>
__global__ __launch_bounds__(PROBE_BLOCK) void device_sweep_kernel(uint64_t first, uint64_t count, uint32_t seed, SweepOut *res) {
    for (uint32_t k = 0; k < PROBE_SWEEP_ITEMS; k++) {
        const uint64_t rel = ((uint64_t)blockIdx.x * PROBE_SWEEP_ITEMS + k) * PROBE_BLOCK + threadIdx.x;
        if (rel >= count) continue;
        const uint64_t index = first + rel;
        uint32_t a, b = 0u, got;
        bool ok;
        if (WHICH == RTW_SWEEP_SQRT) {
            a = (uint32_t)index;
            got = __float_as_uint(sqrt_plain(__uint_as_float(a)));
            ok = sqrt_is_rounded(a, got);
        } else {
            if (WHICH == RTW_SWEEP_DIV_RANDOM) probe_div_random(seed, index, a, b);
            else probe_div_midpoint(seed, index, a, b);
            const float d = __uint_as_float(b), r = rcp_refined(d);
            got = __float_as_uint(div_plain_nz(__uint_as_float(a), d, r));               // what unit, sphere_root and atan2_plain call ...
            ok = div_is_rounded(a, b, got) && got == __float_as_uint(div_plain(__uint_as_float(a), d, r));      // ... and the form that also signs a zero
        }
        if (!ok) {
            const unsigned long long slot = atomicAdd(&res->wrong, 1ull);
            if (slot < RTW_SWEEP_RECORDS) { res->records[slot][0] = a; res->records[slot][1] = b; res->records[slot][2] = got; }
        }
    }
}

int device_sweep_device(int device, hipStream_t stream, uint32_t which, uint64_t first, uint64_t count, uint32_t seed, RtwSweepResult *result,
                        int *last_hip) {
    if (!result || which >= RTW_SWEEP_COUNT || count == 0 || count > (1ull << 32)) return RTW_E_INVALID;
    if (which == RTW_SWEEP_SQRT && (first > (1ull << 32) || first + count > (1ull << 32))) return RTW_E_INVALID;
    if (first + count < first) return RTW_E_INVALID;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { if (last_hip) *last_hip = (int)e; return RTW_E_HIP; }
    DevMem d_r;
    SweepOut back;
    std::memset(&back, 0, sizeof back);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    e = d_r.reserve(sizeof(SweepOut));
    if (e == hipSuccess) e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipMemsetAsync(d_r.ptr, 0, sizeof(SweepOut), stream);
    if (e == hipSuccess) e = hipEventRecord(ev0, stream);
    if (e == hipSuccess) {
        const uint64_t per_block = (uint64_t)PROBE_BLOCK * PROBE_SWEEP_ITEMS;
        const dim3 grid((uint32_t)((count + per_block - 1u) / per_block)), block(PROBE_BLOCK);
        SweepOut *res = d_r.as<SweepOut>();
        if (which == RTW_SWEEP_SQRT) hipLaunchKernelGGL(device_sweep_kernel<RTW_SWEEP_SQRT>, grid, block, 0, stream, first, count, seed, res);
        else if (which == RTW_SWEEP_DIV_RANDOM) hipLaunchKernelGGL(device_sweep_kernel<RTW_SWEEP_DIV_RANDOM>, grid, block, 0, stream, first, count, seed, res);
        else hipLaunchKernelGGL(device_sweep_kernel<RTW_SWEEP_DIV_MIDPOINT>, grid, block, 0, stream, first, count, seed, res);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev1, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&back, d_r.ptr, sizeof(SweepOut), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    const int rc = probe_status(stream, e, last_hip);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (rc != RTW_OK) return rc;
    std::memset(result, 0, sizeof *result);
    result->tested = count;
    result->wrong = back.wrong;
    result->n_records = back.wrong < RTW_SWEEP_RECORDS ? (uint32_t)back.wrong : RTW_SWEEP_RECORDS;
    for (uint32_t i = 0; i < result->n_records; i++) {
        result->records[i].a = back.records[i][0]; result->records[i].b = back.records[i][1]; result->records[i].got = back.records[i][2];
    }
    result->kernel_ms = ms;
    return RTW_OK;
}

} // namespace rtw

using namespace rtw;

extern "C" {

int rtw_rounding_check(uint32_t which, const uint32_t *a, const uint32_t *b, const uint32_t *got, size_t n, uint8_t *ok) {
    if (which >= RTW_SWEEP_COUNT || !a || !got || !ok || n == 0 || (which != RTW_SWEEP_SQRT && !b)) return RTW_E_INVALID;
    for (size_t i = 0; i < n; i++) ok[i] = (which == RTW_SWEEP_SQRT ? sqrt_is_rounded(a[i], got[i]) : div_is_rounded(a[i], b[i], got[i])) ? 1 : 0;
    return RTW_OK;
}

int rtw_sweep_operands(uint32_t which, uint64_t first, size_t n, uint32_t seed, uint32_t *out) {
    if ((which != RTW_SWEEP_DIV_RANDOM && which != RTW_SWEEP_DIV_MIDPOINT) || !out || n == 0) return RTW_E_INVALID;
    for (size_t i = 0; i < n; i++) {
        if (which == RTW_SWEEP_DIV_RANDOM) probe_div_random(seed, first + i, out[2 * i], out[2 * i + 1]);
        else probe_div_midpoint(seed, first + i, out[2 * i], out[2 * i + 1]);
    }
    return RTW_OK;
}

} // extern "C"
