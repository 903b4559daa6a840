// rtw_atrous_dev.h -- the a-trous filter's device path (rtw_atrous.hip) as rtw_shim.hip's context entry point sees it, and what it shares
// with the variance-steered filter's (rtw_svgf.hip): the workgroup shape and the context's scratch.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw_devmem.h"
#include "rtw.h"

namespace rtw {

constexpr uint32_t ABX = 32, ABY = 16;                   // workgroup: 32 x 16 pixels, a wave covers two rows of 32
constexpr size_t ATROUS_TILE_LDS_MAX = 64u * 1024u;      // a tile beyond this is not tried: one workgroup per CU reads mostly halo

// Device buffers of a context's a-trous, variance-steered a-trous and variance-estimate calls: the ping-pong buffers and the staging of
// host arguments (grown on demand, kept until the context is destroyed).
struct AtrousScratch {
    DevMem ping, pong;                             // the levels' two buffers, [h][w][3] f32 each
    DevMem in, depth, normal, idx, albedo, emitted;   // the caller's host buffers, staged
    DevMem out;                                    // the result when the caller's buffer is host memory
    DevMem vping, vpong;                           // rtw_svgf.hip: the levels' two variance planes, [h][w] f32 each
    DevMem variance, moments, len;                 // rtw_svgf.hip: the caller's host buffers, staged
    DevMem out_variance;                           // rtw_svgf.hip: a variance result whose buffer is host memory
    hipEvent_t ev[2] = { nullptr, nullptr };
};
void atrous_scratch_free(AtrousScratch *s);
// *scratch with its events, created on first use.  hipSuccess, or the failed call's code (hipErrorOutOfMemory: no host memory either).
hipError_t atrous_scratch_get(AtrousScratch **scratch);

// rtw_ctx_atrous_filter on `device` / `stream`; *scratch is created on first use.  layout: RTW_OPT_ATROUS_LAYOUT (0 = the measured choice).
// A failed HIP call stores its code in *last_hip.
int atrous_filter_device(int device, hipStream_t stream, AtrousScratch **scratch, uint32_t layout, const float *in, uint32_t w, uint32_t h,
                         const float *depth, const float *normal, const int32_t *idx, const float *albedo, const float *emitted,
                         const RtwAtrous *p, float *out, RtwFilterStats *stats, int *last_hip);

} // namespace rtw
