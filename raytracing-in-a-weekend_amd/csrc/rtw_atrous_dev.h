// rtw_atrous_dev.h -- the a-trous filter's device path (rtw_atrous.hip) as rtw_shim.hip's context entry point sees it.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// Device buffers of a context's a-trous calls: the two ping-pong buffers and the staging of host arguments (grown on demand, kept until
// the context is destroyed).
struct AtrousScratch;
void atrous_scratch_free(AtrousScratch *s);

// rtw_ctx_atrous_filter on `device` / `stream`; *scratch is created on first use.  layout: RTW_OPT_ATROUS_LAYOUT (0 = the measured choice).
// A failed HIP call stores its code in *last_hip.
int atrous_filter_device(int device, hipStream_t stream, AtrousScratch **scratch, uint32_t layout, const float *in, uint32_t w, uint32_t h,
                         const float *depth, const float *normal, const int32_t *idx, const float *albedo, const float *emitted,
                         const RtwAtrous *p, float *out, RtwFilterStats *stats, int *last_hip);

} // namespace rtw
