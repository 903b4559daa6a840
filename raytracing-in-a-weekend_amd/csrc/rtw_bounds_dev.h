// rtw_bounds_dev.h -- the device path of the neighbourhood colour bounds (rtw_bounds.hip) as rtw_shim.hip's context entry point sees it.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// Device buffers of a context's rtw_ctx_colour_bounds calls: the staging of host arguments and results (grown on demand, kept until the
// context is destroyed).
struct BoundsScratch;
void bounds_scratch_free(BoundsScratch *s);

// rtw_ctx_colour_bounds on `device` / `stream`; *scratch is created on first use.  layout: RTW_OPT_ATROUS_LAYOUT (0 = the measured choice).
// A failed HIP call stores its code in *last_hip.
int colour_bounds_device(int device, hipStream_t stream, BoundsScratch **scratch, uint32_t layout, const float *in, uint32_t w, uint32_t h,
                         const int32_t *idx, const RtwColourBounds *p, float *out_lo, float *out_hi, float *out_clamped, RtwFilterStats *stats,
                         int *last_hip);

} // namespace rtw
