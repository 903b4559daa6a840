// rtw_upsample_dev.h -- the device path of the guide-steered upsampling (rtw_upsample.hip) as rtw_shim.hip's context entry point sees it.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// Device buffers of a context's rtw_ctx_upsample_filter calls: the staging of host arguments and results (grown on demand, kept until the
// context is destroyed).
struct UpsampleScratch;
void upsample_scratch_free(UpsampleScratch *s);

// rtw_ctx_upsample_filter on `device` / `stream`; *scratch is created on first use.  layout: RTW_OPT_ATROUS_LAYOUT (0 = the measured choice).
// A failed HIP call stores its code in *last_hip.
int upsample_filter_device(int device, hipStream_t stream, UpsampleScratch **scratch, uint32_t layout, const float *lo, uint32_t w_lo,
                           uint32_t h_lo, const RtwGuides *g_lo, uint32_t w, uint32_t h, const RtwGuides *g_hi, const RtwUpsample *p, float *out,
                           float *wsum_out, RtwFilterStats *stats, int *last_hip);

} // namespace rtw
