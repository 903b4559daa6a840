// rtw_display_dev.h -- the device path of the display stage (rtw_display.hip) as rtw_shim.hip's context entry points see it.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// Device buffers of a context's rtw_ctx_luminance_histogram and rtw_ctx_display calls: the staging of host arguments and results (grown on
// demand) and the histogram's 258 counters; kept until the context is destroyed.
struct DisplayScratch;
void display_scratch_free(DisplayScratch *s);

// rtw_ctx_luminance_histogram on `device` / `stream`; *scratch is created on first use.  count: RTW_OPT_HISTOGRAM_COUNT (0 = the measured
// choice).  A failed HIP call stores its code in *last_hip.
int luminance_histogram_device(int device, hipStream_t stream, DisplayScratch **scratch, uint32_t count, const float *in, uint32_t w, uint32_t h,
                               uint32_t *hist, uint32_t *counts, RtwFilterStats *stats, int *last_hip);

// rtw_ctx_display likewise.
int display_device(int device, hipStream_t stream, DisplayScratch **scratch, const float *in, uint32_t w, uint32_t h, const RtwDisplay *p,
                   void *out, RtwFilterStats *stats, int *last_hip);

} // namespace rtw
