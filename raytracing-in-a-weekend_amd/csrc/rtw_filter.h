// rtw_filter.h -- the bilateral and the guided post-process (rtw_filter.hip) as rtw_shim.hip's context entry point sees it.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// Device buffers of a context's filter calls (grown on demand, kept until the context is destroyed).
struct FilterScratch;
void filter_scratch_free(FilterScratch *f);

// rtw_ctx_bilateral_filter on `device` / `stream`; *scratch is created on first use.  A failed HIP call stores its code in *last_hip.
int bilateral_filter_device(int device, hipStream_t stream, FilterScratch **scratch, const void *in, uint32_t w, uint32_t h,
                            const RtwBilateral *p, uint8_t *out, RtwFilterStats *stats, int *last_hip);

// rtw_ctx_guided_filter likewise, on the same scratch.  layout: RTW_OPT_GUIDED_LAYOUT (0 = chosen by size).
int guided_filter_device(int device, hipStream_t stream, FilterScratch **scratch, uint32_t layout, const void *in, uint32_t w, uint32_t h,
                         const float *depth, const float *normal, const int32_t *idx, const RtwGuidedFilter *p, uint8_t *out,
                         RtwFilterStats *stats, int *last_hip);

} // namespace rtw
