// rtw_filter.h -- the bilateral post-process (rtw_filter.hip) as rtw_shim.hip's context entry point sees it.
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

} // namespace rtw
