// rtw_bloom_dev.h -- the device path of bloom (rtw_bloom.hip) as rtw_shim.hip's context entry point sees it.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// Device buffers of a context's rtw_ctx_bloom calls: the staging of host arguments and results and the pyramid (all grown on demand); kept
// until the context is destroyed.
struct BloomScratch;
void bloom_scratch_free(BloomScratch *s);

// rtw_ctx_bloom on `device` / `stream`; *scratch is created on first use.  layout: RTW_OPT_ATROUS_LAYOUT (0 = the measured choice per kernel
// and level size).  A failed HIP call stores its code in *last_hip.
int bloom_device(int device, hipStream_t stream, BloomScratch **scratch, uint32_t layout, const float *in, uint32_t w, uint32_t h,
                 const RtwBloom *p, float *out, float *layer_out, RtwFilterStats *stats, int *last_hip);

} // namespace rtw
