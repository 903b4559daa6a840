// rtw_temporal_dev.h -- the temporal accumulation's device path (rtw_temporal.hip) as rtw_shim.hip's context entry point sees it.
#pragma once
#include <hip/hip_runtime.h>
#include "rtw.h"

namespace rtw {

// Device buffers of a context's temporal calls: the staging of host arguments and results (grown on demand, kept until the context is
// destroyed).
struct TemporalScratch;
void temporal_scratch_free(TemporalScratch *s);

// The buffers of rtw_ctx_temporal_accumulate, in the order of its arguments.
struct TemporalBuffers {
    const float *cur, *depth, *normal;
    const int32_t *idx;
    const float *prev_color, *prev_moments, *prev_len, *prev_depth, *prev_normal;
    const int32_t *prev_idx;
    float *out_color, *out_moments, *out_len, *out_variance;
};

// rtw_ctx_temporal_accumulate on `device` / `stream`; *scratch is created on first use.  A failed HIP call stores its code in *last_hip.
// m: rtw_ctx_temporal_accumulate_motion's table and prev_xy (rtw_temporal.h; host or device memory) -- null, or both of its pointers null:
// the launch of rtw_ctx_temporal_accumulate.
// pt: rtw_ctx_temporal_accumulate_points' prev_point and carried_normal (host or device memory) -- null, or prev_point null: the launch
// `m` alone selects.
// bd: rtw_ctx_temporal_accumulate_bounded's hist_lo, hist_hi and out_clipped (host or device memory) -- null, or all three null: the launch
// `m` and `pt` select.
struct TemporalMotion;
struct TemporalPoints;
struct TemporalBounds;
int temporal_accumulate_device(int device, hipStream_t stream, TemporalScratch **scratch, uint32_t w, uint32_t h, const RtwCamera *cam,
                               const RtwCamera *prev_cam, const TemporalBuffers &b, const RtwTemporal *p, const TemporalMotion *m,
                               const TemporalPoints *pt, const TemporalBounds *bd, RtwFilterStats *stats, int *last_hip);

} // namespace rtw
