// rtw_svgf_dev.h -- the device paths of the variance estimate and the variance-steered a-trous filter (rtw_svgf.hip) as rtw_shim.hip's
// context entry points see them.  Both use the a-trous filter's scratch (rtw_atrous_dev.h).
#pragma once
#include "rtw_atrous_dev.h"

namespace rtw {

// rtw_ctx_variance_estimate / rtw_ctx_svgf_filter on `device` / `stream`; *scratch is created on first use.  layout: RTW_OPT_ATROUS_LAYOUT
// (0 = the measured choice).  A failed HIP call stores its code in *last_hip.
int variance_estimate_device(int device, hipStream_t stream, AtrousScratch **scratch, uint32_t layout, const float *moments, const float *len,
                             uint32_t w, uint32_t h, const float *depth, const float *normal, const int32_t *idx, const RtwVarianceEstimate *p,
                             float *out, RtwFilterStats *stats, int *last_hip);
int svgf_filter_device(int device, hipStream_t stream, AtrousScratch **scratch, uint32_t layout, const float *in, const float *variance, uint32_t w,
                       uint32_t h, const float *depth, const float *normal, const int32_t *idx, const float *albedo, const float *emitted,
                       const RtwAtrous *p, const RtwSvgf *vp, float *out, float *out_variance, RtwFilterStats *stats, int *last_hip);

} // namespace rtw
