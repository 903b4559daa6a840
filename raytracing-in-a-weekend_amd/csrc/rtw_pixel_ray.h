// rtw_pixel_ray.h -- the direction of RTW_RAYS_PIXEL's ray through pixel (i, j) (include/rtw.h), as ONE definition for rtw_pixel_rays
// (rtw_host.cpp), the surface kernel (rtw_query.hip) and the temporal pass (rtw_temporal.h): f32, one rounding per written operation.
// Plain C++ when no HIP compiler reads it (rtw_host.cpp is also built without one).
#pragma once
#include "rtw.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RTW_PIXEL_RAY_HD __host__ __device__
#else
#define RTW_PIXEL_RAY_HD
#endif

namespace rtw {

// d = (pixel00 + delta_u * ((float)i + ox)) + delta_v * ((float)j + oy), not normalised
RTW_PIXEL_RAY_HD inline void pixel_ray_dir(const RtwCamera &cam, uint32_t i, uint32_t j, float ox, float oy, float &dx, float &dy, float &dz) {
    const float a = (float)i + ox, b = (float)j + oy;
    dx = (cam.pixel00[0] + cam.delta_u[0] * a) + cam.delta_v[0] * b;
    dy = (cam.pixel00[1] + cam.delta_u[1] * a) + cam.delta_v[1] * b;
    dz = (cam.pixel00[2] + cam.delta_u[2] * a) + cam.delta_v[2] * b;
}

} // namespace rtw
