// rtw_ao.cpp -- the host form of the ambient-occlusion sampling rule: rtw_ao_rays writes the rays ambient_occlusion_kernel
// (rtw_occluded.hip) makes in registers, from the same definitions (rtw_ao.h).  Pure host code: no HIP call.
#include "rtw_ao.h"
#include "rtw.h"
#include <cstddef>

using namespace rtw;

int rtw_ao_rays(const float *points, const float *normals, uint32_t n, uint32_t samples, uint32_t seed, float *rays_out) {
    if (!points || !normals || !rays_out || n == 0 || !ao_samples_ok(samples)) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const float *p = points + 3 * (size_t)i, *nn = normals + 3 * (size_t)i;
        const lv3 nrm = lmk(nn[0], nn[1], nn[2]);
        const bool skip = ao_skipped(nrm);
        const uint32_t base = ao_point_base(seed, i);
        float *r = rays_out + 6 * (size_t)samples * i;
        for (uint32_t k = 0; k < samples; k++, r += 6) {
            if (skip) { for (int c = 0; c < 6; c++) r[c] = 0.0f; continue; }
            const lv3 d = ao_dir(base, k, nrm);
            r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
            r[3] = d.x; r[4] = d.y; r[5] = d.z;
        }
    }
    return RTW_OK;
}
