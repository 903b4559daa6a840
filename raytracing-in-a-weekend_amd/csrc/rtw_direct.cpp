// rtw_direct.cpp -- the host forms of the direct-lighting rule: rtw_light_samples writes the segments direct_light_kernel (rtw_occluded.hip)
// makes in registers and their weights, rtw_light_reduce sums an item's weights in the kernel's association, both from the same
// definitions (rtw_direct.h).  Pure host code: no HIP call.
#include "rtw_direct.h"
#include "rtw.h"
#include <cstddef>

using namespace rtw;

// The row of one light of a list against a scene's top-level spheres and quads, under rtw_lights_validate's checks of that light
// (light_row_of, rtw_shim.hip: a known kind, an index within the scene and below the quad code bit)
static int direct_row_of(const RtwScene *scene, const RtwLight &l, DirectRow &row) {
    if (l.kind == RTW_LIGHT_SPHERE) {
        if (l.index >= scene->n_spheres || !scene->spheres) return RTW_E_INVALID;
        row = direct_row_sphere(scene->spheres[l.index].center, scene->spheres[l.index].radius);
    } else if (l.kind == RTW_LIGHT_QUAD) {
        if (l.index >= scene->n_quads || !scene->quads || l.index >= LIGHT_HIT_QUAD) return RTW_E_INVALID;
        row = direct_row_quad(scene->quads[l.index].origin, scene->quads[l.index].u, scene->quads[l.index].v);
    } else return RTW_E_INVALID;
    return RTW_OK;
}

int rtw_light_samples(const RtwScene *scene, const RtwLight *lights, uint32_t n_lights, const float *points, const float *normals, uint32_t n,
                      uint32_t samples, uint32_t seed, float *rays_out, float *weight_out) {
    if (!scene || !lights || n_lights == 0 || n_lights > RTW_MAX_LIGHTS) return RTW_E_INVALID;
    if (!points || !normals || !rays_out || !weight_out || n == 0 || !ao_samples_ok(samples)) return RTW_E_INVALID;
    DirectRow rows[RTW_MAX_LIGHTS];
    for (uint32_t l = 0; l < n_lights; l++)
        if (const int rc = direct_row_of(scene, lights[l], rows[l])) return rc;
    for (uint32_t i = 0; i < n; i++) {
        const float *pp = points + 3 * (size_t)i, *nn = normals + 3 * (size_t)i;
        const lv3 p = lmk(pp[0], pp[1], pp[2]), nrm = lmk(nn[0], nn[1], nn[2]);
        for (uint32_t l = 0; l < n_lights; l++) {
            const uint32_t base = direct_item_base(seed, i, l);
            const size_t item = (size_t)i * n_lights + l;
            float *r = rays_out + 6 * (size_t)samples * item, *w = weight_out + (size_t)samples * item;
            for (uint32_t k = 0; k < samples; k++, r += 6) {
                lv3 d;
                float G;
                if (!direct_sample(rows[l], base, k, p, nrm, d, G)) { for (int c = 0; c < 6; c++) r[c] = 0.0f; w[k] = 0.0f; continue; }
                r[0] = pp[0]; r[1] = pp[1]; r[2] = pp[2];
                r[3] = d.x; r[4] = d.y; r[5] = d.z;
                w[k] = G;
            }
        }
    }
    return RTW_OK;
}

int rtw_light_reduce(const float *weights, uint32_t samples, float *out) {
    if (!weights || !out || !ao_samples_ok(samples)) return RTW_E_INVALID;
    *out = direct_sum(weights, samples) * (1.0f / (float)samples);
    return RTW_OK;
}
