// rtw_light.h -- Rust2's light-biased integrators (Rust2/src/viewport/ray_color.rs:55-164) and the material_pdf methods they call
// (Rust2/src/objects/material.rs:45-62, 93-99, 199-232).  The pure pieces are __host__ __device__, one definition for the light build of the
// render kernels (SPEC 9) and for the host entry points rtw_light_mid / rtw_material_pdf / rtw_light_term (rtw_shim.hip) that the CPU tests
// call.  f32, one rounding per written operation, no FMA (-ffp-contract=off), the reference's operation order (DESIGN.md "Light-biased
// integrators").  Only the light builds (SPEC 9, 10, 11) compile the device part.
#pragma once
#include "rtw_device.h"

namespace rtw {

// ---- pure pieces ------------------------------------------------------------------------------------------------------------------
struct lv3 { float x, y, z; };
__host__ __device__ __forceinline__ lv3 lmk(float x, float y, float z) { lv3 r; r.x = x; r.y = y; r.z = z; return r; }
__host__ __device__ __forceinline__ lv3 lsub(lv3 a, lv3 b) { return lmk(a.x - b.x, a.y - b.y, a.z - b.z); }
__host__ __device__ __forceinline__ lv3 ladd(lv3 a, lv3 b) { return lmk(a.x + b.x, a.y + b.y, a.z + b.z); }
__host__ __device__ __forceinline__ lv3 lscale(lv3 a, float s) { return lmk(a.x * s, a.y * s, a.z * s); }
__host__ __device__ __forceinline__ lv3 lneg(lv3 a) { return lmk(-a.x, -a.y, -a.z); }
__host__ __device__ __forceinline__ float ldot(lv3 a, lv3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// Vec3::unit (Rust2/src/vec3.rs:219-221): self / self.length()
__host__ __device__ __forceinline__ lv3 lunit(lv3 a) {
    const float l = __builtin_sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
    return lmk(a.x / l, a.y / l, a.z / l);
}
// Vec3's PartialEq (vec3.rs:18-20, 286-288): (a - b).close_to_zero(), every |component| < 1e-7 (false for a NaN)
__host__ __device__ __forceinline__ bool leq(lv3 a, lv3 b) {
    const lv3 d = lsub(a, b);
    return __builtin_fabsf(d.x) < 1e-7f && __builtin_fabsf(d.y) < 1e-7f && __builtin_fabsf(d.z) < 1e-7f;
}
// Vec3::reflect (vec3.rs:283-285): self - n * 2.0 * self.dot(n)
__host__ __device__ __forceinline__ lv3 lreflect(lv3 a, lv3 n) { return lsub(a, lscale(lscale(n, 2.0f), ldot(a, n))); }
// aabb.rs:87-92
__host__ __device__ __forceinline__ float l_minf(float a, float b) { return a <= b ? a : b; }
__host__ __device__ __forceinline__ float l_maxf(float a, float b) { return a >= b ? a : b; }

// The mid-point of a sphere's box (sphere.rs:22-34, Interval::new + mid_point aabb.rs:52-60)
__host__ __device__ __forceinline__ void light_mid_sphere(const float c[3], float r, float mid[3]) {
    for (int k = 0; k < 3; k++) {
        const float a = c[k] - r, b = c[k] + r;
        mid[k] = (l_minf(a, b) + l_maxf(a, b)) * 0.5f;
    }
}
// ... of a quad's (quad.rs:53-110): the four corners, an axis thinner than MIN_AABB_WIDTH = 0.005 widened about its centre
__host__ __device__ __forceinline__ void light_mid_quad(const float o[3], const float u[3], const float v[3], float mid[3]) {
    const float W = 0.005f;
    for (int k = 0; k < 3; k++) {
        const float op = (o[k] + u[k]) + v[k], vc = o[k] + v[k], uc = o[k] + u[k];
        float mn = l_minf(l_minf(op, vc), l_minf(uc, o[k]));
        float mx = l_maxf(l_maxf(op, vc), l_maxf(uc, o[k]));
        if (mx - mn < W) {
            const float c = 0.5f * (mx + mn);
            mx = c + W * 0.5f;
            mn = c - W * 0.5f;
        }
        mid[k] = (mn + mx) * 0.5f;
    }
}

// MirrorGlass::refract / reflectance (material.rs:114-128); powi(5) = x * ((x*x) * (x*x))
__host__ __device__ __forceinline__ lv3 l_refract(lv3 uv, lv3 n, float etai_over_etat) {
    float cos_theta = ldot(lneg(uv), n);
    if (cos_theta > 1.0f) cos_theta = 1.0f;
    const lv3 perp = lscale(ladd(uv, lscale(n, cos_theta)), etai_over_etat);
    const lv3 par = lscale(n, -__builtin_sqrtf(__builtin_fabsf(1.0f - ldot(perp, perp))));
    return ladd(perp, par);
}
__host__ __device__ __forceinline__ float l_reflectance(float cosine, float ref_idx) {
    float r0 = (1.0f - ref_idx) / (1.0f + ref_idx);
    r0 = r0 * r0;
    const float x = 1.0f - cosine, x2 = x * x;
    return r0 + (1.0f - r0) * (x * (x2 * x2));
}

// material_pdf(h, r) of the material RTW_INTEGRATOR_RUST2 selects for {metallicness, opacity, ir}; h = {p, n, incoming ray (din, tm)},
// r = {ro, rd, rtm}.  Lambertian material.rs:45-62, Mirror :93-99 (`*r == self.on_hit(h)`: Ray's derived PartialEq -- origin and direction
// with Vec3's 1e-7 rule, time exactly; on_hit reflects the UN-normalised direction), MirrorGlass :199-232.
__host__ __device__ __forceinline__ float light_material_pdf(float metallicness, float opacity, float ir, lv3 p, lv3 n, lv3 din, float tm,
                                                             lv3 ro, lv3 rd, float rtm) {
    if (opacity > 0.0f) {
        if (!leq(ro, p)) return 0.0f;
        const bool front = !(ldot(din, n) > 0.0f);
        const lv3 nn = front ? n : lneg(n);
        const float ratio = front ? 1.0f / ir : ir;
        const lv3 ud = lunit(din);
        float ct = ldot(lneg(ud), nn);
        if (ct > 1.0f) ct = 1.0f;
        const float st = __builtin_sqrtf(1.0f - ct * ct);
        const bool cannot_refract = ratio * st > 1.0f;
        const lv3 refl = lreflect(ud, nn);
        if (cannot_refract && leq(refl, rd)) return 1.0f;
        const float rfl = l_reflectance(ct, ratio);
        if (leq(refl, rd)) return rfl;
        if (leq(l_refract(ud, nn, ratio), rd)) return 1.0f - rfl;
        return 0.0f;
    }
    if (metallicness == 1.0f)
        return (leq(ro, p) && leq(rd, lreflect(din, n)) && rtm == tm) ? 1.0f : 0.0f;
    if (!leq(ro, p)) return 0.0f;
    const float cosv = ldot(lunit(rd), lunit(n));
    float c = ldot(din, n) >= 0.0f ? -cosv : cosv;
    if (c < 0.0f) c = 0.0f;                                   // f32::clamp(0.0, 1.0): NaN and -0.0 pass through
    if (c > 1.0f) c = 1.0f;
    return c * 0.318309886183790671538f;
}

// One light whose shadow ray found it (ray_color.rs:84-90 / :140-150).  `biased`: light_biased_ray_color, else light_biased_ray_cast.
// Returns false when light_biased_ray_color skips the light.
__host__ __device__ __forceinline__ bool light_add(bool biased, float pdf, lv3 e, float t, lv3 dir, float w, lv3 &S, float &count) {
    if (biased) {
        if (pdf <= 1.0f / (255.0f * l_maxf(l_maxf(e.x, e.y), e.z))) return false;       // (255. * max).recip()
        const float distance2 = t * t * ldot(dir, dir);
        count = count + w;
        S = ladd(S, lmk(e.x * pdf / distance2 * w, e.y * pdf / distance2 * w, e.z * pdf / distance2 * w));
        return true;
    }
    const float distance2 = t * t * ldot(dir, dir);
    count = count + 1.0f;                                      // (an integer in the reference: at most RTW_MAX_LIGHTS, exact in f32)
    S = ladd(S, lmk(e.x * pdf / distance2, e.y * pdf / distance2, e.z * pdf / distance2));
    return true;
}

// ---- the light list in the kernel arguments -----------------------------------------------------------------------------------------
// Wave-uniform and only ever read: one 16-byte row per light, {mid-point, code of the light's object}.
enum : uint32_t {                         // object codes of a closest hit: top-level sphere i = i,
    LIGHT_HIT_QUAD = 0x80000000u,         // top-level quad k = LIGHT_HIT_QUAD | k,
    LIGHT_HIT_INSTANCE = 0xFFFFFFFFu,     // an instance (never a light),
    LIGHT_HIT_NONE = 0xFFFFFFFEu          // nothing
};
// render_bvh's lane flag word (F_HAVE .. F_DONE = bits 0..3 there) in the light build: bit 4 says the query in flight is a shadow query,
// bits 8..15 hold the pending light (the bounce count of the specialised builds lives there; the light build keeps Path.k)
enum : uint32_t { LF_SHADOW = 16u, LF_LIGHT_SHIFT = 8u, LF_LIGHT_MASK = 0xFF00u };
struct DevLights {
    float row[RTW_MAX_LIGHTS][4];         // mid.x, mid.y, mid.z, code (bits)
    uint32_t n;
    float weight;                         // biased_weight
    uint32_t pad[2];
};
static_assert(sizeof(DevLights) == 16 * RTW_MAX_LIGHTS + 16, "DevLights is RTW_MAX_LIGHTS + 1 f4 rows");

#if defined(__HIPCC__)
// ---- device: what a surface hit keeps while its shadow queries run ------------------------------------------------------------------
struct LightPath {
    v3 scat;                              // the scattered direction, drawn AT the hit as the reference does (LIGHT_BIASED)
    v3 n, din;                            // h.n, h.r.direction
    float tm;                             // h.r.time (the path's; the shadow rays run at time 0)
    float metallicness, opacity, ir;
    v3 cm, e;                             // ColorResult{multiplied, emmited} of the surface
    v3 S; float count;
};
__device__ __forceinline__ lv3 tol(v3 a) { return lmk(a.x, a.y, a.z); }

// Row i of the light list, read from the kernel-argument block through the constant address space: a scalar load where i is wave-uniform
// (render_brute's loop), a vector load where it is per lane (render_bvh's pending light).  `off` = offsetof(KArgs, lights).
__device__ __forceinline__ f4 light_row(uint32_t off, uint32_t i) {
    const char __attribute__((address_space(4))) *base = (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    return ((cf4_ptr)(base + off))[i];
}

// The closest-hit walk over quads and instances for a shadow ray: which object wins, no record.  Returns the object code when a quad or an
// instance beats the sphere result (t_out = its t), LIGHT_HIT_NONE otherwise.  As geom_closest without media (the light integrators refuse
// scenes with a constant-density instance).  QUAT: the quaternion build (SPEC 11), the ray enters an instance as in geom_closest<.., true>.
template <bool QUAT = false>
__device__ __forceinline__ uint32_t shadow_geom_pick(const DevGeom &g, v3 o, v3 d, float tm, float mint, float maxt, bool sphere_found, float sphere_t,
                                                     float &t_out, uint32_t &n_sph, uint32_t &n_quad, const f4 *quats = nullptr) {
    bool found = sphere_found;
    float ht = sphere_t;
    uint32_t code = LIGHT_HIT_NONE;
    {
        bool qfound = false; float qt = 0.0f; uint32_t qk = 0;
        for (uint32_t k = 0; k < g.n_quads; ++k) {
            float t;
            if (quad_pick(g.quads, k, o, d, mint, maxt, qfound, qt, t)) { qfound = true; qt = t; qk = k; }
        }
        n_quad += g.n_quads;
        if (qfound && (!found || ht > qt)) { ht = qt; found = true; code = LIGHT_HIT_QUAD | qk; }
    }
    bool ifound = false; float it = 0.0f;
    for (uint32_t i = 0; i < g.n_inst; ++i) {
        const DevInstance in = g.inst[i];
        const v3 tr = ld3(in.tr);
        v3 lo, ld;
        if constexpr (QUAT) { const quat qn = inst_quat(quats, i); lo = quat_rot(qn, o - tr); ld = quat_rot(qn, d); }
        else { lo = rotated(o - tr, in.back, in.back_k); ld = rotated(d, in.back, in.back_k); }
        float ct; int c;
        if (!instance_pick(g, in, lo, ld, tm, mint, maxt, ct, c, n_sph, n_quad)) continue;
        if (!ifound || it > ct) { it = ct; ifound = true; }
    }
    if (ifound && (!found || ht > it)) { ht = it; code = LIGHT_HIT_INSTANCE; }
    t_out = ht;
    return code;
}
#endif

} // namespace rtw
