// rtw_occluded.hip -- any-hit occlusion queries over the whole scene of a context (rtw_ctx_scene_occluded): for each ray,
// "is anything in the way within [mint, maxt]?" -- one byte, 1 exactly when rtw_ctx_scene_hits (rtw_query.hip) reports an index >= 0.
// A kernel of its own: no render kernel and no closest-hit query reads this file.  ambient_occlusion_kernel (rtw_ctx_ambient_occlusion /
// rtw_ctx_ao_map) lives here too: it makes its rays in registers (rtw_ao.h) and walks them with the same function, and so
// does direct_light_kernel (rtw_ctx_direct_light / rtw_ctx_direct_light_map; the rule: rtw_direct.h).
//
// Why the bit is exact: in every group the acceptance of a candidate with nothing found so far depends on that candidate and on
// [mint, maxt] alone, a later group's result never takes a hit away, and the trees only prune.  So "some candidate is accepted" is "the
// closest-hit query found something".  The groups come in scene_hits_kernel's order and each group's candidates in the order its walk meets
// them, so a lane's work here is a PREFIX of its work there: it stops at its first accepted candidate, tests and counts nothing more, and a
// wave-uniform list loop ends when a ballot says no lane of the wave is still open.
//
// q_sphere and q_ray_ordinary are TWINS of the functions of the same names in rtw_query.hip, and q_sphere_tree_any of q_sphere_tree (that file's
// kernels do not change, so they keep their copies).  Change them together.
#include "rtw_kernels.h"
#include "rtw_occl.h"
#include "rtw_ao.h"
#include "rtw_direct.h"

namespace rtw {

namespace {

#define RTW_Q_KU 1.4305115e-6f      /* 24 * 2^-24: the rounding bound of the reference's quadratic (rtw_kernels.hip RTW_KU) */
#define RTW_Q_DONE ((int)0x80000000) /* stack sentinel / empty tree (DevBvh.root of an empty tree is the same value) */

template <class T> __device__ __forceinline__ T q_lds_get(uint32_t addr) { return *(const __attribute__((address_space(3))) T *)(uintptr_t)addr; }
template <class T> __device__ __forceinline__ void q_lds_put(uint32_t addr, T v) { *(__attribute__((address_space(3))) T *)(uintptr_t)addr = v; }

// One exact sphere test (sphere.rs:99-121) as rtw_query.hip's q_sphere with nothing found so far: is the root in range?  LIST: the list walk's
// first candidate (`min_hit == None`), which a NaN root enters; else the tree's (best_t = maxt, best = -1: x < maxt || x == maxt).
template <bool MOVING, bool LIST>
__device__ __forceinline__ bool q_sphere_any(f4 g, f4 vv, v3 o, v3 d, float tm, float a, float ra, bool a_plain, float mint, float maxt) {
    float cx = g.x, cy = g.y, cz = g.z;
    if (MOVING) { cx = cx + vv.x * tm; cy = cy + vv.y * tm; cz = cz + vv.z * tm; }       // sphere.rs:100
    const float ocx = o.x - cx, ocy = o.y - cy, ocz = o.z - cz;
    const float b = ocx * d.x + ocy * d.y + ocz * d.z;
    const float c = (ocx * ocx + ocy * ocy + ocz * ocz) - g.w;
    const float disc = b * b - a * c;
    bool take = false;
    if (!(disc < 0.0f)) {
        const float x = sphere_root(b, disc, a, ra, a_plain, mint);
        const bool in = !(x < mint || x > maxt);
        take = in && (LIST ? true : (x < maxt || x == maxt));
    }
    return take;
}

// The sphere group in list order (wave-uniform index, scalar loads) until no lane of the wave is open
template <bool MOVING>
__device__ __forceinline__ bool q_sphere_list_any(const DevScene &sc, v3 o, v3 d, float tm, float a, float ra, bool a_plain, float mint, float maxt,
                                                  bool open, uint32_t &n_tests) {
    cf4_ptr geom = (cf4_ptr)(uintptr_t)sc.geom;
    cf4_ptr vel = (cf4_ptr)(uintptr_t)sc.vel;
    const f4 zero = { 0, 0, 0, 0 };
    bool hit = false;
    for (uint32_t s = 0; s < sc.n; ++s) {
        if (ballot64(open) == 0ull) break;
        const f4 g = geom[s], vv = MOVING ? vel[s] : zero;
        if (open) {
            n_tests++;
            if (q_sphere_any<MOVING, true>(g, vv, o, d, tm, a, ra, a_plain, mint, maxt)) { hit = true; open = false; }
        }
    }
    return hit;
}

// The sphere group through the tree, q_sphere_tree's order: the spheres kept outside it first, then the per-lane walk with its stack in LDS
// ([level][thread]; level 0 holds the sentinel), the nearer child first.  A lane ends at its first accepted sphere: its node becomes the
// sentinel.  best_t stays maxt until then, so hi_lim is a constant of the ray.  Every lane here is open.
template <bool MOVING>
__device__ __forceinline__ bool q_sphere_tree_any(const DevScene &sc, const DevBvh &bv, v3 o, v3 d, float tm, float a, float ra, bool a_plain,
                                                  float mint, float maxt, uint32_t sp0, uint32_t sp_top, uint32_t &n_tests, uint32_t &n_nodes,
                                                  bool &overflow) {
    bool hit = false;
    {
        cf4_ptr bg = (cf4_ptr)(uintptr_t)bv.big_geom;
        cf4_ptr bvel = (cf4_ptr)(uintptr_t)bv.big_vel;
        for (uint32_t k = 0; k < bv.n_big; ++k) {
            if (ballot64(!hit) == 0ull) break;
            const f4 g = bg[k], vv = MOVING ? bvel[k] : f4{ 0, 0, 0, 0 };
            if (!hit) {
                n_tests++;
                hit = q_sphere_any<MOVING, false>(g, vv, o, d, tm, a, ra, a_plain, mint, maxt);
            }
        }
    }
    // per-ray constants of the thick-ray slab test: conservative bounds only, so the hardware approximations with safety factors
    const float ex = o.x - bv.cx, ey = o.y - bv.cy, ez = o.z - bv.cz;
    const float M = (__builtin_fabsf(ex) + __builtin_fabsf(ey) + __builtin_fabsf(ez)) * 1.0001f + bv.centre_radius;   // >= |o - C| + R_c
    const float q = (M * M + bv.r_max2) * RTW_Q_KU;
    const float sq_q = __builtin_amdgcn_sqrtf(q) * 1.0001f;
    float rho = fminf(q * bv.inv_2rmin, sq_q);
    rho = rho * 1.0001f + 4.8e-7f * (fabsf(o.x) + fabsf(o.y) + fabsf(o.z) + bv.abs_max);
    const float tau = sq_q * 1.0002f * __builtin_amdgcn_rsqf(a) + 1e-30f;
    float ix = __builtin_amdgcn_rcpf(d.x), iy = __builtin_amdgcn_rcpf(d.y), iz = __builtin_amdgcn_rcpf(d.z);
    if (!(fabsf(d.x) >= 1e-20f)) ix = copysignf(1e20f, d.x);
    if (!(fabsf(d.y) >= 1e-20f)) iy = copysignf(1e20f, d.y);
    if (!(fabsf(d.z) >= 1e-20f)) iz = copysignf(1e20f, d.z);
    const float kpx = -(o.x + rho) * ix, kpy = -(o.y + rho) * iy, kpz = -(o.z + rho) * iz;      // t(lo) = fma(lo, 1/d, -(o + rho) / d)
    const float kmx = -(o.x - rho) * ix, kmy = -(o.y - rho) * iy, kmz = -(o.z - rho) * iz;      // t(hi) = fma(hi, 1/d, -(o - rho) / d)
    const float lo_lim = mint - tau, hi_lim = maxt + tau;

    const uint32_t level = RTW_BLOCK * 4u;
    uint32_t sp = sp0;
    q_lds_put<int>(sp, RTW_Q_DONE);
    int node = hit ? RTW_Q_DONE : bv.root;
    for (;;) {
        if (ballot64(node != RTW_Q_DONE) == 0ull) break;
        if (node >= 0) {                                           // an inner node: two slab tests, the nearer child next, the farther pushed
            const f4 *np = (const f4 *)(bv.nodes + node);
            const f4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const int c0 = __float_as_int(n3.x), c1 = __float_as_int(n3.y);
            n_nodes++;
            float t1, t2;
            t1 = __builtin_fmaf(n0.x, ix, kpx); t2 = __builtin_fmaf(n0.w, ix, kmx);
            float e0 = fminf(t1, t2), x0 = fmaxf(t1, t2);
            t1 = __builtin_fmaf(n0.y, iy, kpy); t2 = __builtin_fmaf(n1.x, iy, kmy);
            e0 = fmaxf(e0, fminf(t1, t2)); x0 = fminf(x0, fmaxf(t1, t2));
            t1 = __builtin_fmaf(n0.z, iz, kpz); t2 = __builtin_fmaf(n1.y, iz, kmz);
            e0 = fmaxf(e0, fminf(t1, t2)); x0 = fminf(x0, fmaxf(t1, t2));
            t1 = __builtin_fmaf(n1.z, ix, kpx); t2 = __builtin_fmaf(n2.y, ix, kmx);
            float e1 = fminf(t1, t2), x1 = fmaxf(t1, t2);
            t1 = __builtin_fmaf(n1.w, iy, kpy); t2 = __builtin_fmaf(n2.z, iy, kmy);
            e1 = fmaxf(e1, fminf(t1, t2)); x1 = fminf(x1, fmaxf(t1, t2));
            t1 = __builtin_fmaf(n2.x, iz, kpz); t2 = __builtin_fmaf(n2.w, iz, kmz);
            e1 = fmaxf(e1, fminf(t1, t2)); x1 = fminf(x1, fmaxf(t1, t2));
            const float m0 = fmaxf(e0, lo_lim), m1 = fmaxf(e1, lo_lim);
            const bool h0 = m0 <= fminf(x0, hi_lim), h1 = m1 <= fminf(x1, hi_lim);
            if (h0 && h1) {
                const bool near0 = m0 <= m1;
                if (sp < sp_top) { sp += level; q_lds_put<int>(sp, near0 ? c1 : c0); }
                else overflow = true;                              // (never with build_bvh's depth; reported as RTW_E_INTERNAL)
                node = near0 ? c0 : c1;
            } else if (h0 || h1) {
                node = h0 ? c0 : c1;
            } else {
                node = q_lds_get<int>(sp); sp -= level;
            }
        }
        if (node < 0 && node != RTW_Q_DONE) {                      // a leaf: the exact test; accepted ends the lane, else the next entry off the stack
            const uint32_t s = (uint32_t)~node;
            n_tests++;
            if (q_sphere_any<MOVING, false>(sc.geom[s], MOVING ? sc.vel[s] : f4{ 0, 0, 0, 0 }, o, d, tm, a, ra, a_plain, mint, maxt)) { hit = true; node = RTW_Q_DONE; }
            else { node = q_lds_get<int>(sp); sp -= level; }
        }
    }
    return hit;
}

// rtw_query.hip's q_ray_ordinary: can the sphere tree answer this ray?  Any other ray walks the list.
__device__ __forceinline__ bool q_ray_ordinary(v3 o, v3 d, float a, float span) {
    const float no = __builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z);
    const float nd = __builtin_fabsf(d.x) + __builtin_fabsf(d.y) + __builtin_fabsf(d.z);
    return no + nd < 0x1p60f && a >= 1e-30f && a <= 1e30f && fmaxf(nd, 2.0f) * (span + no + 1.0f) <= 1e18f;      // (nd >= |d|; NaN fails)
}

// The per-ray sequence of the any-hit pass, ONE definition for scene_occluded_kernel and ambient_occlusion_kernel: spheres by tree or list
// under q_ray_ordinary, then quads, then instances with media skipped, then the triangles or their placements.  `open`: nothing has accepted
// the lane's ray yet; a lane that comes in closed (it has no ray) tests and counts nothing.  Returns `open`.  The ballots see the lanes
// that are active at the call, so a lane outside the call and a lane that comes in closed weigh the same: nothing.
template <bool TREE, bool MOVING>
__device__ __forceinline__ bool occluded_walk(const OccludedArgs &A, const unsigned char *q_lds, v3 o, v3 d, bool open, uint32_t &n_sph,
                                              uint32_t &n_nodes, uint32_t &n_quad, bool &overflow) {
    const float tm = A.time, mint = A.mint, maxt = A.maxt;
    const float a = dot(d, d);
    const float ra = rcp_refined(a);
    const bool a_plain = ballot64(open && !in_range(a, 0x1p-20f, 0x1p20f)) == 0ull;  // see sphere_root()
    // ---- spheres ----
    bool listed = true;
    if (TREE) {
        if (open && q_ray_ordinary(o, d, a, A.span)) {
            const uint32_t sp0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)q_lds + threadIdx.x * 4u;
            if (q_sphere_tree_any<MOVING>(A.sc, A.bvh, o, d, tm, a, ra, a_plain, mint, maxt, sp0, sp0 + (A.levels - 1u) * (RTW_BLOCK * 4u),
                                          n_sph, n_nodes, overflow)) open = false;
            listed = false;
        }
    }
    if (listed) { if (q_sphere_list_any<MOVING>(A.sc, o, d, tm, a, ra, a_plain, mint, maxt, open, n_sph)) open = false; }
    // ---- quads in list order ----
    const DevGeom &g = A.geom;
    for (uint32_t k = 0; k < g.n_quads; ++k) {
        if (ballot64(open) == 0ull) break;
        if (open) {
            float t;
            n_quad++;
            if (quad_pick(g.quads, k, o, d, mint, maxt, false, 0.0f, t)) open = false;
        }
    }
    // ---- instances (instance.rs:250-310), media skipped: any member accepted is the instance accepted ----
    for (uint32_t k = 0; k < g.n_inst; ++k) {
        if (ballot64(open) == 0ull) break;
        const DevInstance in = g.inst[k];
        if (in.medium == RTW_MEDIUM_CONST_DENSITY) continue;
        if (open) {
            const v3 tr = ld3(in.tr);
            v3 lo, ld;
            if (A.inst_quats) { const quat qn = inst_quat(A.inst_quats, k); lo = quat_rot(qn, o - tr); ld = quat_rot(qn, d); }   // (a wave-uniform branch)
            else { lo = rotated(o - tr, in.back, in.back_k); ld = rotated(d, in.back, in.back_k); }
            float ct; int code;
            if (instance_pick(g, in, lo, ld, tm, mint, maxt, ct, code, n_sph, n_quad)) open = false;
        }
    }
    // ---- triangles last ----
    if (A.mesh_rows) {                                             // (a wave-uniform branch) the placements stand in for the world-space triangles
        if (mesh_any(A.tris, A.mesh_rows, A.n_mesh, A.mesh_top, A.n_mesh_top, o, d, mint, maxt, open, n_quad, n_nodes)) open = false;
    } else if (A.tris.n) {
        if (tri_any(A.tris, o, d, mint, maxt, open, n_quad, n_nodes)) open = false;
    }
    return open;
}

// The counters of a lane summed over the wave, one atomic per wave and counter (as scene_hits_kernel), on the workgroup's line of `counters`.
// n_points: the points that cast rays (ambient_occlusion_kernel; [4]), 0 elsewhere.
__device__ __forceinline__ void occluded_count(unsigned long long *counters, uint32_t n_sph, uint32_t n_nodes, uint32_t n_quad, bool overflow,
                                               uint32_t n_points) {
    unsigned long long s0 = n_sph, s1 = n_nodes, s2 = n_quad;
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    const bool any_overflow = ballot64(overflow) != 0ull;
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long *line = counters + (blockIdx.x % RTW_QUERY_SLOTS) * RTW_QUERY_STRIDE;
        if (s0) atomicAdd(&line[0], s0);
        if (s1) atomicAdd(&line[1], s1);
        if (s2) atomicAdd(&line[2], s2);
        if (any_overflow) atomicAdd(&line[3], 1ull);
        if (n_points) atomicAdd(&line[4], (unsigned long long)n_points);
    }
}

} // namespace

// TREE: the sphere group goes through the tree (stack in dynamic LDS).  One ray per lane.
template <bool TREE, bool MOVING>
__global__ __launch_bounds__(RTW_BLOCK) void scene_occluded_kernel(const OccludedArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const uint32_t i = blockIdx.x * RTW_BLOCK + threadIdx.x;
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    if (i < A.n) {
        const float2 *r = (const float2 *)(A.rays + 6 * (size_t)i);
        const float2 r0 = r[0], r1 = r[1], r2 = r[2];
        const v3 o = mk(r0.x, r0.y, r1.x), d = mk(r1.y, r2.x, r2.y);
        const bool open = occluded_walk<TREE, MOVING>(A, q_lds, o, d, true, n_sph, n_nodes, n_quad, overflow);
        A.out[i] = open ? (uint8_t)0 : (uint8_t)1;
    }
    occluded_count(A.counters, n_sph, n_nodes, n_quad, overflow, 0u);
}

// Ambient occlusion (rtw_ctx_ambient_occlusion / rtw_ctx_ao_map): L = min(samples, 64) lanes form a group that owns one
// point, a wave holds 64 / L points, and a lane takes sample k = lane_in_group + round * L in samples / L rounds.  Lane 0 of a group loads
// the point and its normal -- CAM: forms them from the depth pass's depth, index and normal of pixel i and the pixel's ray, by the rule of
// rtw_depth_rays -- and the group gets them by a cross-lane read.  Every lane makes its ray in registers (rtw_ao.h) and walks it with
// occluded_walk; a round's occluded count is the popcount of a ballot under the group's lane mask.  No lane leaves before the end: every
// cross-lane read below finds its source lane active.
// ONE: samples <= 64, a single round.  Nothing of the point then lives across the walk (the point, the normal, the stream's prefix and the
// frame the compiler hoists out of the round loop: up to 37 VGPRs), and the build keeps the 7 waves per SIMD of scene_occluded_kernel; the
// build with the loop runs at 4 - 5.
template <bool CAM, bool TREE, bool MOVING, bool ONE>
__global__ __launch_bounds__(RTW_BLOCK) void ambient_occlusion_kernel(const AoArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const uint32_t lg = A.lg_group, L = 1u << lg;                  // (wave-uniform: samples is a kernel argument)
    const uint32_t lane = threadIdx.x & 63u, g_lane = lane & (L - 1u), g_first = lane - g_lane;
    const unsigned long long point = (unsigned long long)blockIdx.x * (RTW_BLOCK >> lg) + (threadIdx.x >> lg);
    const bool in = point < A.q.n;
    const uint32_t i = (uint32_t)point;
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    v3 p = mk(0.0f, 0.0f, 0.0f), nrm = p;
    if (in && g_lane == 0u) {
        if (CAM) {
            if (A.idx[i] >= 0) {                                   // (a miss pixel is skipped: its normal stays 0 0 0)
                const uint32_t px = i % A.width, py = i / A.width;
                const float fx = (float)px / (float)A.width, fy = (float)py / (float)A.height;
                const v3 o = ld3(A.cam.origin);
                const v3 d = unit((ld3(A.cam.pixel00) + ld3(A.cam.delta_u) * fx) + ld3(A.cam.delta_v) * fy);
                const v3 nn = ld3(A.normals + 3 * (size_t)i);
                p = o + d * A.depth[i];
                nrm = dot(d, nn) > 0.0f ? -nn : nn;                // faced towards the viewer
            }
        } else {
            p = ld3(A.points + 3 * (size_t)i);
            nrm = ld3(A.normals + 3 * (size_t)i);
        }
    }
    if (L > 1u) {
        p.x = __shfl(p.x, (int)g_first); p.y = __shfl(p.y, (int)g_first); p.z = __shfl(p.z, (int)g_first);
        nrm.x = __shfl(nrm.x, (int)g_first); nrm.y = __shfl(nrm.y, (int)g_first); nrm.z = __shfl(nrm.z, (int)g_first);
    }
    const lv3 ln = lmk(nrm.x, nrm.y, nrm.z);
    const bool casts = in && !ao_skipped(ln);                      // (a point past n has the normal 0 0 0 as well)
    const uint32_t base = ao_point_base(A.seed, i);
    const unsigned long long g_mask = (L == 64u ? ~0ull : ((1ull << L) - 1ull)) << g_first;
    uint32_t occluded = 0;
    for (uint32_t round = 0; round < (ONE ? 1u : A.samples); round += (ONE ? 1u : L)) {     // (samples / L rounds, wave-uniform; ONE: no loop)
        const lv3 dir = ao_dir(base, round + g_lane, ln);
        const bool open = occluded_walk<TREE, MOVING>(A.q, q_lds, p, mk(dir.x, dir.y, dir.z), casts, n_sph, n_nodes, n_quad, overflow);
        occluded += (uint32_t)__builtin_popcountll(ballot64(!open) & g_mask);
    }
    if (in && g_lane == 0u) A.ao_out[i] = casts ? (float)(A.samples - occluded) * (1.0f / (float)A.samples) : 1.0f;
    const uint32_t n_points = (uint32_t)__builtin_popcountll(ballot64(casts && g_lane == 0u));
    occluded_count(A.q.counters, n_sph, n_nodes, n_quad, overflow, n_points);
}

// Direct lighting (rtw_ctx_direct_light / rtw_ctx_direct_light_map): ambient_occlusion_kernel's lane mapping over ITEMS.  A
// group of L = min(samples, 64) lanes owns item i * n_lights + l -- point i under light l --, so the groups of a wave may belong to different
// points and lights.  Lane 0 of a group loads (CAM: forms) the point and its normal and the group gets them by a cross-lane read; every lane
// reads the light's row, makes its segment and weight in registers (rtw_direct.h) and walks the segment with occluded_walk, coming in closed
// when the sample is not cast.  The visible count is the popcount of a ballot under the group's lane mask; the weights are summed in the
// fixed association of direct_sum: a lane's rounds in ascending order, then lane g adds lane g + off for off = L/2 .. 1 (a lane with
// g >= off adds something that nobody reads).  No lane leaves before the end: every cross-lane read finds its source lane active.
// ONE: samples <= 64, no round loop (as ambient_occlusion_kernel: nothing of the item but its weight lives across the walk).
template <bool CAM, bool TREE, bool MOVING, bool ONE>
__global__ __launch_bounds__(RTW_BLOCK) void direct_light_kernel(const DirectArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const uint32_t lg = A.lg_group, L = 1u << lg;                  // (wave-uniform: samples is a kernel argument)
    const uint32_t lane = threadIdx.x & 63u, g_lane = lane & (L - 1u), g_first = lane - g_lane;
    const unsigned long long item = (unsigned long long)blockIdx.x * (RTW_BLOCK >> lg) + (threadIdx.x >> lg);
    const bool in = item < (unsigned long long)A.q.n * A.n_lights;
    const uint32_t it = (uint32_t)item;
    const uint32_t i = in ? it / A.n_lights : 0u, l = in ? it - i * A.n_lights : 0u;      // (an item past the end reads row 0 and casts nothing)
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    v3 p = mk(0.0f, 0.0f, 0.0f), nrm = p;
    if (in && g_lane == 0u) {
        if (CAM) {
            if (A.idx[i] >= 0) {                                   // (a miss pixel is skipped: its normal stays 0 0 0)
                const uint32_t px = i % A.width, py = i / A.width;
                const float fx = (float)px / (float)A.width, fy = (float)py / (float)A.height;
                const v3 o = ld3(A.cam.origin);
                const v3 d = unit((ld3(A.cam.pixel00) + ld3(A.cam.delta_u) * fx) + ld3(A.cam.delta_v) * fy);
                const v3 nn = ld3(A.normals + 3 * (size_t)i);
                p = o + d * A.depth[i];
                nrm = dot(d, nn) > 0.0f ? -nn : nn;                // faced towards the viewer
            }
        } else {
            p = ld3(A.points + 3 * (size_t)i);
            nrm = ld3(A.normals + 3 * (size_t)i);
        }
    }
    if (L > 1u) {
        p.x = __shfl(p.x, (int)g_first); p.y = __shfl(p.y, (int)g_first); p.z = __shfl(p.z, (int)g_first);
        nrm.x = __shfl(nrm.x, (int)g_first); nrm.y = __shfl(nrm.y, (int)g_first); nrm.z = __shfl(nrm.z, (int)g_first);
    }
    const lv3 lp = lmk(p.x, p.y, p.z), ln = lmk(nrm.x, nrm.y, nrm.z);
    const DirectRow row = A.lights[l];
    const uint32_t base = direct_item_base(A.seed, i, l);
    const unsigned long long g_mask = (L == 64u ? ~0ull : ((1ull << L) - 1ull)) << g_first;
    uint32_t visible = 0, n_cast = 0;
    float sum = 0.0f;
    for (uint32_t round = 0; round < (ONE ? 1u : A.samples); round += (ONE ? 1u : L)) {     // (samples / L rounds, wave-uniform; ONE: no loop)
        lv3 dir;
        float G;
        const bool cast = direct_sample(row, base, round + g_lane, lp, ln, dir, G) && in;
        const bool open = occluded_walk<TREE, MOVING>(A.q, q_lds, p, mk(dir.x, dir.y, dir.z), cast, n_sph, n_nodes, n_quad, overflow);
        visible += (uint32_t)__builtin_popcountll(ballot64(open) & g_mask);              // (open at the end: cast and free)
        n_cast += (uint32_t)__builtin_popcountll(ballot64(cast));                        // (the wave's; wave-uniform)
        sum = sum + (open ? G : 0.0f);
    }
    for (uint32_t off = L >> 1; off > 0u; off >>= 1) sum = sum + __shfl_down(sum, off);
    if (in && g_lane == 0u) {
        const float inv = 1.0f / (float)A.samples;
        A.vis_out[it] = (float)visible * inv;
        if (A.irr_out) A.irr_out[it] = sum * inv;
    }
    occluded_count(A.q.counters, n_sph, n_nodes, n_quad, overflow, n_cast);
}

void launch_scene_occluded(const OccludedArgs &q, bool tree, hipStream_t stream) {
    typedef void (*occl_fn)(const OccludedArgs);
    const bool moving = q.sc.moving != 0u;
    const occl_fn fn = tree ? (moving ? scene_occluded_kernel<true, true> : scene_occluded_kernel<true, false>)
                            : (moving ? scene_occluded_kernel<false, true> : scene_occluded_kernel<false, false>);
    const uint32_t lds = tree ? q.levels * RTW_BLOCK * 4u : 0u;
    hipLaunchKernelGGL(fn, dim3((q.n + RTW_BLOCK - 1) / RTW_BLOCK), dim3(RTW_BLOCK), lds, stream, q);
}

typedef void (*ao_fn)(const AoArgs);
template <bool CAM, bool TREE, bool MOVING>
static ao_fn pick_ao(bool one) { return one ? ambient_occlusion_kernel<CAM, TREE, MOVING, true> : ambient_occlusion_kernel<CAM, TREE, MOVING, false>; }

void launch_ambient_occlusion(const AoArgs &q, bool from_camera, bool tree, hipStream_t stream) {
    const bool moving = q.q.sc.moving != 0u;
    const bool one = q.samples <= 64u;
    const ao_fn fns[2][2][2] = {
        { { pick_ao<false, false, false>(one), pick_ao<false, false, true>(one) }, { pick_ao<false, true, false>(one), pick_ao<false, true, true>(one) } },
        { { pick_ao<true, false, false>(one), pick_ao<true, false, true>(one) }, { pick_ao<true, true, false>(one), pick_ao<true, true, true>(one) } } };
    const uint32_t lds = tree ? q.q.levels * RTW_BLOCK * 4u : 0u;
    const uint32_t per_block = RTW_BLOCK >> q.lg_group;            // points of a workgroup
    hipLaunchKernelGGL(fns[from_camera][tree][moving], dim3((uint32_t)(((unsigned long long)q.q.n + per_block - 1u) / per_block)), dim3(RTW_BLOCK), lds, stream, q);
}

typedef void (*direct_fn)(const DirectArgs);
template <bool CAM, bool TREE, bool MOVING>
static direct_fn pick_direct(bool one) { return one ? direct_light_kernel<CAM, TREE, MOVING, true> : direct_light_kernel<CAM, TREE, MOVING, false>; }

void launch_direct_light(const DirectArgs &q, bool from_camera, bool tree, hipStream_t stream) {
    const bool moving = q.q.sc.moving != 0u;
    const bool one = q.samples <= 64u;
    const direct_fn fns[2][2][2] = {
        { { pick_direct<false, false, false>(one), pick_direct<false, false, true>(one) }, { pick_direct<false, true, false>(one), pick_direct<false, true, true>(one) } },
        { { pick_direct<true, false, false>(one), pick_direct<true, false, true>(one) }, { pick_direct<true, true, false>(one), pick_direct<true, true, true>(one) } } };
    const uint32_t lds = tree ? q.q.levels * RTW_BLOCK * 4u : 0u;
    const uint32_t per_block = RTW_BLOCK >> q.lg_group;            // items of a workgroup
    const unsigned long long items = (unsigned long long)q.q.n * q.n_lights;
    hipLaunchKernelGGL(fns[from_camera][tree][moving], dim3((uint32_t)((items + per_block - 1u) / per_block)), dim3(RTW_BLOCK), lds, stream, q);
}

} // namespace rtw
