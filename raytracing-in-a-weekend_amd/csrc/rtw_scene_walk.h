// rtw_scene_walk.h -- what the scene query kernels share on the device, ONE definition each: the closest-hit pass (rtw_query.hip) and the
// any-hit passes (rtw_occluded.hip) include it, and nothing else does.  Device code only.  The pieces know nothing of the pass that calls
// them: a caller differs from the other in what it passes in.
//
// The sphere tree only prunes (DESIGN.md "Conservative traversal"; the per-ray paddings of q_tree_walk are those of render_bvh's trav_begin,
// global-node variant), and every surviving candidate runs the exact test of q_sphere_root, so a pass through the tree answers bit for bit
// what the same pass answers from the list.
#pragma once
#include "rtw_kernels.h"

namespace rtw {

namespace {

#define RTW_Q_KU 1.4305115e-6f      /* 24 * 2^-24: the rounding bound of the reference's quadratic (rtw_kernels.hip RTW_KU) */
#define RTW_Q_DONE ((int)0x80000000) /* stack sentinel / empty tree (DevBvh.root of an empty tree is the same value) */

template <class T> __device__ __forceinline__ T q_lds_get(uint32_t addr) { return *(const __attribute__((address_space(3))) T *)(uintptr_t)addr; }
template <class T> __device__ __forceinline__ void q_lds_put(uint32_t addr, T v) { *(__attribute__((address_space(3))) T *)(uintptr_t)addr = v; }

// One exact sphere test (sphere.rs:99-121), the arithmetic of closest_brute / exact_sphere, up to the root x and whether it lies within
// [mint, maxt] (a NaN root does: the reference's range tests pass it).  `accept(x, in)` is the caller's rule for a root -- list order, ties to
// the lower index, the first one -- and runs under the branch of the root, so a wave in which no lane has a root skips it.
template <bool MOVING, class Accept>
__device__ __forceinline__ void q_sphere_root(f4 g, f4 vv, v3 o, v3 d, float tm, float a, float ra, bool a_plain, float mint, float maxt, Accept accept) {
    float cx = g.x, cy = g.y, cz = g.z;
    if (MOVING) { cx = cx + vv.x * tm; cy = cy + vv.y * tm; cz = cz + vv.z * tm; }       // sphere.rs:100
    const float ocx = o.x - cx, ocy = o.y - cy, ocz = o.z - cz;
    const float b = ocx * d.x + ocy * d.y + ocz * d.z;
    const float c = (ocx * ocx + ocy * ocy + ocz * ocz) - g.w;
    const float disc = b * b - a * c;
    if (!(disc < 0.0f)) {
        const float x = sphere_root(b, disc, a, ra, a_plain, mint);
        accept(x, !(x < mint || x > maxt));
    }
}

// The per-lane walk of the sphere tree with its stack in LDS ([level][thread], one conflict-free row per level; level 0 holds the sentinel),
// the nearer child first.  `sp0`: LDS byte address of the lane's level-0 slot, `sp_top` of its last level.  `start`: bv.root, or RTW_Q_DONE
// for a lane that a sphere outside the tree has already settled.  `hi()`: the largest root the caller still accepts, read at every inner
// node.  `leaf(s)`: the caller's exact test of sphere s; true ends the lane, its node becomes the sentinel.
template <class Hi, class Leaf>
__device__ __forceinline__ void q_tree_walk(const DevBvh &bv, v3 o, v3 d, float a, float mint, uint32_t sp0, uint32_t sp_top, int start, Hi hi, Leaf leaf,
                                            uint32_t &n_tests, uint32_t &n_nodes, bool &overflow) {
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
    const float lo_lim = mint - tau;

    const uint32_t level = RTW_BLOCK * 4u;
    uint32_t sp = sp0;
    q_lds_put<int>(sp, RTW_Q_DONE);
    int node = start;
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
            const float hi_lim = hi() + tau;
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
        if (node < 0 && node != RTW_Q_DONE) {                      // a leaf: the exact test, then the sentinel or the next entry off the stack
            n_tests++;
            if (leaf((uint32_t)~node)) node = RTW_Q_DONE;
            else { node = q_lds_get<int>(sp); sp -= level; }
        }
    }
}

// Can the tree answer this ray?  The pruning presumes the reference's quadratic in ORDINARY f32 (rtw_shim.hip decides the same for a
// render from its camera): a finite ray, |o| + |d| below 2^60, d.d within [1e-30, 1e30], and |d| x (the farthest centre + |o|) below 1e18.
// Any other ray (NaN roots pass the reference's range tests: an order-dependent answer) walks the list.
__device__ __forceinline__ bool q_ray_ordinary(v3 o, v3 d, float a, float span) {
    const float no = __builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z);
    const float nd = __builtin_fabsf(d.x) + __builtin_fabsf(d.y) + __builtin_fabsf(d.z);
    return no + nd < 0x1p60f && a >= 1e-30f && a <= 1e30f && fmaxf(nd, 2.0f) * (span + no + 1.0f) <= 1e18f;      // (nd >= |d|; NaN fails)
}

// The LDS byte address of the calling lane's level-0 stack slot, and of its last level
__device__ __forceinline__ uint32_t q_stack_base(const unsigned char *q_lds) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)q_lds + threadIdx.x * 4u;
}
__device__ __forceinline__ uint32_t q_stack_top(uint32_t sp0, uint32_t levels) { return sp0 + (levels - 1u) * (RTW_BLOCK * 4u); }

// Ray i of an [n][6] array = o, d
__device__ __forceinline__ void q_ray_load(const float *rays, uint32_t i, v3 &o, v3 &d) {
    const float2 *r = (const float2 *)(rays + 6 * (size_t)i);
    const float2 r0 = r[0], r1 = r[1], r2 = r[2];
    o = mk(r0.x, r0.y, r1.x); d = mk(r1.y, r2.x, r2.y);
}

// The ray of pixel i = (i % width, i / width) of Rust2's camera, the rule of rtw_depth_rays (Rust2/src/viewport.rs:77-80 then :63):
// left_top + delta_x * (i / width) + delta_y * (j / height), normalised
__device__ __forceinline__ void q_pixel_ray(const RtwCamera &cam, uint32_t width, uint32_t height, uint32_t i, v3 &o, v3 &d) {
    const uint32_t px = i % width, py = i / width;
    const float fx = (float)px / (float)width, fy = (float)py / (float)height;
    o = ld3(cam.origin);
    d = unit((ld3(cam.pixel00) + ld3(cam.delta_u) * fx) + ld3(cam.delta_v) * fy);
}

// The counters of a lane summed over the wave, one atomic per wave and counter (as tri_hits_kernel), on the workgroup's line of `counters`.
// n_fifth: the wave's count of what the pass casts ([4]: the points of ambient_occlusion_kernel, the rays of direct_light_kernel), 0 for
// the passes that have none.  ONE sequence with two ways in, because the compiler's register allocation follows the way in: the any-hit
// kernels call q_count_flush (written out in them, the eight round-loop builds of direct_light_kernel take a VGPR more), scene_hits_kernel
// writes RTW_Q_COUNT_FLUSH as its last statement (through the function, in every form tried -- by value, by reference, the counts as one
// struct, the fifth counter compiled out -- three of its builds spill other numbers of SGPRs).  `make asm` shows both.
#define RTW_Q_COUNT_FLUSH(counters, n_sph, n_nodes, n_quad, overflow, n_fifth) do { \
    unsigned long long s0 = n_sph, s1 = n_nodes, s2 = n_quad; \
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); } \
    const bool any_overflow = ballot64(overflow) != 0ull; \
    if ((threadIdx.x & 63u) == 0) { \
        unsigned long long *line = (counters) + (blockIdx.x % RTW_QUERY_SLOTS) * RTW_QUERY_STRIDE; \
        if (s0) atomicAdd(&line[0], s0); \
        if (s1) atomicAdd(&line[1], s1); \
        if (s2) atomicAdd(&line[2], s2); \
        if (any_overflow) atomicAdd(&line[3], 1ull); \
        if (n_fifth) atomicAdd(&line[4], (unsigned long long)(n_fifth)); \
    } } while (0)
__device__ __forceinline__ void q_count_flush(unsigned long long *counters, uint32_t n_sph, uint32_t n_nodes, uint32_t n_quad, bool overflow,
                                              uint32_t n_fifth) {
    RTW_Q_COUNT_FLUSH(counters, n_sph, n_nodes, n_quad, overflow, n_fifth);
}

// The lane mapping of the fused passes: L = min(samples, 64) lanes form a group that owns one item, a wave holds 64 / L items, and a lane
// takes sample k = g_lane + round * L in samples / L rounds.  (wave-uniform in L: samples is a kernel argument)
struct LaneGroup {
    uint32_t L, g_lane, g_first;  // lanes of a group, the lane's place in its group, the wave lane of the group's lane 0
    unsigned long long item;      // the group's item, which may lie past the end
    unsigned long long g_mask;    // the group's lanes in a ballot
};
__device__ __forceinline__ LaneGroup q_lane_group(uint32_t lg) {
    LaneGroup G;
    G.L = 1u << lg;
    const uint32_t lane = threadIdx.x & 63u;
    G.g_lane = lane & (G.L - 1u); G.g_first = lane - G.g_lane;
    G.item = (unsigned long long)blockIdx.x * (RTW_BLOCK >> lg) + (threadIdx.x >> lg);
    G.g_mask = (G.L == 64u ? ~0ull : ((1ull << G.L) - 1ull)) << G.g_first;
    return G;
}

// The surface point i of a group and its normal: lane 0 of the group loads them -- CAM: forms them from the depth pass's depth, index and
// normal of pixel i and the pixel's ray, the normal faced towards the viewer -- and the group gets them by a cross-lane read.  `in`: the
// group's item exists; else, and for a miss pixel, the point and the normal stay 0 0 0.  Every lane of the wave must be here: the cross-lane
// read finds its source lane active only then, which is why no lane of a fused pass leaves before its end.  A: AoArgs or DirectArgs, which
// name the fields read here alike (points, normals, cam, width, height, depth, idx).
struct GroupPoint { v3 p, nrm; };
template <bool CAM, class A>
__device__ __forceinline__ GroupPoint q_group_point(const A &S, const LaneGroup &G, bool in, uint32_t i) {
    v3 p = mk(0.0f, 0.0f, 0.0f), nrm = p;
    if (in && G.g_lane == 0u) {
        if (CAM) {
            if (S.idx[i] >= 0) {                                   // (a miss pixel is skipped: its normal stays 0 0 0)
                v3 o, d;
                q_pixel_ray(S.cam, S.width, S.height, i, o, d);
                const v3 nn = ld3(S.normals + 3 * (size_t)i);
                p = o + d * S.depth[i];
                nrm = dot(d, nn) > 0.0f ? -nn : nn;                // faced towards the viewer
            }
        } else {
            p = ld3(S.points + 3 * (size_t)i);
            nrm = ld3(S.normals + 3 * (size_t)i);
        }
    }
    if (G.L > 1u) {
        p.x = __shfl(p.x, (int)G.g_first); p.y = __shfl(p.y, (int)G.g_first); p.z = __shfl(p.z, (int)G.g_first);
        nrm.x = __shfl(nrm.x, (int)G.g_first); nrm.y = __shfl(nrm.y, (int)G.g_first); nrm.z = __shfl(nrm.z, (int)G.g_first);
    }
    return { p, nrm };
}

} // namespace

} // namespace rtw
