// rtw_query.hip -- scene ray queries (rtw_ctx_scene_hits) and Rust2's depth_map (rtw_ctx_depth_map, Rust2/src/viewport.rs:62-85): ONE
// closest-hit query per ray over all four groups of a context's scene -- spheres, quads, instances, triangles -- with no path around it.
// A kernel of its own: no render kernel reads this file.
//
// Every value reported is the render's: the sphere root is sphere_root() (rtw_device.h), quads and instances go through quad_pick /
// instance_pick, triangles through tri_closest (rtw_tri.h) or the zero-safe tree walk (tri_tree_walk, rtw_mesh.h), mesh placements through mesh_closest, and the tie rule is Scene::collision_normal's as the oracle restates it
// (closest_hit): within a group the first of equal t in list order, a later group only when strictly closer.  The sphere tree only prunes
// (DESIGN.md "Conservative traversal"; the per-ray paddings below are those of render_bvh's trav_begin, global-node variant), and every
// surviving candidate runs the exact test with ties to the lower index, so RTW_ACCEL_BVH answers bit for bit what RTW_ACCEL_BRUTE answers.
// Constant-density instances are skipped: their hit is a random free path, and a query has no sample stream.
#include "rtw_kernels.h"
#include "rtw_mesh.h"

namespace rtw {

namespace {

#define RTW_Q_KU 1.4305115e-6f      /* 24 * 2^-24: the rounding bound of the reference's quadratic (rtw_kernels.hip RTW_KU) */
#define RTW_Q_DONE ((int)0x80000000) /* stack sentinel / empty tree (DevBvh.root of an empty tree is the same value) */

template <class T> __device__ __forceinline__ T q_lds_get(uint32_t addr) { return *(const __attribute__((address_space(3))) T *)(uintptr_t)addr; }
template <class T> __device__ __forceinline__ void q_lds_put(uint32_t addr, T v) { *(__attribute__((address_space(3))) T *)(uintptr_t)addr = v; }

// One exact sphere test (sphere.rs:99-121), the arithmetic of closest_brute / exact_sphere.  LIST: candidates come in list order, the
// reference's `min_hit == None || min_hit > i` (a NaN root can only enter first); else: any order, ties to the lower index, best_t starts at maxt.
template <bool MOVING, bool LIST>
__device__ __forceinline__ void q_sphere(f4 g, f4 vv, uint32_t s, v3 o, v3 d, float tm, float a, float ra, bool a_plain, float mint, float maxt,
                                         int &best, float &best_t) {
    float cx = g.x, cy = g.y, cz = g.z;
    if (MOVING) { cx = cx + vv.x * tm; cy = cy + vv.y * tm; cz = cz + vv.z * tm; }       // sphere.rs:100
    const float ocx = o.x - cx, ocy = o.y - cy, ocz = o.z - cz;
    const float b = ocx * d.x + ocy * d.y + ocz * d.z;
    const float c = (ocx * ocx + ocy * ocy + ocz * ocz) - g.w;
    const float disc = b * b - a * c;
    if (!(disc < 0.0f)) {
        const float x = sphere_root(b, disc, a, ra, a_plain, mint);
        const bool in = !(x < mint || x > maxt);
        const bool take = in && (LIST ? (best < 0 || best_t > x) : (x < best_t || (x == best_t && s < (uint32_t)best)));
        best = take ? (int)s : best; best_t = take ? x : best_t;
    }
}

// The sphere group in list order (wave-uniform index, scalar loads)
template <bool MOVING>
__device__ __forceinline__ void q_sphere_list(const DevScene &sc, v3 o, v3 d, float tm, float a, float ra, bool a_plain, float mint, float maxt,
                                              int &best, float &best_t) {
    cf4_ptr geom = (cf4_ptr)(uintptr_t)sc.geom;
    cf4_ptr vel = (cf4_ptr)(uintptr_t)sc.vel;
    const f4 zero = { 0, 0, 0, 0 };
    best = -1; best_t = 0.0f;
    for (uint32_t s = 0; s < sc.n; ++s) q_sphere<MOVING, true>(geom[s], MOVING ? vel[s] : zero, s, o, d, tm, a, ra, a_plain, mint, maxt, best, best_t);
}

// The sphere group through the tree: the spheres kept outside it first, then a per-lane walk with its stack in LDS ([level][thread], one
// conflict-free row per level; level 0 holds the sentinel).  `sp0`: LDS byte address of the lane's level-0 slot, `sp_top` of its last level.
template <bool MOVING>
__device__ __forceinline__ void q_sphere_tree(const DevScene &sc, const DevBvh &bv, v3 o, v3 d, float tm, float a, float ra, bool a_plain,
                                              float mint, float maxt, uint32_t sp0, uint32_t sp_top, int &best, float &best_t,
                                              uint32_t &n_tests, uint32_t &n_nodes, bool &overflow) {
    best = -1; best_t = maxt;
    {
        cf4_ptr bg = (cf4_ptr)(uintptr_t)bv.big_geom;
        cf4_ptr bvel = (cf4_ptr)(uintptr_t)bv.big_vel;
        typedef const uint32_t __attribute__((address_space(4))) *cu32_ptr;
        cu32_ptr bidx = (cu32_ptr)(uintptr_t)bv.big_index;
        for (uint32_t k = 0; k < bv.n_big; ++k)
            q_sphere<MOVING, false>(bg[k], MOVING ? bvel[k] : f4{ 0, 0, 0, 0 }, bidx[k], o, d, tm, a, ra, a_plain, mint, maxt, best, best_t);
        n_tests += bv.n_big;
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
    const float lo_lim = mint - tau;

    const uint32_t level = RTW_BLOCK * 4u;
    uint32_t sp = sp0;
    q_lds_put<int>(sp, RTW_Q_DONE);
    int node = bv.root;
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
            const float hi_lim = best_t + tau;
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
        if (node < 0 && node != RTW_Q_DONE) {                      // a leaf: the exact test, then the next entry off the stack
            const uint32_t s = (uint32_t)~node;
            q_sphere<MOVING, false>(sc.geom[s], MOVING ? sc.vel[s] : f4{ 0, 0, 0, 0 }, s, o, d, tm, a, ra, a_plain, mint, maxt, best, best_t);
            n_tests++;
            node = q_lds_get<int>(sp); sp -= level;
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

} // namespace

// CAM: the ray of pixel i is built from the camera by the rule of rtw_depth_rays; else it is read from A.rays.  NORMALS: normal_out is
// written (the stores and the winner's normal compile out otherwise).  TREE: the sphere group goes through the tree (stack in dynamic LDS).
template <bool CAM, bool NORMALS, bool TREE, bool MOVING>
__global__ __launch_bounds__(RTW_BLOCK) void scene_hits_kernel(const QueryArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const uint32_t i = blockIdx.x * RTW_BLOCK + threadIdx.x;
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    if (i < A.n) {
        v3 o, d;
        if (CAM) {
            // Rust2/src/viewport.rs:77-80 then :63: left_top + delta_x * (i / width) + delta_y * (j / height), normalised
            const uint32_t px = i % A.width, py = i / A.width;
            const float fx = (float)px / (float)A.width, fy = (float)py / (float)A.height;
            o = ld3(A.cam.origin);
            d = unit((ld3(A.cam.pixel00) + ld3(A.cam.delta_u) * fx) + ld3(A.cam.delta_v) * fy);
        } else {
            const float2 *r = (const float2 *)(A.rays + 6 * (size_t)i);
            const float2 r0 = r[0], r1 = r[1], r2 = r[2];
            o = mk(r0.x, r0.y, r1.x); d = mk(r1.y, r2.x, r2.y);
        }
        const float tm = A.time, mint = A.mint, maxt = A.maxt;
        const float a = dot(d, d);
        const float ra = rcp_refined(a);
        const bool a_plain = ballot64(!in_range(a, 0x1p-20f, 0x1p20f)) == 0ull;          // see sphere_root()
        // ---- spheres ----
        int best = -1; float best_t = 0.0f;
        bool listed = true;
        if (TREE) {
            if (q_ray_ordinary(o, d, a, A.span)) {
                const uint32_t sp0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)q_lds + threadIdx.x * 4u;
                q_sphere_tree<MOVING>(A.sc, A.bvh, o, d, tm, a, ra, a_plain, mint, maxt, sp0, sp0 + (A.levels - 1u) * (RTW_BLOCK * 4u), best, best_t,
                                      n_sph, n_nodes, overflow);
                listed = false;
            }
        }
        if (listed) { q_sphere_list<MOVING>(A.sc, o, d, tm, a, ra, a_plain, mint, maxt, best, best_t); n_sph += A.sc.n; }
        bool found = best >= 0;
        float ht = best_t;
        int idx = best;
        int win = 0;                                               // 0: sphere `best`, 1: quad qk, 2: instance ii (member icode), 3: triangle tk, 4: triangle tk of placement mk
        // ---- quads: the closest in list order, then against the spheres (strictly closer) ----
        const DevGeom &g = A.geom;
        uint32_t qk = 0;
        {
            bool qfound = false; float qt = 0.0f;
            for (uint32_t k = 0; k < g.n_quads; ++k) {
                float t;
                if (quad_pick(g.quads, k, o, d, mint, maxt, qfound, qt, t)) { qfound = true; qt = t; qk = k; }
            }
            n_quad += g.n_quads;
            if (qfound && (!found || ht > qt)) { ht = qt; found = true; win = 1; idx = (int)(A.sc.n + qk); }
        }
        // ---- instances (instance.rs:250-310), media skipped ----
        bool ifound = false; float it = 0.0f; uint32_t ii = 0; int icode = 0;
        for (uint32_t k = 0; k < g.n_inst; ++k) {
            const DevInstance in = g.inst[k];
            if (in.medium == RTW_MEDIUM_CONST_DENSITY) continue;
            const v3 tr = ld3(in.tr);
            v3 lo, ld;
            if (A.inst_quats) { const quat qn = inst_quat(A.inst_quats, k); lo = quat_rot(qn, o - tr); ld = quat_rot(qn, d); }   // (a wave-uniform branch)
            else { lo = rotated(o - tr, in.back, in.back_k); ld = rotated(d, in.back, in.back_k); }
            float ct; int code;
            if (!instance_pick(g, in, lo, ld, tm, mint, maxt, ct, code, n_sph, n_quad)) continue;
            if (!ifound || it > ct) { it = ct; ii = k; icode = code; ifound = true; }
        }
        if (ifound && (!found || ht > it)) { ht = it; found = true; win = 2; idx = (int)(A.sc.n + g.n_quads + ii); }
        // ---- triangles last ----
        int tk = -1, mp = -1;
        if (A.mesh_rows) {                                         // (a wave-uniform branch) the placements stand in for the world-space triangles
            float tt;
            mp = mesh_closest(A.tris, A.mesh_rows, A.n_mesh, A.mesh_top, A.n_mesh_top, o, d, mint, maxt, found, ht, tk, tt, n_quad, n_nodes);
            if (mp >= 0) { ht = tt; found = true; win = 4; idx = (int)(A.sc.n + g.n_quads + g.n_inst) + mp; }
        } else if (A.tris.n) {
            float tt;
            if (A.tris.nodes != nullptr && tri_ray_ordinary(A.tris, o, d)) tk = tri_tree_walk(A.tris, o, d, mint, maxt, found, ht, tt, n_quad, n_nodes);
            else tk = tri_closest(A.tris, o, d, mint, maxt, found, ht, tt, n_quad, n_nodes);          // (the list walk)
            if (tk >= 0) { ht = tt; found = true; win = 3; idx = (int)(A.sc.n + g.n_quads + g.n_inst) + tk; }
        }
        A.t_out[i] = found ? ht : A.miss_t;
        if (A.idx_out) A.idx_out[i] = found ? idx : -1;
        if (NORMALS) {
            v3 nrm = mk(0.0f, 0.0f, 0.0f);
            if (found) {
                if (win == 0) {                                    // sphere.rs:127
                    const f4 gg = A.sc.geom[best];
                    v3 c = mk(gg.x, gg.y, gg.z);
                    if (MOVING) { const f4 vv = A.sc.vel[best]; c = c + mk(vv.x, vv.y, vv.z) * tm; }
                    nrm = unit((o + d * ht) - c);
                } else if (win == 1) {
                    nrm = ld3(g.quads[qk].normal);
                } else if (win == 2) {                             // the member's normal in the instance's frame, rotated forward (instance.rs:304)
                    const DevInstance &in = g.inst[ii];
                    const v3 tr = ld3(in.tr);
                    const bool rq = A.inst_quats != nullptr;
                    quat qn = qmk(1.0f, 0.0f, 0.0f, 0.0f);
                    if (rq) qn = inst_quat_lane(A.inst_quats, ii);
                    const v3 lo = rq ? quat_rot(qn, o - tr) : rotated(o - tr, in.back, in.back_k), ld = rq ? quat_rot(qn, d) : rotated(d, in.back, in.back_k);
                    v3 ln;
                    if (icode >= 0) {
                        const f4 gg = g.igeom[icode], vv = g.ivel[icode];
                        const v3 c = mk(gg.x, gg.y, gg.z) + mk(vv.x, vv.y, vv.z) * tm;
                        ln = unit((lo + ld * ht) - c);
                    } else ln = ld3(g.iquads[(uint32_t)~icode].normal);
                    nrm = rq ? quat_rot(qn, ln) : rotated(ln, in.fwd, in.fwd_k);      // Rust2: q.rotate(n), the same q as on the way in
                } else if (win == 3) {
                    nrm = ld3(A.tris.list[tk].normal);
                } else {                                           // q.rotate(n'), the same q as on the way in
                    quat qn; v3 pos;
                    mesh_row_lane(A.mesh_rows, (uint32_t)mp, qn, pos);
                    nrm = mesh_rot(qn, ld3(A.tris.list[tk].normal));
                }
            }
            *reinterpret_cast<float3 *>(A.normal_out + 3 * (size_t)i) = make_float3(nrm.x, nrm.y, nrm.z);
        }
    }
    // counters: summed over the wave, one atomic per wave and counter (as tri_hits_kernel), on the workgroup's line of A.counters
    unsigned long long s0 = n_sph, s1 = n_nodes, s2 = n_quad;
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off); s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    const bool any_overflow = ballot64(overflow) != 0ull;
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long *line = A.counters + (blockIdx.x % RTW_QUERY_SLOTS) * RTW_QUERY_STRIDE;
        if (s0) atomicAdd(&line[0], s0);
        if (s1) atomicAdd(&line[1], s1);
        if (s2) atomicAdd(&line[2], s2);
        if (any_overflow) atomicAdd(&line[3], 1ull);
    }
}

typedef void (*query_fn)(const QueryArgs);
template <bool CAM, bool NORMALS, bool TREE>
static query_fn pick_query_moving(bool moving) {
    return moving ? scene_hits_kernel<CAM, NORMALS, TREE, true> : scene_hits_kernel<CAM, NORMALS, TREE, false>;
}
template <bool CAM, bool NORMALS>
static query_fn pick_query_tree(bool tree, bool moving) {
    return tree ? pick_query_moving<CAM, NORMALS, true>(moving) : pick_query_moving<CAM, NORMALS, false>(moving);
}

void launch_scene_hits(const QueryArgs &q, bool from_camera, bool tree, hipStream_t stream) {
    const bool normals = q.normal_out != nullptr, moving = q.sc.moving != 0u;
    const query_fn fn = from_camera ? (normals ? pick_query_tree<true, true>(tree, moving) : pick_query_tree<true, false>(tree, moving))
                                    : (normals ? pick_query_tree<false, true>(tree, moving) : pick_query_tree<false, false>(tree, moving));
    const uint32_t lds = tree ? q.levels * RTW_BLOCK * 4u : 0u;
    hipLaunchKernelGGL(fn, dim3((q.n + RTW_BLOCK - 1) / RTW_BLOCK), dim3(RTW_BLOCK), lds, stream, q);
}

} // namespace rtw
