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
// The exact sphere test, the tree walk, q_ray_ordinary and the counters are rtw_scene_walk.h's, the ONE definition this file shares with
// rtw_query.hip: what differs between the passes is the acceptance of a root in range and what a leaf does to its lane, both written here.
#include "rtw_scene_walk.h"
#include "rtw_occl.h"
#include "rtw_ao.h"
#include "rtw_direct.h"

namespace rtw {

namespace {

// One sphere candidate of the any-hit pass: rtw_query.hip's q_sphere with nothing found so far.  LIST: the list walk's first candidate
// (`min_hit == None`), which a NaN root enters; else the tree's (best_t = maxt, best = -1: x < maxt || x == maxt, which a NaN root fails
// there as here -- the host's and q_ray_ordinary's conditions keep such roots out of the tree, and the two passes stay equal if one gets in).
template <bool MOVING, bool LIST>
__device__ __forceinline__ bool q_sphere_any(f4 g, f4 vv, v3 o, v3 d, float tm, float a, float ra, bool a_plain, float mint, float maxt) {
    bool take = false;
    q_sphere_root<MOVING>(g, vv, o, d, tm, a, ra, a_plain, mint, maxt, [&](float x, bool in) { take = in && (LIST ? true : (x < maxt || x == maxt)); });
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

// The sphere group through the tree, rtw_query.hip's q_sphere_tree's order: the spheres kept outside it first, until a ballot says no lane
// is open, then q_tree_walk.  A lane ends at its first accepted sphere: one outside the tree starts it at the sentinel, a leaf makes its
// node the sentinel.  Nothing is found until then, so the walk prunes against maxt: hi_lim is a constant of the ray.  Every lane here is open.
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
    q_tree_walk(bv, o, d, a, mint, sp0, sp_top, hit ? RTW_Q_DONE : bv.root, [&] { return maxt; },
                [&](uint32_t s) {
                    hit = q_sphere_any<MOVING, false>(sc.geom[s], MOVING ? sc.vel[s] : f4{ 0, 0, 0, 0 }, o, d, tm, a, ra, a_plain, mint, maxt);
                    return hit;
                },
                n_tests, n_nodes, overflow);
    return hit;
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
            const uint32_t sp0 = q_stack_base(q_lds);
            if (q_sphere_tree_any<MOVING>(A.sc, A.bvh, o, d, tm, a, ra, a_plain, mint, maxt, sp0, q_stack_top(sp0, A.levels), n_sph, n_nodes,
                                          overflow)) open = false;
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

} // namespace

// TREE: the sphere group goes through the tree (stack in dynamic LDS).  One ray per lane.
template <bool TREE, bool MOVING>
__global__ __launch_bounds__(RTW_BLOCK) void scene_occluded_kernel(const OccludedArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const uint32_t i = blockIdx.x * RTW_BLOCK + threadIdx.x;
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    if (i < A.n) {
        v3 o, d;
        q_ray_load(A.rays, i, o, d);
        const bool open = occluded_walk<TREE, MOVING>(A, q_lds, o, d, true, n_sph, n_nodes, n_quad, overflow);
        A.out[i] = open ? (uint8_t)0 : (uint8_t)1;
    }
    q_count_flush(A.counters, n_sph, n_nodes, n_quad, overflow, 0u);
}

// Ambient occlusion (rtw_ctx_ambient_occlusion / rtw_ctx_ao_map): a group of lanes owns one point (q_lane_group) and gets
// it and its normal from its lane 0 (q_group_point).  Every lane makes its ray in registers (rtw_ao.h) and walks it with occluded_walk; a
// round's occluded count is the popcount of a ballot under the group's lane mask.  No lane leaves before the end: every cross-lane read
// finds its source lane active.
// ONE: samples <= 64, a single round.  Nothing of the point then lives across the walk (the point, the normal, the stream's prefix and the
// frame the compiler hoists out of the round loop: up to 37 VGPRs), and the build keeps the 7 waves per SIMD of scene_occluded_kernel; the
// build with the loop runs at 4 - 5.
template <bool CAM, bool TREE, bool MOVING, bool ONE>
__global__ __launch_bounds__(RTW_BLOCK) void ambient_occlusion_kernel(const AoArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const LaneGroup G = q_lane_group(A.lg_group);
    const bool in = G.item < A.q.n;
    const uint32_t i = (uint32_t)G.item;
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    const GroupPoint gp = q_group_point<CAM>(A, G, in, i);
    const v3 p = gp.p, nrm = gp.nrm;
    const lv3 ln = lmk(nrm.x, nrm.y, nrm.z);
    const bool casts = in && !ao_skipped(ln);                      // (a point past n has the normal 0 0 0 as well)
    const uint32_t base = ao_point_base(A.seed, i);
    uint32_t occluded = 0;
    for (uint32_t round = 0; round < (ONE ? 1u : A.samples); round += (ONE ? 1u : G.L)) {   // (samples / L rounds, wave-uniform; ONE: no loop)
        const lv3 dir = ao_dir(base, round + G.g_lane, ln);
        const bool open = occluded_walk<TREE, MOVING>(A.q, q_lds, p, mk(dir.x, dir.y, dir.z), casts, n_sph, n_nodes, n_quad, overflow);
        occluded += (uint32_t)__builtin_popcountll(ballot64(!open) & G.g_mask);
    }
    if (in && G.g_lane == 0u) A.ao_out[i] = casts ? (float)(A.samples - occluded) * (1.0f / (float)A.samples) : 1.0f;
    const uint32_t n_points = (uint32_t)__builtin_popcountll(ballot64(casts && G.g_lane == 0u));
    q_count_flush(A.q.counters, n_sph, n_nodes, n_quad, overflow, n_points);
}

// Direct lighting (rtw_ctx_direct_light / rtw_ctx_direct_light_map): ambient_occlusion_kernel's lane mapping over ITEMS.  A
// group owns item i * n_lights + l -- point i under light l --, so the groups of a wave may belong to different points and lights.  Every
// lane reads the light's row, makes its segment and weight in registers (rtw_direct.h) and walks the segment with occluded_walk, coming in
// closed when the sample is not cast.  The visible count is the popcount of a ballot under the group's lane mask; the weights are summed in
// the fixed association of direct_sum: a lane's rounds in ascending order, then lane g adds lane g + off for off = L/2 .. 1 (a lane with
// g >= off adds something that nobody reads).  No lane leaves before the end, as above.
// ONE: samples <= 64, no round loop (as ambient_occlusion_kernel: nothing of the item but its weight lives across the walk).
template <bool CAM, bool TREE, bool MOVING, bool ONE>
__global__ __launch_bounds__(RTW_BLOCK) void direct_light_kernel(const DirectArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const LaneGroup G = q_lane_group(A.lg_group);
    const bool in = G.item < (unsigned long long)A.q.n * A.n_lights;
    const uint32_t it = (uint32_t)G.item;
    const uint32_t i = in ? it / A.n_lights : 0u, l = in ? it - i * A.n_lights : 0u;      // (an item past the end reads row 0 and casts nothing)
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    const GroupPoint gp = q_group_point<CAM>(A, G, in, i);
    const v3 p = gp.p, nrm = gp.nrm;
    const lv3 lp = lmk(p.x, p.y, p.z), ln = lmk(nrm.x, nrm.y, nrm.z);
    const DirectRow row = A.lights[l];
    const uint32_t base = direct_item_base(A.seed, i, l);
    uint32_t visible = 0, n_cast = 0;
    float sum = 0.0f;
    for (uint32_t round = 0; round < (ONE ? 1u : A.samples); round += (ONE ? 1u : G.L)) {   // (samples / L rounds, wave-uniform; ONE: no loop)
        lv3 dir;
        float W;
        const bool cast = direct_sample(row, base, round + G.g_lane, lp, ln, dir, W) && in;
        const bool open = occluded_walk<TREE, MOVING>(A.q, q_lds, p, mk(dir.x, dir.y, dir.z), cast, n_sph, n_nodes, n_quad, overflow);
        visible += (uint32_t)__builtin_popcountll(ballot64(open) & G.g_mask);            // (open at the end: cast and free)
        n_cast += (uint32_t)__builtin_popcountll(ballot64(cast));                        // (the wave's; wave-uniform)
        sum = sum + (open ? W : 0.0f);
    }
    for (uint32_t off = G.L >> 1; off > 0u; off >>= 1) sum = sum + __shfl_down(sum, off);
    if (in && G.g_lane == 0u) {
        const float inv = 1.0f / (float)A.samples;
        A.vis_out[it] = (float)visible * inv;
        if (A.irr_out) A.irr_out[it] = sum * inv;
    }
    q_count_flush(A.q.counters, n_sph, n_nodes, n_quad, overflow, n_cast);
}

void launch_scene_occluded(const OccludedArgs &q, bool tree, hipStream_t stream) {
    typedef void (*occl_fn)(const OccludedArgs);
    const occl_fn fn = with_bools([](auto tr, auto moving) -> occl_fn { return scene_occluded_kernel<tr.value, moving.value>; },
                                  tree, q.sc.moving != 0u);
    const uint32_t lds = tree ? q.levels * RTW_BLOCK * 4u : 0u;
    hipLaunchKernelGGL(fn, dim3((q.n + RTW_BLOCK - 1) / RTW_BLOCK), dim3(RTW_BLOCK), lds, stream, q);
}

void launch_ambient_occlusion(const AoArgs &q, bool from_camera, bool tree, hipStream_t stream) {
    typedef void (*ao_fn)(const AoArgs);
    const ao_fn fn = with_bools([](auto cam, auto tr, auto moving, auto one) -> ao_fn {
        return ambient_occlusion_kernel<cam.value, tr.value, moving.value, one.value>;
    }, from_camera, tree, q.q.sc.moving != 0u, q.samples <= 64u);
    const uint32_t lds = tree ? q.q.levels * RTW_BLOCK * 4u : 0u;
    const uint32_t per_block = RTW_BLOCK >> q.lg_group;        // points of a workgroup
    hipLaunchKernelGGL(fn, dim3((uint32_t)(((unsigned long long)q.q.n + per_block - 1u) / per_block)), dim3(RTW_BLOCK), lds, stream, q);
}

void launch_direct_light(const DirectArgs &q, bool from_camera, bool tree, hipStream_t stream) {
    typedef void (*direct_fn)(const DirectArgs);
    const direct_fn fn = with_bools([](auto cam, auto tr, auto moving, auto one) -> direct_fn {
        return direct_light_kernel<cam.value, tr.value, moving.value, one.value>;
    }, from_camera, tree, q.q.sc.moving != 0u, q.samples <= 64u);
    const uint32_t lds = tree ? q.q.levels * RTW_BLOCK * 4u : 0u;
    const uint32_t per_block = RTW_BLOCK >> q.lg_group;        // items of a workgroup
    const unsigned long long items = (unsigned long long)q.q.n * q.n_lights;
    hipLaunchKernelGGL(fn, dim3((uint32_t)((items + per_block - 1u) / per_block)), dim3(RTW_BLOCK), lds, stream, q);
}

} // namespace rtw
