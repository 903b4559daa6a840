// rtw_query.hip -- scene ray queries (rtw_ctx_scene_hits) and Rust2's depth_map (rtw_ctx_depth_map, Rust2/src/viewport.rs:62-85): ONE
// closest-hit query per ray over all four groups of a context's scene -- spheres, quads, instances, triangles -- with no path around it.
// A kernel of its own: no render kernel reads this file.
//
// Every value reported is the render's: the sphere root is sphere_root() (rtw_device.h), quads and instances go through quad_pick /
// instance_pick, triangles through tri_closest (rtw_tri.h) or the zero-safe tree walk (tri_tree_walk, rtw_mesh.h), mesh placements through mesh_closest, and the tie rule is Scene::collision_normal's as the oracle restates it
// (closest_hit): within a group the first of equal t in list order, a later group only when strictly closer.  The sphere tree only prunes
// (DESIGN.md "Conservative traversal"), and every surviving candidate runs the exact test with ties to the lower index, so RTW_ACCEL_BVH
// answers bit for bit what RTW_ACCEL_BRUTE answers.  Constant-density instances are skipped: their hit is a random free path, and a query
// has no sample stream.
//
// The exact sphere test up to its root, the tree walk with its paddings, q_ray_ordinary, the pixel ray, the ray load and the counter flush
// are rtw_scene_walk.h's, the ONE definition this file shares with the any-hit passes of rtw_occluded.hip.  What is this
// pass's own stays here: the acceptance of a root in range (q_sphere) and the loop over all the spheres kept outside the tree.
#include "rtw_scene_walk.h"
#include "rtw_mesh.h"
#include "rtw_pixel_ray.h"

namespace rtw {

namespace {

// One sphere candidate of the closest-hit pass: q_sphere_root's root, then this pass's acceptance.  LIST: candidates come in list order, the
// reference's `min_hit == None || min_hit > i` (a NaN root can only enter first); else: any order, ties to the lower index, best_t starts at maxt.
template <bool MOVING, bool LIST>
__device__ __forceinline__ void q_sphere(f4 g, f4 vv, uint32_t s, v3 o, v3 d, float tm, float a, float ra, bool a_plain, float mint, float maxt,
                                         int &best, float &best_t) {
    q_sphere_root<MOVING>(g, vv, o, d, tm, a, ra, a_plain, mint, maxt, [&](float x, bool in) {
        const bool take = in && (LIST ? (best < 0 || best_t > x) : (x < best_t || (x == best_t && s < (uint32_t)best)));
        best = take ? (int)s : best; best_t = take ? x : best_t;
    });
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

// The sphere group through the tree: the spheres kept outside it first, all n_big of them, then q_tree_walk from the root.  The walk prunes
// against the closest root so far, and no leaf ends the lane: a later sphere may be closer.
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
    q_tree_walk(bv, o, d, a, mint, sp0, sp_top, bv.root, [&] { return best_t; },
                [&](uint32_t s) {
                    q_sphere<MOVING, false>(sc.geom[s], MOVING ? sc.vel[s] : f4{ 0, 0, 0, 0 }, s, o, d, tm, a, ra, a_plain, mint, maxt, best, best_t);
                    return false;
                },
                n_tests, n_nodes, overflow);
}

} // namespace

// CAM: the ray of pixel i is built from the camera by the rule of rtw_depth_rays; else it is read from A.rays.  NORMALS: normal_out is
// written (the stores and the winner's normal compile out otherwise).  TREE: the sphere group goes through the tree (stack in dynamic LDS).
// SURF (rtw_ctx_scene_surface / rtw_ctx_surface_map): the winner's hit record as the render's SHADE step reads it -- albedo,
// emission, material -- is formed once, after the walk, by the render's own record functions, and written; the camera's ray may follow
// RTW_RAYS_PIXEL; normal_out may be null.  Everything of it compiles out of the other builds.
template <bool CAM, bool NORMALS, bool TREE, bool MOVING, bool SURF = false>
__global__ __launch_bounds__(RTW_BLOCK) void scene_hits_kernel(const QueryArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
    const uint32_t i = blockIdx.x * RTW_BLOCK + threadIdx.x;
    uint32_t n_sph = 0, n_nodes = 0, n_quad = 0;
    bool overflow = false;
    if (i < A.n) {
        v3 o, d;
        if (CAM) {
            if (SURF && A.ray_rule == RTW_RAYS_PIXEL) {            // (a wave-uniform branch) Viewport's pixel ray, RTW_SAMPLER_NO_RAND's at offset 0 0
                const uint32_t px = i % A.width, py = i / A.width;
                o = ld3(A.cam.origin);
                pixel_ray_dir(A.cam, px, py, A.off_x, A.off_y, d.x, d.y, d.z);
            } else q_pixel_ray(A.cam, A.width, A.height, i, o, d);
        } else q_ray_load(A.rays, i, o, d);
        const float tm = A.time, mint = A.mint, maxt = A.maxt;
        const float a = dot(d, d);
        const float ra = rcp_refined(a);
        const bool a_plain = ballot64(!in_range(a, 0x1p-20f, 0x1p20f)) == 0ull;          // see sphere_root()
        // ---- spheres ----
        int best = -1; float best_t = 0.0f;
        bool listed = true;
        if (TREE) {
            if (q_ray_ordinary(o, d, a, A.span)) {
                const uint32_t sp0 = q_stack_base(q_lds);
                q_sphere_tree<MOVING>(A.sc, A.bvh, o, d, tm, a, ra, a_plain, mint, maxt, sp0, q_stack_top(sp0, A.levels), best, best_t, n_sph, n_nodes,
                                      overflow);
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
            if (!SURF || A.normal_out) *reinterpret_cast<float3 *>(A.normal_out + 3 * (size_t)i) = make_float3(nrm.x, nrm.y, nrm.z);
        }
        if (SURF) {                                                // the winner's record, with the operands the render gives the same functions
            v3 cm = mk(0.0f, 0.0f, 0.0f), em = cm, mt = cm;
            if (found) {
                const DevNoise nz = { nullptr, nullptr };          // (never read: a context with texture noise is refused)
                GeomHit h;
                if (win == 0) {                                    // shade_hit (rtw_kernels.hip)
                    const f4 gg = A.sc.geom[best];
                    v3 c = mk(gg.x, gg.y, gg.z);
                    if (MOVING) { const f4 vv = A.sc.vel[best]; c = c + mk(vv.x, vv.y, vv.z) * tm; }
                    const v3 normal = unit((o + d * ht) - c);
                    const DevMat mat = A.sc.mat[best];
                    h.emitted = ld3(mat.emitted);
                    if (A.rust2 && mat.tex >= 0) rust2_sphere_color(A.sc, mat, normal, h.cm, h.emitted);
                    else h.cm = sphere_albedo(A.sc, mat, normal);
                    h.m = mat_params(mat);
                } else if (win == 1) {
                    quad_record(A.sc, nz, g.quads, qk, o, d, ht, h);
                } else if (win == 2) {                             // in the instance's frame (geom_closest)
                    const DevInstance &in = g.inst[ii];
                    const v3 tr = ld3(in.tr);
                    v3 lo, ld;
                    if (A.inst_quats) { const quat qn = inst_quat_lane(A.inst_quats, ii); lo = quat_rot(qn, o - tr); ld = quat_rot(qn, d); }
                    else { lo = rotated(o - tr, in.back, in.back_k); ld = rotated(d, in.back, in.back_k); }
                    member_record(A.sc, nz, g, icode, lo, ld, tm, ht, h);
                } else if (win == 3) {
                    tri_record(A.sc, A.tris, (uint32_t)tk, o, d, ht, A.rust2 != 0u, h);
                } else {                                           // in the placement's frame (shade_geom)
                    quat qn; v3 pos;
                    mesh_row_lane(A.mesh_rows, (uint32_t)mp, qn, pos);
                    tri_record(A.sc, A.tris, (uint32_t)tk, mesh_rot(qn, o - pos), mesh_rot(qn, d), ht, true, h);
                }
                cm = h.cm; em = h.emitted; mt = mk(h.m.metallicness, h.m.opacity, h.m.ir);
            }
            *reinterpret_cast<float3 *>(A.albedo_out + 3 * (size_t)i) = make_float3(cm.x, cm.y, cm.z);
            if (A.emitted_out) *reinterpret_cast<float3 *>(A.emitted_out + 3 * (size_t)i) = make_float3(em.x, em.y, em.z);
            if (A.material_out) *reinterpret_cast<float3 *>(A.material_out + 3 * (size_t)i) = make_float3(mt.x, mt.y, mt.z);
            if (A.tri_out || A.bary_out) {                         // (a wave-uniform branch) the triangle under the ray and the point's place in it
                const bool on_tri = found && win >= 3;
                float alfa = 0.0f, beta = 0.0f;
                if (on_tri) {                                      // tri_inside on the ray tri_record was given, above
                    v3 lo = o, ld = d;
                    if (win == 4) {
                        quat qn; v3 pos;
                        mesh_row_lane(A.mesh_rows, (uint32_t)mp, qn, pos);
                        lo = mesh_rot(qn, o - pos); ld = mesh_rot(qn, d);
                    }
                    const DevTri &q = A.tris.list[tk];
                    tri_inside(q.origin, q.u, q.v, q.w, lo.x, lo.y, lo.z, ld.x, ld.y, ld.z, ht, alfa, beta);
                }
                if (A.tri_out) A.tri_out[i] = on_tri ? tk : -1;
                if (A.bary_out) *reinterpret_cast<float2 *>(A.bary_out + 2 * (size_t)i) = make_float2(alfa, beta);
            }
        }
    }
    RTW_Q_COUNT_FLUSH(A.counters, n_sph, n_nodes, n_quad, overflow, 0u);
}

void launch_scene_hits(const QueryArgs &q, bool from_camera, bool tree, hipStream_t stream) {
    typedef void (*query_fn)(const QueryArgs);
    const query_fn fn = q.albedo_out != nullptr                    // the surface builds: the normal is always formed, its store is a run-time check
        ? with_bools([](auto cam, auto tr, auto moving) -> query_fn {
              return scene_hits_kernel<cam.value, true, tr.value, moving.value, true>;
          }, from_camera, tree, q.sc.moving != 0u)
        : with_bools([](auto cam, auto normals, auto tr, auto moving) -> query_fn {
              return scene_hits_kernel<cam.value, normals.value, tr.value, moving.value>;
          }, from_camera, q.normal_out != nullptr, tree, q.sc.moving != 0u);
    const uint32_t lds = tree ? q.levels * RTW_BLOCK * 4u : 0u;
    hipLaunchKernelGGL(fn, dim3((q.n + RTW_BLOCK - 1) / RTW_BLOCK), dim3(RTW_BLOCK), lds, stream, q);
}

} // namespace rtw
