// rtw_mesh.h -- mesh placements: Rust2's `Instance` of triangles (Rust2/src/objects/instance.rs:215-255 around triangle.rs).  The context's
// triangle mesh is placed n times, each placement a position and a quaternion, all sharing the mesh's one tree (rtw.h "mesh
// placements").  Compiled by the placement build of the render kernels (SPEC 12), by the query kernel (rtw_query.hip) and by the kernel of
// rtw_ctx_mesh_instance_hits; the host pieces by rtw_tri.cpp.  The any-hit kernel (rtw_occluded.hip) reads it through rtw_occl.h, which holds
// the any-hit twins of the walks below.  No other kernel reads this file.
// The placement group's walk -- mesh_closest, with the top-level tree over the placements -- is ONE __host__ __device__
// definition: rtw_mesh_instance_hits_tree (rtw_tri.cpp) runs on the host what the kernels run.
#pragma once
#include "rtw_tri.h"
#include "rtw_quat.h"

namespace rtw {

// A placement as the device reads it: two f4 rows {qn.w, qn.x, qn.y, qn.z}, {position, 0}; qn = quat_normalised(q), formed on the host.

// ---- host and device: the rows of a placement list, and one placement's list walk ------------------------------------------------------
// The checks of rtw_ctx_set_mesh_instances on the placements themselves; rows ([2 n] f4, may be null) receives what the kernels read.
// One pose ([7] f32 = position xyz, quat wxyz: the layout of RtwMeshInstance): false for a component that is not finite or a quaternion whose
// len is 0 or not finite, else its two rows.  The host forms the rows of a list with it (mesh_rows), the device those of a moved placement
// (mesh_top_refit_leaf, rtw_refit.h): one definition, the same bits (1.0f / sqrtf correctly rounded on both sides, denormals kept).
__host__ __device__ inline bool mesh_pose_rows(const float *pose, f4 &a, f4 &b) {
    const quat q = qmk(pose[3], pose[4], pose[5], pose[6]);
    for (int k = 0; k < 3; k++) if (!(pose[k] - pose[k] == 0.0f)) return false;
    if (!(q.w - q.w == 0.0f) || !(q.x - q.x == 0.0f) || !(q.y - q.y == 0.0f) || !(q.z - q.z == 0.0f)) return false;
    const float l = quat_len(q);
    if (!(l > 0.0f) || !(l - l == 0.0f)) return false;
    const quat qn = quat_normalised(q);
    a.x = qn.w; a.y = qn.x; a.z = qn.y; a.w = qn.z;
    b.x = pose[0]; b.y = pose[1]; b.z = pose[2]; b.w = 0.0f;
    return true;
}

inline bool mesh_rows(const RtwMeshInstance *p, uint32_t n, f4 *rows) {
    static_assert(sizeof(RtwMeshInstance) == 7 * sizeof(float), "a placement is one pose");
    for (uint32_t i = 0; i < n; i++) {
        f4 a, b;
        if (!mesh_pose_rows(reinterpret_cast<const float *>(p + i), a, b)) return false;
        if (rows) { rows[2 * (size_t)i] = a; rows[2 * (size_t)i + 1] = b; }
    }
    return true;
}

// The placement group on the host: placements in list order, in each the triangle group rule on the local ray (tri_closest_host); a later
// placement only when strictly closer.  Returns the placement or -1; tri = its triangle, bt = its t.
inline int mesh_closest_host(const DevTri *list, uint32_t n_tris, const f4 *rows, uint32_t n, const float *r, float mint, float maxt,
                             int &tri, float &bt) {
    int best = -1; tri = -1; bt = 0.0f;
    for (uint32_t k = 0; k < n; k++) {
        const f4 a = rows[2 * (size_t)k], b = rows[2 * (size_t)k + 1];
        const quat qn = qmk(a.x, a.y, a.z, a.w);
        float ox, oy, oz, dx, dy, dz;
        quat_rotate_n(qn, r[0] - b.x, r[1] - b.y, r[2] - b.z, ox, oy, oz);
        quat_rotate_n(qn, r[3], r[4], r[5], dx, dy, dz);
        float t;
        const int j = tri_closest_host(list, n_tris, ox, oy, oz, dx, dy, dz, mint, maxt, t);
        if (j >= 0 && (best < 0 || bt > t)) { best = (int)k; tri = j; bt = t; }
    }
    return best;
}

// ---- host and device: the walks ------------------------------------------------------------------------------------------------------------
// The top-level tree's slab test pads a box by RTW_MESH_TOP_RAY_PAD |o|_inf per ray (512 u: c1 of DESIGN.md 4.11 is 464, beyond the 128 u of
// RTW_TRI_RAY_PAD, so the top nodes have a pad of their own) and serves rays with |o| + |d| t_bound <= RTW_MESH_TOP_REACH; placements lie
// within RTW_MESH_TOP_REACH of the origin (mesh_top_build), so that such a ray passes tri_ray_ordinary in every placement's frame: a rotation
// grows the inf-norm by at most sqrt(3), and sqrt(3) (1 + 32 u) (2^38 + 2^38) < 2^40.
#define RTW_MESH_TOP_RAY_PAD 0x1p-15f
#define RTW_MESH_TOP_REACH 0x1p38f

__host__ __device__ __forceinline__ uint32_t mesh_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
// The next f32 above a finite x: `t < mesh_next_up(x)` is `t <= x`
__host__ __device__ __forceinline__ float mesh_next_up(float x) {
    const uint32_t b = mesh_bits(x);
    if ((b << 1) == 0u) return __builtin_bit_cast(float, 1u);
    return __builtin_bit_cast(float, (b >> 31) ? b - 1u : b + 1u);
}

__host__ __device__ __forceinline__ v3 mesh_rot(quat qn, v3 a) {
    v3 o;
    quat_rotate_n(qn, a.x, a.y, a.z, o.x, o.y, o.z);
    return o;
}
// Rows of placement k for a per-lane k (the top-level tree's leaves; the record of the placement a lane's ray hit)
__host__ __device__ __forceinline__ void mesh_row_lane(const f4 *rows, uint32_t k, quat &qn, v3 &pos) {
    const f4 *q = rows + 2 * (size_t)k;
    const f4 a = q[0], b = q[1];
    qn = qmk(a.x, a.y, a.z, a.w); pos = mk(b.x, b.y, b.z);
}
// ... and for a wave-uniform k (the placement loop): scalar loads through the constant address space
__host__ __device__ __forceinline__ void mesh_row(const f4 *rows, uint32_t k, quat &qn, v3 &pos) {
#ifdef __HIP_DEVICE_COMPILE__
    cf4_ptr q = (cf4_ptr)(uintptr_t)(rows + 2 * (size_t)k);
    const f4 a = q[0], b = q[1];
    qn = qmk(a.x, a.y, a.z, a.w); pos = mk(b.x, b.y, b.z);
#else
    mesh_row_lane(rows, k, qn, pos);
#endif
}
// tri_load / tri_load_uniform (rtw_tri.h) for both sides: the host reads every row the plain way
__host__ __device__ __forceinline__ DevTri mesh_tri_load(const DevTri *base, uint32_t k) {
#ifdef __HIP_DEVICE_COMPILE__
    return tri_load(base, k);
#else
    return base[k];
#endif
}
__host__ __device__ __forceinline__ DevTri mesh_tri_load_uniform(const DevTri *base, uint32_t k) {
#ifdef __HIP_DEVICE_COMPILE__
    return tri_load_uniform(base, k);
#else
    return base[k];
#endif
}

// The slab test of one node {a = lo, skip; b = hi, leaf} of a TriNode tree for the ray (o, 1 / d) against [mint, lim]: the boxes padded by rr,
// the interval widened by RTW_TRI_T_PAD at each end, and -- any_zero -- the slab of an axis along which the direction is EXACTLY zero decided
// by where the origin lies (below).  The mesh's tree and the top-level tree over placements both test their nodes with it.
struct SlabRay { float ix, iy, iz; bool zx, zy, zz, any_zero; };
__host__ __device__ __forceinline__ SlabRay slab_ray(v3 d) {
    SlabRay s;
    s.ix = 1.0f / d.x; s.iy = 1.0f / d.y; s.iz = 1.0f / d.z;
    s.zx = d.x == 0.0f; s.zy = d.y == 0.0f; s.zz = d.z == 0.0f;
#ifdef __HIP_DEVICE_COMPILE__
    s.any_zero = ballot64(s.zx || s.zy || s.zz) != 0ull;            // wave-uniform: the selects below run only in waves that hold such a ray
#else
    s.any_zero = s.zx || s.zy || s.zz;
#endif
    return s;
}
__host__ __device__ __forceinline__ bool slab_hit(const SlabRay &s, f4 a, f4 b, v3 o, float rr, float mint, float lim) {
    const float BIG = 0x1.fffffep127f;
    float x0 = ((a.x - rr) - o.x) * s.ix, x1 = ((b.x + rr) - o.x) * s.ix;
    float y0 = ((a.y - rr) - o.y) * s.iy, y1 = ((b.y + rr) - o.y) * s.iy;
    float z0 = ((a.z - rr) - o.z) * s.iz, z1 = ((b.z + rr) - o.z) * s.iz;
    if (s.any_zero) {
        if (s.zx) { const bool in = (a.x - rr) <= o.x && o.x <= (b.x + rr); x0 = in ? -BIG : BIG; x1 = BIG; }
        if (s.zy) { const bool in = (a.y - rr) <= o.y && o.y <= (b.y + rr); y0 = in ? -BIG : BIG; y1 = BIG; }
        if (s.zz) { const bool in = (a.z - rr) <= o.z && o.z <= (b.z + rr); z0 = in ? -BIG : BIG; z1 = BIG; }
    }
    float ne = fminf(x0, x1), fa = fmaxf(x0, x1);
    ne = fmaxf(ne, fminf(y0, y1)); fa = fminf(fa, fmaxf(y0, y1));
    ne = fmaxf(ne, fminf(z0, z1)); fa = fminf(fa, fmaxf(z0, z1));
    ne = ne - __builtin_fabsf(ne) * RTW_TRI_T_PAD;
    fa = fa + __builtin_fabsf(fa) * RTW_TRI_T_PAD;
    return fmaxf(ne, mint) <= fminf(fa, lim);
}

// The triangle group through its tree: tri_closest's stackless walk (rtw_tri.h) -- the same boxes, paddings, candidates and tie rule --
// with the slab of an axis along which the direction is EXACTLY zero decided by where the origin lies instead of by 1 / 0.  There
// (lo - o) * inf is +-inf, the widening `ne - |ne| * pad` makes inf - inf = NaN, fmaxf / fminf drop the NaN and NO box is pruned any more: the
// ray visits every node and tests every triangle -- the right answer, a 200k-triangle list walk late.  A depth map meets such rays as a
// matter of course (pixel width / 2 of an axis-aligned camera has d.x == 0 down the whole column; DESIGN.md 4.8 has the measurement), and so
// does every ray of it that enters a placement with the identity quaternion.  With d.x == 0 the point o + d t keeps x = o.x for every t, so
// a box whose padded x-range does not hold o.x cannot hold a hit: pruning it is exact.
// The ONE zero-safe walk: the query kernel's triangle group, its placements, the placement build of the render kernels and the kernel of
// rtw_ctx_mesh_instance_hits all call it (tri_closest keeps its own copy: it is compiled into every SPEC 8 kernel, which do not change).
// Only for rays tri_ray_ordinary() accepts (finite, within the cull's reach) with the tree present; the others walk the list.
__host__ __device__ __forceinline__ int tri_tree_walk(const DevTris &T, v3 o, v3 d, float mint, float maxt, bool found, float ht, float &bt,
                                                      uint32_t &n_tests, uint32_t &n_nodes) {
    int best = -1; bt = 0.0f;
    const SlabRay s = slab_ray(d);
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float rr = ao * RTW_TRI_RAY_PAD;
    float lim = found ? ht : maxt;
    uint32_t ni = 0;
    while (ni < T.n_nodes) {
        const f4 *q = (const f4 *)(T.nodes + ni);
        const f4 a = q[0], b = q[1];
        n_nodes++;
        const uint32_t skip = mesh_bits(a.w), leaf = mesh_bits(b.w);
        if (!slab_hit(s, a, b, o, rr, mint, lim)) { ni = skip; continue; }
        if (leaf == 0u) { ni++; continue; }
        const uint32_t first = leaf >> 3, cnt = leaf & 7u;
        for (uint32_t j = 0; j < cnt; ++j) {
            const DevTri r = mesh_tri_load(T.leaf, first + j);
            const int idx = (int)r.index;
            float t;
            auto could_win = [&](float x) { return best < 0 ? (!found || x < ht) : (x < bt || (x == bt && idx < best)); };
            if (tri_test(r, o.x, o.y, o.z, d.x, d.y, d.z, mint, maxt, could_win, t)) { best = idx; bt = t; lim = t; }
        }
        n_tests += cnt;
        ni = skip;
    }
    return best;
}

// The triangle list for one ray (tri_closest's list half): the group's closest in list order, kept only when it replaces the result so far
__host__ __device__ __forceinline__ int tri_list_walk(const DevTris &T, v3 o, v3 d, float mint, float maxt, bool found, float ht, float &bt, uint32_t &n_tests) {
    int best = -1; bt = 0.0f;
    for (uint32_t k = 0; k < T.n; ++k) {
        const DevTri r = mesh_tri_load_uniform(T.list, k);
        float t;
        if (tri_test(r, o.x, o.y, o.z, d.x, d.y, d.z, mint, maxt, [&](float x) { return best < 0 || bt > x; }, t)) { best = (int)k; bt = t; }
    }
    n_tests += T.n;
    if (best >= 0 && found && !(ht > bt)) best = -1;
    return best;
}

// One placement for one ray: the ray in the placement's frame -- o' = q.rotate(o - position), d' = q.rotate(d) -- asks the mesh, through the
// tree where the LOCAL ray passes tri_ray_ordinary, else through the list (the same answer).  `found` / `ht`: only a hit with t < ht is taken.
__host__ __device__ __forceinline__ int mesh_placement(const DevTris &T, quat qn, v3 pos, v3 o, v3 d, float mint, float maxt, bool found, float ht,
                                                       float &t, uint32_t &n_tests, uint32_t &n_nodes) {
    const v3 po = mesh_rot(qn, o - pos), pd = mesh_rot(qn, d);
    if (T.nodes != nullptr && tri_ray_ordinary(T, po, pd)) return tri_tree_walk(T, po, pd, mint, maxt, found, ht, t, n_tests, n_nodes);
    return tri_list_walk(T, po, pd, mint, maxt, found, ht, t, n_tests);
}

// Can the top-level tree answer this ray?  Finite, with a direction (d = 0 meets no triangle and has no slab to test), and within a reach that
// implies tri_ray_ordinary in every placement's frame (above)
__host__ __device__ __forceinline__ bool mesh_top_ray_ordinary(const DevTris &T, v3 o, v3 d) {
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float ad = fmaxf(fmaxf(__builtin_fabsf(d.x), __builtin_fabsf(d.y)), __builtin_fabsf(d.z));
    const bool finite = (o.x - o.x == 0.0f) && (o.y - o.y == 0.0f) && (o.z - o.z == 0.0f) && (d.x - d.x == 0.0f) && (d.y - d.y == 0.0f) && (d.z - d.z == 0.0f);
    return finite && ad > 0.0f && ao + ad * T.t_bound <= RTW_MESH_TOP_REACH;
}

// The placement group through the top-level tree over the placements' world boxes (mesh_top_build, rtw_tri.cpp): a per-lane
// stackless walk in the TriNode format, the nodes read by vector loads, `leaf` naming a run of `order` -- the placement indices in leaf
// order, stored behind the nodes.  The list-order rule -- the closest placement, of equal t the LOWEST index, against the result so far
// only when strictly closer -- has to be explicit here, since the tree meets placements in its own order: a candidate (t, k) replaces the
// best placement (bt, kb) iff t < bt || (t == bt && k < kb), and the first one iff t < ht.  tri_tree_walk / tri_list_walk accept only
// t < bound, so the equality for k < kb reaches them as bound = the next float above bt: t < next_up(bt) is t <= bt.  (Which triangle of a
// placement wins does not depend on the bound: it is the placement's least (t, index) whenever that t passes.)  lim = bt is inclusive in the
// slab test, so a box that holds an equal t is not pruned.
__host__ __device__ __forceinline__ int mesh_top_walk(const DevTris &T, const f4 *rows, const TriNode *top, uint32_t n_top, v3 o, v3 d, float mint,
                                                      float maxt, bool found, float ht, int &tri, float &bt, uint32_t &n_tests, uint32_t &n_nodes) {
    int best = -1; tri = -1; bt = 0.0f;
    const uint32_t *order = (const uint32_t *)(top + n_top);
    const SlabRay s = slab_ray(d);
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float rr = ao * RTW_MESH_TOP_RAY_PAD;
    float lim = found ? ht : maxt;
    uint32_t ni = 0;
    while (ni < n_top) {
        const f4 *q = (const f4 *)(top + ni);
        const f4 a = q[0], b = q[1];
        n_nodes++;
        const uint32_t skip = mesh_bits(a.w), leaf = mesh_bits(b.w);
        if (!slab_hit(s, a, b, o, rr, mint, lim)) { ni = skip; continue; }
        if (leaf == 0u) { ni++; continue; }
        const uint32_t first = leaf >> 3, cnt = leaf & 7u;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t k = order[first + j];
            quat qn; v3 pos;
            mesh_row_lane(rows, k, qn, pos);
            const bool have = best >= 0;
            const float bound = have ? ((int)k < best ? mesh_next_up(bt) : bt) : ht;
            float t;
            const int jt = mesh_placement(T, qn, pos, o, d, mint, maxt, found || have, bound, t, n_tests, n_nodes);
            if (jt >= 0) { best = (int)k; tri = jt; bt = t; lim = t; }
        }
        ni = skip;
    }
    return best;
}

// The placement group.  Returns the winning placement or -1; tri = its triangle (caller's list), bt = its t; `found` / `ht`: the result so
// far (the other groups): the group replaces it only when strictly closer.  (The winner's frame is formed again by the caller, mesh_row_lane
// + mesh_rot: the same operations, the same bits, and thirteen registers not carried round the loop.)
// top != null (wave-uniform; rtw_shim.hip: more than RTW_OPT_MESH_LIST_MAX placements under RTW_ACCEL_BVH, the mesh's tree and the top-level
// tree both usable): a ray mesh_top_ray_ordinary accepts walks the top-level tree.  Every other ray, and every ray of every other context,
// meets the placements in list order: placement k wave-uniform, its rows by scalar loads, each placement's result the bound of the next.
// There the root's slab test in the local frame is the only cull.  The two give the same bits.
__host__ __device__ __forceinline__ int mesh_closest(const DevTris &T, const f4 *rows, uint32_t n, const TriNode *top, uint32_t n_top, v3 o, v3 d,
                                                     float mint, float maxt, bool found, float ht, int &tri, float &bt, uint32_t &n_tests, uint32_t &n_nodes) {
    if (top != nullptr && mesh_top_ray_ordinary(T, o, d)) return mesh_top_walk(T, rows, top, n_top, o, d, mint, maxt, found, ht, tri, bt, n_tests, n_nodes);
    int best = -1; tri = -1; bt = 0.0f;
    for (uint32_t k = 0; k < n; ++k) {
        quat qn; v3 pos;
        mesh_row(rows, k, qn, pos);
        float t;
        const int j = mesh_placement(T, qn, pos, o, d, mint, maxt, found, ht, t, n_tests, n_nodes);
        if (j >= 0) { best = (int)k; tri = j; bt = t; found = true; ht = t; }
    }
    return best;
}
} // namespace rtw
