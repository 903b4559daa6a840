// rtw_mesh.h -- mesh placements: Rust2's `Instance` of triangles (Rust2/src/objects/instance.rs:215-255 around triangle.rs).  The context's
// triangle mesh is placed n times, each placement a position and a quaternion, all sharing the mesh's one tree (rtw.h "mesh
// placements").  Compiled by the placement build of the render kernels (SPEC 12), by the query kernel (rtw_query.hip) and by the kernel of
// rtw_ctx_mesh_instance_hits; the host pieces by rtw_tri.cpp.  No other kernel reads this file.
#pragma once
#include "rtw_tri.h"
#include "rtw_quat.h"

namespace rtw {

// A placement as the device reads it: two f4 rows {qn.w, qn.x, qn.y, qn.z}, {position, 0}; qn = quat_normalised(q), formed on the host.

// ---- host and device: the rows of a placement list, and one placement's list walk ------------------------------------------------------
// The checks of rtw_ctx_set_mesh_instances on the placements themselves; rows ([2 n] f4, may be null) receives what the kernels read.
inline bool mesh_rows(const RtwMeshInstance *p, uint32_t n, f4 *rows) {
    for (uint32_t i = 0; i < n; i++) {
        const quat q = qmk(p[i].quat[0], p[i].quat[1], p[i].quat[2], p[i].quat[3]);
        for (int k = 0; k < 3; k++) if (!(p[i].position[k] - p[i].position[k] == 0.0f)) return false;
        if (!(q.w - q.w == 0.0f) || !(q.x - q.x == 0.0f) || !(q.y - q.y == 0.0f) || !(q.z - q.z == 0.0f)) return false;
        const float l = quat_len(q);
        if (!(l > 0.0f) || !(l - l == 0.0f)) return false;
        if (rows) {
            const quat qn = quat_normalised(q);
            f4 a, b;
            a.x = qn.w; a.y = qn.x; a.z = qn.y; a.w = qn.z;
            b.x = p[i].position[0]; b.y = p[i].position[1]; b.z = p[i].position[2]; b.w = 0.0f;
            rows[2 * (size_t)i] = a; rows[2 * (size_t)i + 1] = b;
        }
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

// ---- device ----------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ v3 mesh_rot(quat qn, v3 a) {
    v3 o;
    quat_rotate_n(qn, a.x, a.y, a.z, o.x, o.y, o.z);
    return o;
}
// Rows of placement k for a wave-uniform k (the placement loop): scalar loads through the constant address space
__device__ __forceinline__ void mesh_row(const f4 *rows, uint32_t k, quat &qn, v3 &pos) {
    cf4_ptr q = (cf4_ptr)(uintptr_t)(rows + 2 * (size_t)k);
    const f4 a = q[0], b = q[1];
    qn = qmk(a.x, a.y, a.z, a.w); pos = mk(b.x, b.y, b.z);
}
// ... and for a per-lane k (the record of the placement a lane's ray hit)
__device__ __forceinline__ void mesh_row_lane(const f4 *rows, uint32_t k, quat &qn, v3 &pos) {
    const f4 *q = rows + 2 * (size_t)k;
    const f4 a = q[0], b = q[1];
    qn = qmk(a.x, a.y, a.z, a.w); pos = mk(b.x, b.y, b.z);
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
__device__ __forceinline__ int tri_tree_walk(const DevTris &T, v3 o, v3 d, float mint, float maxt, bool found, float ht, float &bt,
                                             uint32_t &n_tests, uint32_t &n_nodes) {
    int best = -1; bt = 0.0f;
    const float ix = 1.0f / d.x, iy = 1.0f / d.y, iz = 1.0f / d.z;
    const bool zx = d.x == 0.0f, zy = d.y == 0.0f, zz = d.z == 0.0f;
    const bool any_zero = ballot64(zx || zy || zz) != 0ull;             // wave-uniform: the selects below run only in waves that hold such a ray
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float rr = ao * RTW_TRI_RAY_PAD;
    const float BIG = 0x1.fffffep127f;
    float lim = found ? ht : maxt;
    uint32_t ni = 0;
    while (ni < T.n_nodes) {
        const f4 *q = (const f4 *)(T.nodes + ni);
        const f4 a = q[0], b = q[1];
        n_nodes++;
        float x0 = ((a.x - rr) - o.x) * ix, x1 = ((b.x + rr) - o.x) * ix;
        float y0 = ((a.y - rr) - o.y) * iy, y1 = ((b.y + rr) - o.y) * iy;
        float z0 = ((a.z - rr) - o.z) * iz, z1 = ((b.z + rr) - o.z) * iz;
        if (any_zero) {
            if (zx) { const bool in = (a.x - rr) <= o.x && o.x <= (b.x + rr); x0 = in ? -BIG : BIG; x1 = BIG; }
            if (zy) { const bool in = (a.y - rr) <= o.y && o.y <= (b.y + rr); y0 = in ? -BIG : BIG; y1 = BIG; }
            if (zz) { const bool in = (a.z - rr) <= o.z && o.z <= (b.z + rr); z0 = in ? -BIG : BIG; z1 = BIG; }
        }
        float ne = fminf(x0, x1), fa = fmaxf(x0, x1);
        ne = fmaxf(ne, fminf(y0, y1)); fa = fminf(fa, fmaxf(y0, y1));
        ne = fmaxf(ne, fminf(z0, z1)); fa = fminf(fa, fmaxf(z0, z1));
        ne = ne - __builtin_fabsf(ne) * RTW_TRI_T_PAD;
        fa = fa + __builtin_fabsf(fa) * RTW_TRI_T_PAD;
        const uint32_t skip = __float_as_uint(a.w), leaf = __float_as_uint(b.w);
        if (!(fmaxf(ne, mint) <= fminf(fa, lim))) { ni = skip; continue; }
        if (leaf == 0u) { ni++; continue; }
        const uint32_t first = leaf >> 3, cnt = leaf & 7u;
        for (uint32_t j = 0; j < cnt; ++j) {
            const DevTri r = tri_load(T.leaf, first + j);
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
__device__ __forceinline__ int tri_list_walk(const DevTris &T, v3 o, v3 d, float mint, float maxt, bool found, float ht, float &bt, uint32_t &n_tests) {
    int best = -1; bt = 0.0f;
    for (uint32_t k = 0; k < T.n; ++k) {
        const DevTri r = tri_load_uniform(T.list, k);
        float t;
        if (tri_test(r, o.x, o.y, o.z, d.x, d.y, d.z, mint, maxt, [&](float x) { return best < 0 || bt > x; }, t)) { best = (int)k; bt = t; }
    }
    n_tests += T.n;
    if (best >= 0 && found && !(ht > bt)) best = -1;
    return best;
}

// The placement group: placement k (wave-uniform, rows by scalar loads) takes the ray into its frame -- o' = q.rotate(o - position), d' =
// q.rotate(d) -- and asks the mesh there, through the tree where the LOCAL ray passes tri_ray_ordinary, else through the list (the same
// answer).  `found` / `ht`: the result so far (the other groups, then the earlier placements): a placement is taken only when it replaces it,
// i.e. when strictly closer.  Returns the winning placement or -1; tri = its triangle (caller's list), bt = its t.  (The winner's frame is
// formed again by the caller, mesh_row_lane + mesh_rot: the same operations, the same bits, and thirteen registers not carried round the loop.)
// There is no world-space cull: the root's slab test in the local frame is the cull.
__device__ __forceinline__ int mesh_closest(const DevTris &T, const f4 *rows, uint32_t n, v3 o, v3 d, float mint, float maxt, bool found, float ht,
                                            int &tri, float &bt, uint32_t &n_tests, uint32_t &n_nodes) {
    int best = -1; tri = -1; bt = 0.0f;
    for (uint32_t k = 0; k < n; ++k) {
        quat qn; v3 pos;
        mesh_row(rows, k, qn, pos);
        const v3 po = mesh_rot(qn, o - pos), pd = mesh_rot(qn, d);
        float t;
        int j;
        if (T.nodes != nullptr && tri_ray_ordinary(T, po, pd)) j = tri_tree_walk(T, po, pd, mint, maxt, found, ht, t, n_tests, n_nodes);
        else j = tri_list_walk(T, po, pd, mint, maxt, found, ht, t, n_tests);
        if (j >= 0) { best = (int)k; tri = j; bt = t; found = true; ht = t; }
    }
    return best;
}
} // namespace rtw
