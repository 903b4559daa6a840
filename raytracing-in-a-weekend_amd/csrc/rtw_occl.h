// rtw_occl.h -- any-hit ("is anything in the way?") twins of the TriNode walks of rtw_mesh.h, for rtw_ctx_scene_occluded (rtw_occluded.hip)
// and its host forms rtw_triangle_occluded / rtw_mesh_instance_occluded (rtw_tri.cpp): DESIGN.md 4.14.  ONE __host__ __device__ definition
// each, so the host runs what the kernel runs.  No render kernel and no closest-hit query reads this file.
//
// Each walk is the closest-hit walk of the same name in rtw_mesh.h with nothing found so far (found = false, lim = maxt), stopped at its
// first accepted candidate: the same boxes, paddings, skip links, candidate order and tests (slab_ray, slab_hit, tri_test, mesh_row,
// mesh_row_lane, mesh_rot as they are), the predicate between the plane and the interior test accepting every in-range t -- what could_win
// answers while best < 0 and found is false.  Until that candidate the two walks are in the same state, so an any-hit walk is a PREFIX of the
// closest-hit walk: it returns true exactly when the other returns an index >= 0, and counts no more than it.  Change them together.
#pragma once
#include "rtw_mesh.h"

namespace rtw {

// Is no lane of the wave still open?  (the host has one lane)
__host__ __device__ __forceinline__ bool occl_none_open(bool open) {
#ifdef __HIP_DEVICE_COMPILE__
    return ballot64(open) == 0ull;
#else
    return !open;
#endif
}

__host__ __device__ __forceinline__ bool occl_tri(const DevTri &r, v3 o, v3 d, float mint, float maxt) {
    float t;
    return tri_test(r, o.x, o.y, o.z, d.x, d.y, d.z, mint, maxt, [](float) { return true; }, t);
}

// tri_tree_walk's twin: the lane ends at its first accepted triangle (ni = n_nodes)
__host__ __device__ __forceinline__ bool tri_tree_any(const DevTris &T, v3 o, v3 d, float mint, float maxt, uint32_t &n_tests, uint32_t &n_nodes) {
    const SlabRay s = slab_ray(d);
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float rr = ao * RTW_TRI_RAY_PAD;
    bool hit = false;
    uint32_t ni = 0;
    while (ni < T.n_nodes) {
        const f4 *q = (const f4 *)(T.nodes + ni);
        const f4 a = q[0], b = q[1];
        n_nodes++;
        const uint32_t skip = mesh_bits(a.w), leaf = mesh_bits(b.w);
        if (!slab_hit(s, a, b, o, rr, mint, maxt)) { ni = skip; continue; }
        if (leaf == 0u) { ni++; continue; }
        const uint32_t first = leaf >> 3, cnt = leaf & 7u;
        ni = skip;
        for (uint32_t j = 0; j < cnt; ++j) {
            n_tests++;
            if (occl_tri(mesh_tri_load(T.leaf, first + j), o, d, mint, maxt)) { hit = true; ni = T.n_nodes; break; }
        }
    }
    return hit;
}

// tri_list_walk's twin.  k is wave-uniform (scalar loads), so every lane of the wave enters, `open` or not: a lane that is not open tests and
// counts nothing, and the loop ends when no lane is open.  Returns true when the lane was open and a triangle accepted its ray.
__host__ __device__ __forceinline__ bool tri_list_any(const DevTris &T, v3 o, v3 d, float mint, float maxt, bool open, uint32_t &n_tests) {
    bool hit = false;
    for (uint32_t k = 0; k < T.n; ++k) {
        if (occl_none_open(open)) break;
        const DevTri r = mesh_tri_load_uniform(T.list, k);
        if (open) {
            n_tests++;
            if (occl_tri(r, o, d, mint, maxt)) { hit = true; open = false; }
        }
    }
    return hit;
}

// mesh_placement's twin: the tree where the LOCAL ray passes tri_ray_ordinary, else the list.  Per lane (the top-level tree's leaves) ...
__host__ __device__ __forceinline__ bool mesh_placement_any(const DevTris &T, quat qn, v3 pos, v3 o, v3 d, float mint, float maxt, uint32_t &n_tests,
                                                            uint32_t &n_nodes) {
    const v3 po = mesh_rot(qn, o - pos), pd = mesh_rot(qn, d);
    if (T.nodes != nullptr && tri_ray_ordinary(T, po, pd)) return tri_tree_any(T, po, pd, mint, maxt, n_tests, n_nodes);
    return tri_list_any(T, po, pd, mint, maxt, true, n_tests);
}

// mesh_top_walk's twin: the lane ends at the first placement that accepts its ray (ni = n_top).  Only for rays mesh_top_ray_ordinary accepts.
__host__ __device__ __forceinline__ bool mesh_top_any(const DevTris &T, const f4 *rows, const TriNode *top, uint32_t n_top, v3 o, v3 d, float mint,
                                                      float maxt, uint32_t &n_tests, uint32_t &n_nodes) {
    const uint32_t *order = (const uint32_t *)(top + n_top);
    const SlabRay s = slab_ray(d);
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float rr = ao * RTW_MESH_TOP_RAY_PAD;
    bool hit = false;
    uint32_t ni = 0;
    while (ni < n_top) {
        const f4 *q = (const f4 *)(top + ni);
        const f4 a = q[0], b = q[1];
        n_nodes++;
        const uint32_t skip = mesh_bits(a.w), leaf = mesh_bits(b.w);
        if (!slab_hit(s, a, b, o, rr, mint, maxt)) { ni = skip; continue; }
        if (leaf == 0u) { ni++; continue; }
        const uint32_t first = leaf >> 3, cnt = leaf & 7u;
        ni = skip;
        for (uint32_t j = 0; j < cnt; ++j) {
            quat qn; v3 pos;
            mesh_row_lane(rows, order[first + j], qn, pos);
            if (mesh_placement_any(T, qn, pos, o, d, mint, maxt, n_tests, n_nodes)) { hit = true; ni = n_top; break; }
        }
    }
    return hit;
}

// mesh_closest's twin, the placement group: a ray mesh_top_ray_ordinary accepts walks the top-level tree when there is one (top != null,
// wave-uniform); every other ray meets the placements in list order, k wave-uniform, its rows by scalar loads, until no lane is open.
// Every lane of the wave enters; returns true when the lane was open and a placement accepted its ray.
__host__ __device__ __forceinline__ bool mesh_any(const DevTris &T, const f4 *rows, uint32_t n, const TriNode *top, uint32_t n_top, v3 o, v3 d,
                                                  float mint, float maxt, bool open, uint32_t &n_tests, uint32_t &n_nodes) {
    if (top != nullptr && mesh_top_ray_ordinary(T, o, d)) return open && mesh_top_any(T, rows, top, n_top, o, d, mint, maxt, n_tests, n_nodes);
    bool hit = false;
    for (uint32_t k = 0; k < n; ++k) {
        if (occl_none_open(open)) break;
        quat qn; v3 pos;
        mesh_row(rows, k, qn, pos);
        if (open) {                                                // (the local ray decides tree or list per lane, as mesh_placement)
            const v3 po = mesh_rot(qn, o - pos), pd = mesh_rot(qn, d);
            const bool tree = T.nodes != nullptr && tri_ray_ordinary(T, po, pd);
            if (tree ? tri_tree_any(T, po, pd, mint, maxt, n_tests, n_nodes) : tri_list_any(T, po, pd, mint, maxt, true, n_tests)) { hit = true; open = false; }
        }
    }
    return hit;
}

// The triangle group of a scene without placements: the tree for the rays tri_ray_ordinary accepts, the list for the others
__host__ __device__ __forceinline__ bool tri_any(const DevTris &T, v3 o, v3 d, float mint, float maxt, bool open, uint32_t &n_tests, uint32_t &n_nodes) {
    if (T.nodes != nullptr && tri_ray_ordinary(T, o, d)) return open && tri_tree_any(T, o, d, mint, maxt, n_tests, n_nodes);
    return tri_list_any(T, o, d, mint, maxt, open, n_tests);
}

} // namespace rtw
