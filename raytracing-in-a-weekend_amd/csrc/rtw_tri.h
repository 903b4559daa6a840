// rtw_tri.h -- Rust2 triangles (Rust2/src/objects/triangle.rs): the hit test shared by host and device, the device records, the list walk and
// the traversal of the triangle tree (DESIGN.md "Rust2 triangles").  Only the triangle build of the render kernels (SPEC 8) and the query
// kernel of rtw_ctx_triangle_hits compile any of the device code.
#pragma once
#include "rtw_device.h"
#include <vector>

namespace rtw {

// A triangle as the device reads it: Triangle::new's fields (:28-50) and the inline material, seven 16-byte rows.
struct DevTri {
    float origin[3]; float d;             // d = normal . origin
    float u[3];      uint32_t index;      // position in the caller's list (ties, records)
    float v[3];      float metallicness;
    float normal[3]; float opacity;       // unit(u x v), never flipped
    float w[3];      float ir;            // n / (n . n)
    float albedo[3]; int32_t tex;         // tex < 0: the constant colour (tex_color * 1.0)
    float emitted[3]; uint32_t pad;
};
static_assert(sizeof(DevTri) == 112, "DevTri is seven f4 rows");

// A node of the triangle tree, depth-first order: the left child of an inner node follows it; `skip` is the node after its subtree (n_nodes:
// the end).  leaf = (first << 3) | count, count 1..4 triangles of DevTris.leaf; 0 for an inner node.  Boxes are already inflated by the
// triangles' static error radius (rtw_tri.cpp); the traversal adds the per-ray part.
struct TriNode {
    float lo[3]; uint32_t skip;
    float hi[3]; uint32_t leaf;
};
static_assert(sizeof(TriNode) == 32, "TriNode is two f4 rows");

struct DevTris {
    const DevTri *list;                   // the caller's order (the list walk, records)
    const DevTri *leaf;                   // leaf order of the tree
    const TriNode *nodes;                 // null: walk the list
    uint32_t n, n_nodes;
    float t_bound;                        // max(|mint|, |maxt|) of the render: per-ray check |o| + |d| t_bound <= 2^40
    uint32_t lds_off;                     // render kernels: byte offset of the workgroup's node-visit counter in the dynamic LDS (rtw_shim.hip)
};

#define RTW_TRI_COORD_MAX 0x1p40f         // every bound of the cull's derivation (coordinates, |w|, the reach of a ray)
#define RTW_TRI_RAY_PAD 0x1p-17f          // per-ray inflation: 128 u max|o_i| (u = 2^-24)
#define RTW_TRI_T_PAD 0x1p-20f            // the slab interval is widened by this fraction of |t| at each end (>= 2 gamma_3, PBRT 3.9.2)

// get_hit (triangle.rs:95-112): the plane part.  Operation order as written; -ffp-contract=off on host and device.
__host__ __device__ __forceinline__ bool tri_plane(float nx, float ny, float nz, float dd, float ox, float oy, float oz, float dx, float dy, float dz,
                                                   float mint, float maxt, float &t) {
    const float denominator = nx * dx + ny * dy + nz * dz;
    if (__builtin_fabsf(denominator) <= 1e-8f) return false;
    t = (dd - (nx * ox + ny * oy + nz * oz)) / denominator;
    if (t < mint || t > maxt) return false;
    return true;
}
// ... the interior part (:113-124): point = r.at(t), planar = point - origin, alfa = w . (planar x v), beta = w . (u x planar)
__host__ __device__ __forceinline__ bool tri_inside(const float *org, const float *u, const float *v, const float *w,
                                                    float ox, float oy, float oz, float dx, float dy, float dz, float t, float &alfa, float &beta) {
    const float px = ox + dx * t, py = oy + dy * t, pz = oz + dz * t;
    const float qx = px - org[0], qy = py - org[1], qz = pz - org[2];
    const float cx = qy * v[2] - qz * v[1], cy = qz * v[0] - qx * v[2], cz = qx * v[1] - qy * v[0];
    const float ex = u[1] * qz - u[2] * qy, ey = u[2] * qx - u[0] * qz, ez = u[0] * qy - u[1] * qx;
    alfa = w[0] * cx + w[1] * cy + w[2] * cz;
    beta = w[0] * ex + w[1] * ey + w[2] * ez;
    return !(alfa < 0.0f || beta < 0.0f || alfa + beta > 1.0f);
}
// Triangle::new (:35-49): n = u x v, normal = unit(n) = n / |n|, d = normal . origin, w = n / (n . n)
__host__ __device__ __forceinline__ void tri_derive(const float *org, const float *u, const float *v, float *normal, float &d, float *w) {
    const float nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
    const float len = __builtin_sqrtf(nx * nx + ny * ny + nz * nz);
    normal[0] = nx / len; normal[1] = ny / len; normal[2] = nz / len;
    d = normal[0] * org[0] + normal[1] * org[1] + normal[2] * org[2];
    const float nn = nx * nx + ny * ny + nz * nz;
    w[0] = nx / nn; w[1] = ny / nn; w[2] = nz / nn;
}

// The whole test of DevTri `r` (plane, then interior) -- the list walk's, the tree's, the host's.  `could_win(t)` is asked between the two
// parts: false skips the interior test (a pure shortcut, the result is the same).
template <class F>
__host__ __device__ __forceinline__ bool tri_test(const DevTri &r, float ox, float oy, float oz, float dx, float dy, float dz, float mint, float maxt,
                                                  F could_win, float &t) {
    if (!tri_plane(r.normal[0], r.normal[1], r.normal[2], r.d, ox, oy, oz, dx, dy, dz, mint, maxt, t)) return false;
    if (!could_win(t)) return false;
    float alfa, beta;
    return tri_inside(r.origin, r.u, r.v, r.w, ox, oy, oz, dx, dy, dz, t, alfa, beta);
}

// The triangle group on the host: closest in list order, a later one only when strictly closer (rtw_triangle_hits)
inline int tri_closest_host(const DevTri *list, uint32_t n, float ox, float oy, float oz, float dx, float dy, float dz, float mint, float maxt, float &bt) {
    int best = -1; bt = 0.0f;
    for (uint32_t k = 0; k < n; k++) {
        float t;
        if (tri_test(list[k], ox, oy, oz, dx, dy, dz, mint, maxt, [&](float x) { return best < 0 || bt > x; }, t)) { best = (int)k; bt = t; }
    }
    return best;
}

// The device row loads of a DevTri: scalar (wave-uniform index, the list walk) or vector (per-lane index, leaves and records)
__device__ __forceinline__ DevTri tri_load_uniform(const DevTri *base, uint32_t k) {
    cf4_ptr q = (cf4_ptr)(uintptr_t)(base + k);
    DevTri r;
    const f4 r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
    r.origin[0] = r0.x; r.origin[1] = r0.y; r.origin[2] = r0.z; r.d = r0.w;
    r.u[0] = r1.x; r.u[1] = r1.y; r.u[2] = r1.z;
    r.v[0] = r2.x; r.v[1] = r2.y; r.v[2] = r2.z;
    r.normal[0] = r3.x; r.normal[1] = r3.y; r.normal[2] = r3.z;
    r.w[0] = r4.x; r.w[1] = r4.y; r.w[2] = r4.z;
    return r;
}
__device__ __forceinline__ DevTri tri_load(const DevTri *base, uint32_t k) {
    const f4 *q = (const f4 *)(base + k);
    DevTri r;
    const f4 r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
    r.origin[0] = r0.x; r.origin[1] = r0.y; r.origin[2] = r0.z; r.d = r0.w;
    r.u[0] = r1.x; r.u[1] = r1.y; r.u[2] = r1.z; r.index = __float_as_uint(r1.w);
    r.v[0] = r2.x; r.v[1] = r2.y; r.v[2] = r2.z;
    r.normal[0] = r3.x; r.normal[1] = r3.y; r.normal[2] = r3.z;
    r.w[0] = r4.x; r.w[1] = r4.y; r.w[2] = r4.z;
    return r;
}

// Can the tree answer this ray?  (DESIGN.md "Rust2 triangles": the derivation needs |o| + |d| max(|mint|, |maxt|) <= 2^40; NaN fails it)
__host__ __device__ __forceinline__ bool tri_ray_ordinary(const DevTris &T, v3 o, v3 d) {
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float ad = fmaxf(fmaxf(__builtin_fabsf(d.x), __builtin_fabsf(d.y)), __builtin_fabsf(d.z));
    const bool finite = (o.x - o.x == 0.0f) && (o.y - o.y == 0.0f) && (o.z - o.z == 0.0f) && (d.x - d.x == 0.0f) && (d.y - d.y == 0.0f) && (d.z - d.z == 0.0f);
    return finite && ao + ad * T.t_bound <= RTW_TRI_COORD_MAX;
}

// (The tree half below has a TWIN, tri_tree_walk in rtw_mesh.h: the same boxes, paddings, skip links and tie rule, plus an exact slab for a
//  direction component that is exactly zero -- here such a ray prunes nothing, DESIGN.md 4.8.  Change the two together.)
// The closest triangle (group rule, rtw.h): returns its index in the caller's list, or -1; bt = its t.  `found` / `ht`: the result so far.
// With the tree the group winner is taken only when it would replace (ht > t), which is all the caller uses of it: the list walk's
// group minimum then replaces exactly when the tree's answer exists (t is finite on the tree's rays: the list walk answers all others).
__device__ __forceinline__ int tri_closest(const DevTris &T, v3 o, v3 d, float mint, float maxt, bool found, float ht, float &bt,
                                           uint32_t &n_tests, uint32_t &n_nodes) {
    int best = -1; bt = 0.0f;
    if (T.nodes == nullptr || !tri_ray_ordinary(T, o, d)) {
        for (uint32_t k = 0; k < T.n; ++k) {                  // the list walk (the reference's order)
            const DevTri r = tri_load_uniform(T.list, k);
            float t;
            if (tri_test(r, o.x, o.y, o.z, d.x, d.y, d.z, mint, maxt, [&](float x) { return best < 0 || bt > x; }, t)) { best = (int)k; bt = t; }
        }
        n_tests += T.n;
        if (best >= 0 && found && !(ht > bt)) best = -1;      // (the caller's comparison, done here for both forms)
        return best;
    }
    // the tree: ties to the lower list index; only candidates that replace the result so far (t < ht) are taken
    const float ix = 1.0f / d.x, iy = 1.0f / d.y, iz = 1.0f / d.z;
    const float ao = fmaxf(fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    const float rr = ao * RTW_TRI_RAY_PAD;
    float lim = found ? ht : maxt;
    uint32_t ni = 0;
    while (ni < T.n_nodes) {
        const f4 *q = (const f4 *)(T.nodes + ni);
        const f4 a = q[0], b = q[1];
        n_nodes++;
        float t0 = ((a.x - rr) - o.x) * ix, t1 = ((b.x + rr) - o.x) * ix;
        float ne = fminf(t0, t1), fa = fmaxf(t0, t1);
        t0 = ((a.y - rr) - o.y) * iy; t1 = ((b.y + rr) - o.y) * iy;
        ne = fmaxf(ne, fminf(t0, t1)); fa = fminf(fa, fmaxf(t0, t1));
        t0 = ((a.z - rr) - o.z) * iz; t1 = ((b.z + rr) - o.z) * iz;
        ne = fmaxf(ne, fminf(t0, t1)); fa = fminf(fa, fmaxf(t0, t1));
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

// The workgroup's count of triangle-tree node visits (render kernels of the triangle build): a u32 in the dynamic LDS, zeroed at the kernel's
// start and added to stats[3] at its end.  (A per-lane counter in the kernels' own locals perturbed the code of every existing kernel.)
__device__ __forceinline__ uint32_t *tri_node_counter(const DevTris &T) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tri_lds[];
    return (uint32_t *)(tri_lds + T.lds_off);
}

// The `Hit` of triangle `k` (caller's list) at parameter t: get_hit's record (:118-123) and Triangle::color (:130-136).
__device__ __forceinline__ void tri_record(const DevScene &sc, const DevTris &T, uint32_t k, v3 o, v3 d, float t, bool rust2, GeomHit &h) {
    const DevTri &q = T.list[k];
    const v3 point = o + d * t;
    v3 cm = ld3(q.albedo), emitted = ld3(q.emitted);
    const int32_t tex = q.tex;
    if (tex >= 0) {
        const v3 planar = point - ld3(q.origin);
        const v3 qu = ld3(q.u), qv = ld3(q.v), w = ld3(q.w);
        const v3 pxv = mk(planar.y * qv.z - planar.z * qv.y, planar.z * qv.x - planar.x * qv.z, planar.x * qv.y - planar.y * qv.x);
        const v3 uxp = mk(qu.y * planar.z - qu.z * planar.y, qu.z * planar.x - qu.x * planar.z, qu.x * planar.y - qu.y * planar.x);
        const float alfa = dot(w, pxv), beta = dot(w, uxp);
        const RtwTexture tx = sc.tex[tex];
        if (rust2) {                                           // ImageTexture::color_at(alfa, beta) (Rust2/src/objects/texture.rs:94-105)
            cm = ld3(sc.texels + 3 * (size_t)(tx.texel_offset + rust2_texel_index(alfa, beta, tx.row, tx.col, false)));
            if (tx.emit_tex != 0u) {
                const RtwTexture e = sc.tex[tx.emit_tex - 1u];
                emitted = ld3(sc.texels + 3 * (size_t)(e.texel_offset + rust2_texel_index(alfa, beta, e.row, e.col, true)));
            }
        } else {                                               // the quad's texel rule (quad.rs:64-79)
            const uint32_t ix = alfa != 1.0f ? tex_index(floorf(alfa * (float)tx.row), tx.row - 1) : tx.row - 1;
            const uint32_t iy = beta != 1.0f ? tex_index(floorf(beta * (float)tx.col), tx.col - 1) : tx.col - 1;
            cm = ld3(sc.texels + 3 * (size_t)(tx.texel_offset + iy * tx.row + ix)) * 1.0f;
        }
    }
    h.t = t; h.point = point; h.normal = ld3(q.normal); h.cm = cm;
    h.m = mat_params(q.metallicness, q.opacity, q.ir);
    h.emitted = emitted;
}

// ---- host (rtw_tri.cpp) ----------------------------------------------------------------------------------------------------------------
// The device records of a triangle list, derived fields recomputed (Triangle::new), index = list position.
void tri_prepare(const RtwTriangle *t, uint32_t n, DevTri *list);
// The tree over `list`: nodes (depth-first, skip links), the triangles in leaf order; list_walk = a condition of DESIGN.md "Rust2
// triangles" holds, the tree must not be used (it is built anyway).  Returns false when memory runs out.
struct TriBuild {
    TriNode *nodes = nullptr; uint32_t n_nodes = 0;
    DevTri *leaf = nullptr;
    uint32_t depth = 0;
    bool list_walk = false;
    ~TriBuild();
};
bool tri_build(const DevTri *list, uint32_t n, TriBuild &out);
// The top-level tree over n placements of a mesh whose tree's root is `root` (rows: mesh_rows' output): DESIGN.md 4.11.  nodes in the TriNode
// format, leaf = (first << 3) | count names a run of `order`, the placement indices in leaf order; `packed` is what the device reads: the
// nodes, then the order array behind them.  list_walk: a placement lies beyond the reach of the bound (the tree is built anyway).
struct MeshTopBuild {
    std::vector<TriNode> nodes;
    std::vector<uint32_t> order;
    uint32_t depth = 0;
    bool list_walk = false;
    std::vector<unsigned char> packed() const;
};
bool mesh_top_build(const TriNode &root, const f4 *rows, uint32_t n, MeshTopBuild &out);

} // namespace rtw
