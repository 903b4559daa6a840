// rtw_refit.h -- what the triangle tree's builder (rtw_tri.cpp) and its refit (host: rtw_tri.cpp, device: rtw_refit.hip) share: the inflated
// box of one triangle, the outward roundings, and the two steps of a refit -- one leaf node, one inner node; and the same
// for the top-level tree over mesh placements (builder: mesh_top_build; refit: rtw_tri.cpp / rtw_mesh_move.hip): the world box of one placement
// and the leaf step of its refit.  One __host__ __device__ definition each; every translation unit that includes this is
// built with -ffp-contract=off.
#pragma once
#include "rtw_tri.h"
#include "rtw_mesh.h"

namespace rtw {

// The box of one triangle in double, inflated by the static part of the cull's error radius (DESIGN.md "Rust2 triangles"), and its centre.
struct TriBox { double lo[3], hi[3], c[3]; };

// std::min / std::max as the builder has always used them (the first argument stays on a tie or a NaN), spelled out so that host and device
// select alike
__host__ __device__ __forceinline__ double box_min(double a, double b) { return b < a ? b : a; }
__host__ __device__ __forceinline__ double box_max(double a, double b) { return a < b ? b : a; }
__host__ __device__ __forceinline__ float box_minf(float a, float b) { return b < a ? b : a; }
__host__ __device__ __forceinline__ float box_maxf(float a, float b) { return a < b ? b : a; }

// The f32 neighbour of f towards -inf / +inf (std::nextafter(f, -+INFINITY)) for a number; on the bits, so that no library stands between
// the two sides
__host__ __device__ __forceinline__ float box_next(float f, bool upward) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    if (f == 0.0f) b = upward ? 0x00000001u : 0x80000001u;
    else if (((b >> 31) != 0u) == upward) b = b - 1u;                            // towards zero (from an infinity: the largest number)
    else if ((b & 0x7FFFFFFFu) != 0x7F800000u) b = b + 1u;                       // away from zero (an infinity stays)
    __builtin_memcpy(&f, &b, 4);
    return f;
}
// The outward roundings of a double to f32: the largest f32 <= x, the smallest f32 >= x (NaN stays NaN)
__host__ __device__ __forceinline__ float box_down(double x) { float f = (float)x; if ((double)f > x) f = box_next(f, false); return f; }
__host__ __device__ __forceinline__ float box_up(double x) { float f = (float)x; if ((double)f < x) f = box_next(f, true); return f; }

// The inflated box of a prepared triangle (derived fields set); false: a condition of the cull's derivation fails, the tree must not be used
__host__ __device__ inline bool tri_box(const DevTri &t, TriBox &b) {
    bool ok = true;
    const float *f[] = { t.origin, t.u, t.v, t.normal, t.w };
    for (const float *p : f) for (int k = 0; k < 3; k++) if (!__builtin_isfinite(p[k])) ok = false;
    if (!__builtin_isfinite(t.d)) ok = false;
    if (!ok) {
        for (int k = 0; k < 3; k++) { b.lo[k] = b.hi[k] = b.c[k] = 0.0; }
        return false;
    }
    double amax = 0.0;
    for (int k = 0; k < 3; k++) {
        const double a = t.origin[k], p = a + (double)t.u[k], q = a + (double)t.v[k];
        b.lo[k] = box_min(a, box_min(p, q)); b.hi[k] = box_max(a, box_max(p, q));
        amax = box_max(amax, box_max(__builtin_fabs(b.lo[k]), __builtin_fabs(b.hi[k])));
        if (!(__builtin_fabs((double)t.w[k]) <= 0x1p40)) ok = false;
    }
    const double lu = __builtin_sqrt((double)t.u[0] * t.u[0] + (double)t.u[1] * t.u[1] + (double)t.u[2] * t.u[2]);
    const double lv = __builtin_sqrt((double)t.v[0] * t.v[0] + (double)t.v[1] * t.v[1] + (double)t.v[2] * t.v[2]);
    const double nx = (double)t.u[1] * t.v[2] - (double)t.u[2] * t.v[1], ny = (double)t.u[2] * t.v[0] - (double)t.u[0] * t.v[2],
                 nz = (double)t.u[0] * t.v[1] - (double)t.u[1] * t.v[0];
    const double nl = __builtin_sqrt(nx * nx + ny * ny + nz * nz), e = box_max(lu, lv);
    const double kappa = nl > 0.0 ? e * e / nl : __builtin_huge_val();
    if (!(amax <= 0x1p40) || !(kappa <= 256.0)) ok = false;
    const double r = 0x1p-24 * (256.0 * amax + 4096.0 * kappa * (1.0 + kappa) * e) + 0x1p-100;
    for (int k = 0; k < 3; k++) {
        b.lo[k] -= r; b.hi[k] += r;
        b.c[k] = 0.5 * (b.lo[k] + b.hi[k]);
    }
    return ok;
}

// ---- the refit -----------------------------------------------------------------------------------------------------------
// The topology stays: skip links, leaf words, the leaf order and every `index`.  Both steps are the whole of what either side runs.
//
// One leaf node: each of its triangles takes origin, u, v of its index from `ouv` ([n][9] f32), Triangle::new's derived fields, and is
// written to its slot of `leaf` and to `list[index]` -- rows 0 to 4 without the w words of rows 1 to 4 (index, metallicness, opacity, ir);
// rows 5 and 6 stay.  The node's box becomes the union of the triangles' boxes rounded outward.  Returns how many of them tri_box refuses.
__host__ __device__ inline uint32_t refit_leaf_node(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, uint32_t node) {
    TriNode &nd = nodes[node];
    const uint32_t first = nd.leaf >> 3, cnt = nd.leaf & 7u;
    float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
    uint32_t bad = 0;
    for (uint32_t j = first; j < first + cnt; j++) {
        DevTri &slot = leaf[j];
        const uint32_t index = slot.index;
        const float *s = ouv + 9 * (size_t)index;
        DevTri t;
        for (int k = 0; k < 3; k++) { t.origin[k] = s[k]; t.u[k] = s[3 + k]; t.v[k] = s[6 + k]; }
        tri_derive(t.origin, t.u, t.v, t.normal, t.d, t.w);
        DevTri &row = list[index];
        for (int k = 0; k < 3; k++) {
            slot.origin[k] = row.origin[k] = t.origin[k]; slot.u[k] = row.u[k] = t.u[k]; slot.v[k] = row.v[k] = t.v[k];
            slot.normal[k] = row.normal[k] = t.normal[k]; slot.w[k] = row.w[k] = t.w[k];
        }
        slot.d = row.d = t.d;
        TriBox b;
        if (!tri_box(t, b)) bad++;
        for (int k = 0; k < 3; k++) {
            const float l = box_down(b.lo[k]), h = box_up(b.hi[k]);
            lo[k] = j == first ? l : box_minf(lo[k], l); hi[k] = j == first ? h : box_maxf(hi[k], h);
        }
    }
    for (int k = 0; k < 3; k++) { nd.lo[k] = lo[k]; nd.hi[k] = hi[k]; }
    return bad;
}
// One inner node, after both children: down and up are monotone, so the f32 union of the children's boxes is the outward rounding of the
// double union the builder forms
__host__ __device__ inline void refit_inner_node(TriNode *nodes, uint32_t node) {
    const TriNode &l = nodes[node + 1];
    const TriNode &r = nodes[l.skip];
    TriNode &nd = nodes[node];
    for (int k = 0; k < 3; k++) { nd.lo[k] = box_minf(l.lo[k], r.lo[k]); nd.hi[k] = box_maxf(l.hi[k], r.hi[k]); }
}

// ---- the top-level tree over mesh placements ---------------------------------------------------------------------------
// The world box of one placement {qrow = qn as w, x, y, z; prow = position, 0}.  The local frame is x' = qn.rotate(x - position), so the
// geometry a ray meets stands at conj(qn).rotate(x') + position -- the CONJUGATE rotation, not the q.rotate(p') + position of the hit record.
// The eight corners of the mesh tree's root box (padded by r_static already) are turned in double precision (qn's f32 components are exact
// doubles; the map is linear, so the image of the box lies in the corners' hull), then the box is padded by the static part of 4.11's bound,
// c2 u (|position|_inf + rho) with c2 = 512 and rho the largest corner norm, plus 2^-40 of its size for the double arithmetic itself.
// The builder (mesh_top_build) and the refit on either side (mesh_top_refit_leaf) call this one definition.
__host__ __device__ inline bool placement_box(const TriNode &root, const f4 &qrow, const f4 &prow, TriBox &b) {
    const double w = qrow.x, x = qrow.y, y = qrow.z, z = qrow.w;
    const double pos[3] = { prow.x, prow.y, prow.z };
    double rho = 0.0, pmax = 0.0, amax = 0.0;
    for (int k = 0; k < 3; k++) { b.lo[k] = __builtin_huge_val(); b.hi[k] = -__builtin_huge_val(); pmax = box_max(pmax, __builtin_fabs(pos[k])); }
    for (int c = 0; c < 8; c++) {
        const double v[3] = { (c & 1) ? root.hi[0] : root.lo[0], (c & 2) ? root.hi[1] : root.lo[1], (c & 4) ? root.hi[2] : root.lo[2] };
        rho = box_max(rho, __builtin_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
        // conj(qn) (0, v) qn, the vector part: with r = -(x, y, z) it is v (w^2 - r.r) + 2 r (r.v) + 2 w (r x v)
        const double r[3] = { -x, -y, -z };
        const double rr = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], rv = r[0] * v[0] + r[1] * v[1] + r[2] * v[2];
        const double cx[3] = { r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0] };
        for (int k = 0; k < 3; k++) {
            const double p = v[k] * (w * w - rr) + 2.0 * r[k] * rv + 2.0 * w * cx[k] + pos[k];
            b.lo[k] = box_min(b.lo[k], p); b.hi[k] = box_max(b.hi[k], p);
        }
    }
    const double pad = 0x1p-24 * 512.0 * (pmax + rho);
    for (int k = 0; k < 3; k++) amax = box_max(amax, box_max(__builtin_fabs(b.lo[k]), __builtin_fabs(b.hi[k])));
    const double slack = pad + 0x1p-40 * amax + 0x1p-100;
    for (int k = 0; k < 3; k++) { b.lo[k] -= slack; b.hi[k] += slack; b.c[k] = 0.5 * (b.lo[k] + b.hi[k]); }
    // the reach of the bound: the placement and the mesh within RTW_MESH_TOP_REACH of their origins (the per-ray test of mesh_top_ray_ordinary
    // then implies tri_ray_ordinary in this placement's frame)
    return __builtin_isfinite(rho) && pmax <= (double)RTW_MESH_TOP_REACH && rho <= (double)RTW_MESH_TOP_REACH;
}

// One leaf node of the top-level tree, the whole of what either side runs for it: each of its at most 4 placements k = order[first + j]
// takes its rows from poses[7 k ..] (mesh_pose_rows; `poses` null: the rows stay) -- an INVALID pose writes nothing, the placement keeps its
// previous rows -- and its world box from the rows it now has and `root`, the mesh tree's node 0; the node's box becomes the union of the
// boxes rounded outward.  Each placement sits in exactly one leaf: its rows have one writer.  Counts the invalid poses and the placements
// placement_box puts beyond the reach of its bound.
struct MeshMoveCount { uint32_t invalid, beyond; };
__host__ __device__ inline MeshMoveCount mesh_top_refit_leaf(TriNode *nodes, const uint32_t *order, f4 *rows, const float *poses, const TriNode &root,
                                                            uint32_t node) {
    TriNode &nd = nodes[node];
    const uint32_t first = nd.leaf >> 3, cnt = nd.leaf & 7u;
    float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
    MeshMoveCount n = { 0u, 0u };
    for (uint32_t j = first; j < first + cnt; j++) {
        const uint32_t k = order[j];
        f4 a = rows[2 * (size_t)k], b = rows[2 * (size_t)k + 1];
        if (poses) {
            if (mesh_pose_rows(poses + 7 * (size_t)k, a, b)) { rows[2 * (size_t)k] = a; rows[2 * (size_t)k + 1] = b; }
            else n.invalid++;
        }
        TriBox box;
        if (!placement_box(root, a, b, box)) n.beyond++;
        for (int c = 0; c < 3; c++) {
            const float l = box_down(box.lo[c]), h = box_up(box.hi[c]);
            lo[c] = j == first ? l : box_minf(lo[c], l); hi[c] = j == first ? h : box_maxf(hi[c], h);
        }
    }
    for (int c = 0; c < 3; c++) { nd.lo[c] = lo[c]; nd.hi[c] = hi[c]; }
    return n;
}
// (The inner step is refit_inner_node, above.)

// The motion row of one placement that went from pose `prev` to pose `cur` ([7] f32 each), the whole of what either side runs for it
// (rtw_mesh_instance_motion, rtw.h): with (qn, pos) the rows of mesh_pose_rows -- the very quaternion the walk turns rays by --, points go
// current -> previous by R(conj qn_p) R(qn_c), the normals the hit records carry by R(qn_p) R(conj qn_c); the columns are the images of the
// unit vectors under quat_rotate_n.  Equal bytes: the identity row, moving 0.  A refused pose: moving 1 and NaN in a.  Returns whether a
// pose was refused (equal poses included).
__host__ __device__ inline bool mesh_motion_row(const float *prev, const float *cur, RtwMotionRow &r) {
    bool same = true;
    for (int k = 0; k < 7; k++) same = same && mesh_bits(prev[k]) == mesh_bits(cur[k]);
    f4 ca, cb, pa, pb;
    const bool ok_c = mesh_pose_rows(cur, ca, cb), ok_p = mesh_pose_rows(prev, pa, pb);
    for (int k = 0; k < 9; k++) r.a[k] = r.nrm[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    for (int k = 0; k < 3; k++) r.from[k] = r.to[k] = 0.0f;
    for (int k = 0; k < 7; k++) r.pad[k] = 0u;
    r.moving = same ? 0u : 1u;
    if (same) return !ok_c;
    if (!ok_c || !ok_p) {
        for (int k = 0; k < 9; k++) r.a[k] = __builtin_bit_cast(float, 0x7fc00000u);
        return true;
    }
    const quat qc = qmk(ca.x, ca.y, ca.z, ca.w), qp = qmk(pa.x, pa.y, pa.z, pa.w);
    const quat qcc = qmk(qc.w, -qc.x, -qc.y, -qc.z), qpc = qmk(qp.w, -qp.x, -qp.y, -qp.z);
    for (int j = 0; j < 3; j++) {
        const float e0 = j == 0 ? 1.0f : 0.0f, e1 = j == 1 ? 1.0f : 0.0f, e2 = j == 2 ? 1.0f : 0.0f;
        float x, y, z;
        quat_rotate_n(qc, e0, e1, e2, x, y, z);
        quat_rotate_n(qpc, x, y, z, r.a[j], r.a[3 + j], r.a[6 + j]);
        quat_rotate_n(qcc, e0, e1, e2, x, y, z);
        quat_rotate_n(qp, x, y, z, r.nrm[j], r.nrm[3 + j], r.nrm[6 + j]);
    }
    r.from[0] = cb.x; r.from[1] = cb.y; r.from[2] = cb.z;
    r.to[0] = pb.x; r.to[1] = pb.y; r.to[2] = pb.z;
    return false;
}

// ---- per-pixel motion of a deforming mesh (rtw.h "previous points of a deformed mesh") ----------------------------------------
// The triangle and the barycentrics under a ray whose hit parameter is t, from the mesh's ouv rows alone (rtw_tri_bary): Triangle::new's w
// of the row (tri_derive), then the interior part of the hit test (tri_inside) -- what the surface kernel writes for a winner of kind 3 or 4,
// whose list rows hold the same tri_derive of the same ouv.  `tri` outside [0, n_tris), decided without wrap-around: 0 0, no address formed.
__host__ __device__ inline void tri_bary_one(const float *ouv, uint32_t n_tris, const float *ray, float t, int32_t tri, float *bary) {
    bary[0] = 0.0f; bary[1] = 0.0f;
    if (tri < 0 || (int64_t)tri >= (int64_t)n_tris) return;
    const float *s = ouv + 9 * (size_t)tri;
    float normal[3], w[3], d;
    tri_derive(s, s + 3, s + 6, normal, d, w);
    tri_inside(s, s + 3, s + 6, w, ray[0], ray[1], ray[2], ray[3], ray[4], ray[5], t, bary[0], bary[1]);
}

// What the deform pass takes besides the per-pixel tri and bary: the previous frame's mesh, and for a placed mesh the pixels' ids and the
// previous poses (poses null: the mesh stands in world space; idx and first are then not read).
struct DeformMesh { const float *prev_ouv; uint32_t n_tris; const int32_t *idx; const float *prev_poses; uint32_t n_mesh, first; };

// One pixel: where its surface point lay a frame ago and the normal it had there; the whole of what either side runs for it.
//   a point:   0 <= tri < n_tris (and, with poses, 0 <= k = idx - first < n_mesh in 64 bits);   {o, u, v} = row tri of prev_ouv
//              x'_c = (o_c + alfa * u_c) + beta * v_c;   n' = tri_derive's normal of the row
//              without poses: point = x', normal = n';  with (qn, pos) = mesh_pose_rows(pose k): point = rotate(conj(qn), x') + pos,
//              normal = rotate(qn, n')  (quat_rotate_n: the placement meets rays at conj(qn).rotate(x') + pos and reports qn.rotate(n'))
//   no point:  the quiet NaN 0x7fc00000 in all six; also for a pose mesh_pose_rows refuses.  No address is formed from such a tri or k.
__host__ __device__ inline void deform_point(const DeformMesh &m, int32_t tri, float alfa, float beta, int32_t id, float *point, float *normal) {
    const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
    for (int c = 0; c < 3; c++) { point[c] = qnan; normal[c] = qnan; }
    if (tri < 0 || (int64_t)tri >= (int64_t)m.n_tris) return;
    f4 qa, qb;
    if (m.prev_poses) {
        const int64_t k = (int64_t)id - (int64_t)m.first;
        if (k < 0 || k >= (int64_t)m.n_mesh) return;
        if (!mesh_pose_rows(m.prev_poses + 7 * (size_t)k, qa, qb)) return;
    }
    const float *s = m.prev_ouv + 9 * (size_t)tri;
    float x[3], n[3], w[3], d;
    for (int c = 0; c < 3; c++) x[c] = (s[c] + alfa * s[3 + c]) + beta * s[6 + c];
    tri_derive(s, s + 3, s + 6, n, d, w);
    if (m.prev_poses) {
        const quat qn = qmk(qa.x, qa.y, qa.z, qa.w), qc = qmk(qn.w, -qn.x, -qn.y, -qn.z);
        float r0, r1, r2;
        quat_rotate_n(qc, x[0], x[1], x[2], r0, r1, r2);
        x[0] = r0 + qb.x; x[1] = r1 + qb.y; x[2] = r2 + qb.z;
        quat_rotate_n(qn, n[0], n[1], n[2], r0, r1, r2);
        n[0] = r0; n[1] = r1; n[2] = r2;
    }
    for (int c = 0; c < 3; c++) { point[c] = x[c]; normal[c] = n[c]; }
}
// Everything rtw_deform_motion refuses (rtw.h)
inline bool deform_args_ok(const int32_t *tri, const float *bary, uint32_t n, const DeformMesh &m, const float *point, const float *normal) {
    if (!tri || !bary || !m.prev_ouv || !point || !normal || n == 0 || m.n_tris == 0) return false;
    if (m.prev_poses && (!m.idx || m.n_mesh == 0 || m.n_mesh > RTW_MAX_MESH_INSTANCES)) return false;
    return true;
}

// ---- host (rtw_tri.cpp) ---------------------------------------------------------------------------------------------------------------------
// The order a refit visits the nodes in: `order` holds every node index sorted by height (a leaf: 0; an inner node: 1 + the higher child),
// ties by index; height h owns order[first[h] .. first[h + 1]), first.size() = heights + 1.  Height 0 is the leaf pass, each further height
// one launch.  False when memory runs out.
struct RefitSchedule {
    std::vector<uint32_t> order, first;
};
bool tri_refit_schedule(const TriNode *nodes, uint32_t n_nodes, RefitSchedule &out);
// The refit on the host, over the same schedule: returns the number of triangles tri_box refuses
uint32_t tri_refit_host(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, const RefitSchedule &s);
// The top-level tree's refit on the host, over its schedule (`top_order`: the placement indices in leaf order)
MeshMoveCount mesh_top_refit_host(TriNode *nodes, const uint32_t *top_order, f4 *rows, const float *poses, const TriNode &root, const RefitSchedule &s);

// ---- device (rtw_refit.hip) -----------------------------------------------------------------------------------------------------------------
// The refit on `stream`: the leaf pass, then one launch per height; device pointers, `order` = RefitSchedule.order uploaded, `first` the host
// array; *bad (device u32, zeroed by the caller) receives the count.  Allocates nothing.
void launch_tri_refit(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, const uint32_t *order, const uint32_t *first,
                      uint32_t n_heights, uint32_t *bad, hipStream_t stream);
// The climb alone, one launch of the inner kernel per height 1 .. n_heights - 1 (`first` the host array): the form the triangle refit runs,
// for any tree in the TriNode format
void launch_refit_climb(TriNode *nodes, const uint32_t *order, const uint32_t *first, uint32_t n_heights, hipStream_t stream);

// ---- device (rtw_mesh_move.hip) -------------------------------------------------------------------------------------------------------------
// The top-level tree's refit on `stream` (rtw_ctx_move_mesh_instances): the placement pass -- one thread per leaf node,
// mesh_top_refit_leaf with `root` = the mesh tree's node 0 ON THE DEVICE --, then the climb: one_group false: launch_refit_climb; true: ONE
// launch of one workgroup that loops over the heights itself (d_first: `first` on the device).  counts: two device u32 (invalid, beyond),
// zeroed by the caller.  Allocates nothing.
// Which climb: measured (profiles/mesh_move.log), the one workgroup is ahead of the launches per height at 31, 511, 2047
// and 8191 nodes (by 8 to 19 %) and 39 % behind them at 32 767.  It serves trees of up to 8192 nodes, the largest size at which it was seen
// ahead; where between 8191 and 32 767 nodes the two cross was not resolved.
#define RTW_MESH_CLIMB_ONE_GROUP_MAX 8192u
inline bool mesh_climb_one_group(uint32_t n_nodes) { return n_nodes <= RTW_MESH_CLIMB_ONE_GROUP_MAX; }
void launch_mesh_move(TriNode *top, const uint32_t *top_order, f4 *rows, const float *poses, const TriNode *root, const uint32_t *order,
                      const uint32_t *first, const uint32_t *d_first, uint32_t n_heights, bool one_group, uint32_t *counts, hipStream_t stream);
// rtw_ctx_mesh_instance_motion on `stream`: one thread per placement running mesh_motion_row; device pointers, *n_invalid (device u32, zeroed by
// the caller) receives the count of refused poses.  Allocates nothing.
void launch_mesh_motion(const float *prev_poses, const float *cur_poses, uint32_t n, RtwMotionRow *rows, uint32_t *n_invalid, hipStream_t stream);
// rtw_ctx_deform_motion on `stream`: one thread per pixel running deform_point; device pointers.  Allocates nothing.
void launch_deform_motion(const int32_t *tri, const float *bary, uint32_t n, const DeformMesh &m, float *point, float *normal, hipStream_t stream);

} // namespace rtw
