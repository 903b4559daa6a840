// rtw_tri.cpp -- host side of Rust2's triangles: Triangle::new, the tree builder (binned SAH, leaves of <= 4, bounded depth), its
// self-check and the host list walk (DESIGN.md "Rust2 triangles").
#include "rtw_tri.h"
#include "rtw_mesh.h"
#include "rtw_occl.h"
#include "rtw_refit.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace rtw {

static const float TRI_DEFAULT_M[3] = { 0.0f, 0.0f, 1.0f };     // the quad default (rtw_quad_new: EMPTY_M == SCATTER_M)

void tri_prepare(const RtwTriangle *t, uint32_t n, DevTri *list) {
    for (uint32_t i = 0; i < n; i++) {
        const RtwTriangle &s = t[i];
        DevTri &d = list[i];
        std::memset(&d, 0, sizeof d);
        for (int k = 0; k < 3; k++) {
            d.origin[k] = s.origin[k]; d.u[k] = s.u[k]; d.v[k] = s.v[k];
            d.albedo[k] = s.tex_color[k] * 1.0f;                  // (the quad's texel * 1.0; Rust2's ConstColorTexture: the same bits)
            d.emitted[k] = s.emitted[k];
        }
        tri_derive(d.origin, d.u, d.v, d.normal, d.d, d.w);
        d.index = i;
        d.metallicness = s.metallicness; d.opacity = s.opacity; d.ir = s.ir; d.tex = s.tex;
    }
}

TriBuild::~TriBuild() { delete[] nodes; delete[] leaf; }

namespace {

// (The per-triangle box, tri_box, and the outward roundings live in rtw_refit.h: the refit on the device runs the same definitions.)

// Binned SAH over box centres with a median fallback, leaves of <= 4: the triangle tree's builder, and the top-level tree's over the
// placements' world boxes (mesh_top_build).  `order`: the items in leaf order; a leaf names a run of it.  Deterministic: no RNG, ties by index.
struct Builder {
    const std::vector<TriBox> &box;
    std::vector<uint32_t> idx;
    std::vector<TriNode> nodes;
    std::vector<uint32_t> order;
    uint32_t depth = 0;

    static float down(double x) { return box_down(x); }
    static float up(double x) { return box_up(x); }
    static double area(const double *lo, const double *hi) {
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    }

    void build(uint32_t begin, uint32_t end, uint32_t level) {
        depth = std::max(depth, level);
        const uint32_t me = (uint32_t)nodes.size();
        nodes.push_back(TriNode{});
        double lo[3] = { HUGE_VAL, HUGE_VAL, HUGE_VAL }, hi[3] = { -HUGE_VAL, -HUGE_VAL, -HUGE_VAL };
        double clo[3] = { HUGE_VAL, HUGE_VAL, HUGE_VAL }, chi[3] = { -HUGE_VAL, -HUGE_VAL, -HUGE_VAL };
        for (uint32_t i = begin; i < end; i++) {
            const TriBox &b = box[idx[i]];
            for (int k = 0; k < 3; k++) {
                lo[k] = std::min(lo[k], b.lo[k]); hi[k] = std::max(hi[k], b.hi[k]);
                clo[k] = std::min(clo[k], b.c[k]); chi[k] = std::max(chi[k], b.c[k]);
            }
        }
        for (int k = 0; k < 3; k++) { nodes[me].lo[k] = down(lo[k]); nodes[me].hi[k] = up(hi[k]); }
        const uint32_t n = end - begin;
        if (n <= 4) {
            nodes[me].leaf = ((uint32_t)order.size() << 3) | n;
            for (uint32_t i = begin; i < end; i++) order.push_back(idx[i]);
            nodes[me].skip = (uint32_t)nodes.size();
            return;
        }
        // binned SAH over the box centres (16 bins per axis); past depth 48, or when no split separates anything, the median of the widest axis
        enum { B = 16 };
        int axis = -1; uint32_t split_bin = 0; double best = HUGE_VAL;
        if (level < 48) {
            for (int k = 0; k < 3; k++) {
                const double ext = chi[k] - clo[k];
                if (!(ext > 0.0)) continue;
                uint32_t cnt[B] = {}; double blo[B][3], bhi[B][3];
                for (int j = 0; j < B; j++) for (int a = 0; a < 3; a++) { blo[j][a] = HUGE_VAL; bhi[j][a] = -HUGE_VAL; }
                for (uint32_t i = begin; i < end; i++) {
                    const TriBox &b = box[idx[i]];
                    int j = (int)((b.c[k] - clo[k]) / ext * B); j = j < 0 ? 0 : j >= B ? B - 1 : j;
                    cnt[j]++;
                    for (int a = 0; a < 3; a++) { blo[j][a] = std::min(blo[j][a], b.lo[a]); bhi[j][a] = std::max(bhi[j][a], b.hi[a]); }
                }
                double rlo[3] = { HUGE_VAL, HUGE_VAL, HUGE_VAL }, rhi[3] = { -HUGE_VAL, -HUGE_VAL, -HUGE_VAL };
                double rcost[B]; uint32_t rn = 0;
                for (int j = B - 1; j > 0; j--) {
                    for (int a = 0; a < 3; a++) { rlo[a] = std::min(rlo[a], blo[j][a]); rhi[a] = std::max(rhi[a], bhi[j][a]); }
                    rn += cnt[j];
                    rcost[j] = rn ? area(rlo, rhi) * rn : 0.0;
                }
                double llo[3] = { HUGE_VAL, HUGE_VAL, HUGE_VAL }, lhi[3] = { -HUGE_VAL, -HUGE_VAL, -HUGE_VAL };
                uint32_t ln = 0;
                for (int j = 0; j < B - 1; j++) {
                    for (int a = 0; a < 3; a++) { llo[a] = std::min(llo[a], blo[j][a]); lhi[a] = std::max(lhi[a], bhi[j][a]); }
                    ln += cnt[j];
                    if (ln == 0 || ln == n) continue;
                    const double c = area(llo, lhi) * ln + rcost[j + 1];
                    if (c < best) { best = c; axis = k; split_bin = (uint32_t)j; }
                }
            }
        }
        uint32_t mid;
        if (axis >= 0) {
            const double ext = chi[axis] - clo[axis];
            auto left = [&](uint32_t t) {
                int j = (int)((box[t].c[axis] - clo[axis]) / ext * B); j = j < 0 ? 0 : j >= B ? B - 1 : j;
                return (uint32_t)j <= split_bin;
            };
            mid = (uint32_t)(std::partition(idx.begin() + begin, idx.begin() + end, left) - idx.begin());
        } else {
            int k = 0;
            for (int a = 1; a < 3; a++) if (chi[a] - clo[a] > chi[k] - clo[k]) k = a;
            mid = begin + n / 2;
            std::nth_element(idx.begin() + begin, idx.begin() + mid, idx.begin() + end, [&](uint32_t x, uint32_t y) {
                return box[x].c[k] < box[y].c[k] || (box[x].c[k] == box[y].c[k] && x < y);
            });
        }
        build(begin, mid, level + 1);
        build(mid, end, level + 1);
        nodes[me].leaf = 0;
        nodes[me].skip = (uint32_t)nodes.size();
    }
};

} // namespace

bool tri_build(const DevTri *list, uint32_t n, TriBuild &out) {
    try {
        std::vector<TriBox> box(n);
        bool ok = true;
        for (uint32_t i = 0; i < n; i++) if (!tri_box(list[i], box[i])) ok = false;
        Builder b{ box, {}, {}, {} };
        b.idx.resize(n);
        for (uint32_t i = 0; i < n; i++) b.idx[i] = i;
        b.nodes.reserve(n > 0 ? 2 * ((size_t)n / 2 + 1) : 0);
        b.order.reserve(n);
        if (n) b.build(0, n, 0);
        out.n_nodes = (uint32_t)b.nodes.size();
        out.nodes = new TriNode[b.nodes.size() + 1];
        out.leaf = new DevTri[b.order.size() + 1];
        std::copy(b.nodes.begin(), b.nodes.end(), out.nodes);
        for (size_t i = 0; i < b.order.size(); i++) out.leaf[i] = list[b.order[i]];
        out.depth = b.depth;
        out.list_walk = !ok;
        return true;
    } catch (const std::bad_alloc &) {
        return false;
    }
}

// ---- the refit of the triangle tree ----------------------------------------------------------------------------------------
bool tri_refit_schedule(const TriNode *nodes, uint32_t n_nodes, RefitSchedule &out) {
    try {
        // depth-first order: both children of a node come after it, so one backward sweep knows them
        std::vector<uint32_t> height(n_nodes, 0);
        uint32_t top = 0;
        for (uint32_t i = n_nodes; i-- > 0;) {
            if (!nodes[i].leaf) height[i] = 1u + std::max(height[i + 1], height[nodes[i + 1].skip]);
            top = std::max(top, height[i]);
        }
        out.first.assign(n_nodes ? (size_t)top + 2 : 1, 0);
        for (uint32_t i = 0; i < n_nodes; i++) out.first[height[i] + 1]++;
        for (size_t h = 1; h < out.first.size(); h++) out.first[h] += out.first[h - 1];
        out.order.resize(n_nodes);
        std::vector<uint32_t> at(out.first.begin(), out.first.end() - (n_nodes ? 1 : 0));
        for (uint32_t i = 0; i < n_nodes; i++) out.order[at[height[i]]++] = i;
        return true;
    } catch (const std::bad_alloc &) {
        return false;
    }
}

uint32_t tri_refit_host(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, const RefitSchedule &s) {
    uint32_t bad = 0;
    for (size_t h = 0; h + 1 < s.first.size(); h++)
        for (uint32_t k = s.first[h]; k < s.first[h + 1]; k++) {
            if (h == 0) bad += refit_leaf_node(nodes, leaf, list, ouv, s.order[k]);
            else refit_inner_node(nodes, s.order[k]);
        }
    return bad;
}

MeshMoveCount mesh_top_refit_host(TriNode *nodes, const uint32_t *top_order, f4 *rows, const float *poses, const TriNode &root, const RefitSchedule &s) {
    MeshMoveCount n = { 0u, 0u };
    for (size_t h = 0; h + 1 < s.first.size(); h++)
        for (uint32_t k = s.first[h]; k < s.first[h + 1]; k++) {
            if (h == 0) {
                const MeshMoveCount m = mesh_top_refit_leaf(nodes, top_order, rows, poses, root, s.order[k]);
                n.invalid += m.invalid; n.beyond += m.beyond;
            } else refit_inner_node(nodes, s.order[k]);
        }
    return n;
}

// ---- the top-level tree over mesh placements ---------------------------------------------------------------------------
std::vector<unsigned char> MeshTopBuild::packed() const {
    std::vector<unsigned char> out(nodes.size() * sizeof(TriNode) + order.size() * sizeof(uint32_t));
    if (!nodes.empty()) std::memcpy(out.data(), nodes.data(), nodes.size() * sizeof(TriNode));
    if (!order.empty()) std::memcpy(out.data() + nodes.size() * sizeof(TriNode), order.data(), order.size() * sizeof(uint32_t));
    return out;
}

// (The world box of one placement, placement_box, lives in rtw_refit.h: the refit on the device runs the same definition.)
bool mesh_top_build(const TriNode &root, const f4 *rows, uint32_t n, MeshTopBuild &out) {
    try {
        std::vector<TriBox> box(n);
        bool ok = true;
        for (uint32_t i = 0; i < n; i++) if (!placement_box(root, rows[2 * (size_t)i], rows[2 * (size_t)i + 1], box[i])) ok = false;
        if (!ok) for (uint32_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) if (!std::isfinite(box[i].lo[k]) || !std::isfinite(box[i].hi[k])) {
            box[i].lo[k] = box[i].hi[k] = box[i].c[k] = 0.0;      // (a refused context's tree is never walked: any finite box will do)
        }
        Builder b{ box, {}, {}, {} };
        b.idx.resize(n);
        for (uint32_t i = 0; i < n; i++) b.idx[i] = i;
        b.nodes.reserve(2 * ((size_t)n / 2 + 1));
        b.order.reserve(n);
        if (n) b.build(0, n, 0);
        out.nodes = std::move(b.nodes);
        out.order = std::move(b.order);
        out.depth = b.depth;
        out.list_walk = !ok;
        return true;
    } catch (const std::bad_alloc &) {
        return false;
    }
}

} // namespace rtw

using namespace rtw;

extern "C" {

int rtw_triangle_new(const float origin[3], const float u[3], const float v[3], const float *mat3, const float *emitted,
                     const float color[3], int32_t tex, RtwTriangle *out) {
    if (!origin || !u || !v || !color || !out || tex < -1) return RTW_E_INVALID;
    std::memset(out, 0, sizeof *out);
    const float *m = mat3 ? mat3 : TRI_DEFAULT_M;
    for (int k = 0; k < 3; k++) {
        out->origin[k] = origin[k]; out->u[k] = u[k]; out->v[k] = v[k];
        out->tex_color[k] = color[k];
        out->emitted[k] = emitted ? emitted[k] : 0.0f;
    }
    tri_derive(out->origin, out->u, out->v, out->normal, out->d, out->w);
    out->metallicness = m[0]; out->opacity = m[1]; out->ir = m[2];
    out->tex = tex;
    return RTW_OK;
}

int rtw_triangle_hits(const RtwTriangle *tris, uint32_t n, const float *rays, uint32_t n_rays, float mint, float maxt,
                      float *t_out, int32_t *idx_out) {
    if ((n && !tris) || !rays || !t_out || !idx_out || n_rays == 0) return RTW_E_INVALID;
    std::vector<DevTri> list;
    try { list.resize(n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    tri_prepare(tris, n, list.data());
    for (uint32_t i = 0; i < n_rays; i++) {
        const float *r = rays + 6 * (size_t)i;
        float t;
        const int k = tri_closest_host(list.data(), n, r[0], r[1], r[2], r[3], r[4], r[5], mint, maxt, t);
        t_out[i] = k >= 0 ? t : INFINITY;
        idx_out[i] = k;
    }
    return RTW_OK;
}

// The argument checks rtw_ctx_set_mesh_instances makes, in its order (rtw_shim.hip), without a context
int rtw_mesh_instances_validate(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *p, uint32_t n) {
    if (n_tris && !tris) return RTW_E_INVALID;
    if (!n_tris) return RTW_E_NO_SCENE;
    if ((n && !p) || (!n && p) || n > RTW_MAX_MESH_INSTANCES) return RTW_E_INVALID;
    if (!n) return RTW_OK;
    for (uint32_t i = 0; i < n_tris; i++) if (tris[i].tex >= 0) return RTW_E_INVALID;
    return mesh_rows(p, n, nullptr) ? RTW_OK : RTW_E_INVALID;
}

int rtw_mesh_instance_hits(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *p, uint32_t n, const float *rays, uint32_t n_rays,
                           float mint, float maxt, float *t_out, int32_t *placement_out, int32_t *tri_out, float *normal_out) {
    if (!rays || !t_out || !placement_out || !tri_out || n_rays == 0 || n == 0) return RTW_E_INVALID;
    if (const int rc = rtw_mesh_instances_validate(tris, n_tris, p, n)) return rc;
    std::vector<DevTri> list;
    std::vector<f4> rows;
    try { list.resize(n_tris); rows.resize(2 * (size_t)n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    tri_prepare(tris, n_tris, list.data());
    mesh_rows(p, n, rows.data());
    for (uint32_t i = 0; i < n_rays; i++) {
        float t;
        int j;
        const int k = mesh_closest_host(list.data(), n_tris, rows.data(), n, rays + 6 * (size_t)i, mint, maxt, j, t);
        t_out[i] = k >= 0 ? t : INFINITY;
        placement_out[i] = k;
        tri_out[i] = k >= 0 ? j : -1;
        if (normal_out) {
            float *o = normal_out + 3 * (size_t)i;
            o[0] = o[1] = o[2] = 0.0f;
            if (k >= 0) {
                const f4 a = rows[2 * (size_t)k];
                quat_rotate_n(qmk(a.x, a.y, a.z, a.w), list[j].normal[0], list[j].normal[1], list[j].normal[2], o[0], o[1], o[2]);
            }
        }
    }
    return RTW_OK;
}

// What a context holds for the placements `p` of the mesh `tris`: the rows, the mesh's tree and the top-level tree (rtw_ctx_set_triangles +
// rtw_ctx_set_mesh_instances, without a context)
namespace {
struct HostMesh {
    std::vector<DevTri> list;
    std::vector<f4> rows;
    TriBuild tree;
    MeshTopBuild top;
    std::vector<unsigned char> packed;
};
int host_mesh(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *p, uint32_t n, HostMesh &m) {
    if (n == 0) return RTW_E_INVALID;
    if (const int rc = rtw_mesh_instances_validate(tris, n_tris, p, n)) return rc;
    try { m.list.resize(n_tris); m.rows.resize(2 * (size_t)n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    tri_prepare(tris, n_tris, m.list.data());
    mesh_rows(p, n, m.rows.data());
    if (!tri_build(m.list.data(), n_tris, m.tree)) return RTW_E_NOMEM;
    if (!mesh_top_build(m.tree.nodes[0], m.rows.data(), n, m.top)) return RTW_E_NOMEM;
    return RTW_OK;
}
} // namespace

int rtw_mesh_top_dump(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *p, uint32_t n, RtwTriNode *nodes_out, uint32_t node_cap,
                      uint32_t *n_nodes, uint32_t *order_out, uint32_t *depth, uint32_t *list_walk) {
    static_assert(sizeof(RtwTriNode) == sizeof(TriNode), "the public node is the device's");
    HostMesh m;
    if (const int rc = host_mesh(tris, n_tris, p, n, m)) return rc;
    const uint32_t nn = (uint32_t)m.top.nodes.size();
    if (n_nodes) *n_nodes = nn;
    if (depth) *depth = m.top.depth;
    if (list_walk) *list_walk = (m.top.list_walk || m.tree.list_walk) ? 1u : 0u;
    if (nodes_out) {
        if (node_cap < nn) return RTW_E_INVALID;
        std::memcpy(nodes_out, m.top.nodes.data(), nn * sizeof(TriNode));
    }
    if (order_out) std::memcpy(order_out, m.top.order.data(), n * sizeof(uint32_t));
    return RTW_OK;
}

// What a context holds after rtw_ctx_set_triangles + rtw_ctx_set_mesh_instances(p) + rtw_ctx_move_mesh_instances(moved, ouv), without a context:
// the functions and the schedules the device runs, in its order -- the mesh's refit, the placement pass from the refitted root, the climb
int rtw_mesh_top_refit(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *p, uint32_t n, const float *moved, const float *ouv,
                       RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes, float *rows_out, uint32_t *list_walk, uint32_t *n_invalid) {
    HostMesh m;
    if (const int rc = host_mesh(tris, n_tris, p, n, m)) return rc;
    const uint32_t nn = (uint32_t)m.top.nodes.size();
    if (n_nodes) *n_nodes = nn;
    if (nodes_out && node_cap < nn) return RTW_E_INVALID;
    RefitSchedule ts, s;
    if ((ouv && !tri_refit_schedule(m.tree.nodes, m.tree.n_nodes, ts)) || !tri_refit_schedule(m.top.nodes.data(), nn, s)) return RTW_E_NOMEM;
    uint32_t bad = m.tree.list_walk ? 1u : 0u;
    if (ouv) bad = tri_refit_host(m.tree.nodes, m.tree.leaf, m.list.data(), ouv, ts) ? 1u : 0u;
    const MeshMoveCount c = mesh_top_refit_host(m.top.nodes.data(), m.top.order.data(), m.rows.data(), moved, m.tree.nodes[0], s);
    if (list_walk) *list_walk = bad | (c.beyond ? 2u : 0u);
    if (n_invalid) *n_invalid = c.invalid;
    if (nodes_out) std::memcpy(nodes_out, m.top.nodes.data(), nn * sizeof(TriNode));
    if (rows_out) std::memcpy(rows_out, m.rows.data(), 2 * (size_t)n * sizeof(f4));
    return RTW_OK;
}

// The motion rows of moved placements (rtw.h): mesh_motion_row per placement, the definition rtw_ctx_mesh_instance_motion's kernel runs
int rtw_mesh_instance_motion(const float *prev_poses, const float *cur_poses, uint32_t n, RtwMotionRow *rows_out, uint32_t *n_invalid) {
    if (!prev_poses || !cur_poses || !rows_out || n == 0 || n > RTW_MAX_MESH_INSTANCES) return RTW_E_INVALID;
    uint32_t bad = 0;
    for (uint32_t k = 0; k < n; k++)
        if (mesh_motion_row(prev_poses + 7 * (size_t)k, cur_poses + 7 * (size_t)k, rows_out[k])) bad++;
    if (n_invalid) *n_invalid = bad;
    return RTW_OK;
}

// The triangle's barycentrics under each ray (rtw.h "surface buffers"): tri_bary_one per ray, what the surface kernel writes for a triangle
int rtw_tri_bary(const float *ouv, uint32_t n_tris, const float *rays, uint32_t n, const float *t, const int32_t *tri, float *bary_out) {
    if (!ouv || !rays || !t || !tri || !bary_out || n == 0 || n_tris == 0) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) tri_bary_one(ouv, n_tris, rays + 6 * (size_t)i, t[i], tri[i], bary_out + 2 * (size_t)i);
    return RTW_OK;
}

// The rays as the placements meet them: ray i turned into the frame of placement idx[i] - first (mesh_pose_rows, quat_rotate_n -- the walk's
// own operations); a ray without a valid placement is copied
int rtw_mesh_local_rays(const float *poses, uint32_t n_mesh, uint32_t first, const int32_t *idx, const float *rays, uint32_t n, float *rays_out) {
    if (!poses || !idx || !rays || !rays_out || n == 0 || n_mesh == 0 || n_mesh > RTW_MAX_MESH_INSTANCES) return RTW_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const float *r = rays + 6 * (size_t)i;
        float *o = rays_out + 6 * (size_t)i;
        const int64_t k = (int64_t)idx[i] - (int64_t)first;
        f4 a, b;
        if (k < 0 || k >= (int64_t)n_mesh || !mesh_pose_rows(poses + 7 * (size_t)k, a, b)) {
            for (int c = 0; c < 6; c++) o[c] = r[c];
            continue;
        }
        const quat qn = qmk(a.x, a.y, a.z, a.w);
        float x, y, z;
        quat_rotate_n(qn, r[0] - b.x, r[1] - b.y, r[2] - b.z, x, y, z);
        o[0] = x; o[1] = y; o[2] = z;
        quat_rotate_n(qn, r[3], r[4], r[5], x, y, z);
        o[3] = x; o[4] = y; o[5] = z;
    }
    return RTW_OK;
}

// Previous points of a deformed mesh (rtw.h): deform_point per pixel, the definition rtw_ctx_deform_motion's kernel runs
int rtw_deform_motion(const int32_t *tri, const float *bary, uint32_t n, const float *prev_ouv, uint32_t n_tris, const int32_t *idx,
                      const float *prev_poses, uint32_t n_mesh, uint32_t first, float *prev_point_out, float *carried_normal_out) {
    const DeformMesh m = { prev_ouv, n_tris, idx, prev_poses, prev_poses ? n_mesh : 0u, prev_poses ? first : 0u };
    if (!deform_args_ok(tri, bary, n, m, prev_point_out, carried_normal_out)) return RTW_E_INVALID;
    for (uint32_t p = 0; p < n; p++)
        deform_point(m, tri[p], bary[2 * (size_t)p], bary[2 * (size_t)p + 1], prev_poses ? idx[p] : 0, prev_point_out + 3 * (size_t)p,
                     carried_normal_out + 3 * (size_t)p);
    return RTW_OK;
}

int rtw_mesh_instance_hits_tree(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *p, uint32_t n, const float *rays, uint32_t n_rays,
                                float mint, float maxt, float *t_out, int32_t *placement_out, int32_t *tri_out, float *normal_out, RtwStats *stats) {
    if (!rays || !t_out || !placement_out || !tri_out || n_rays == 0 || n == 0) return RTW_E_INVALID;
    HostMesh m;
    if (const int rc = host_mesh(tris, n_tris, p, n, m)) return rc;
    try { m.packed = m.top.packed(); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    // the views a context forms under RTW_ACCEL_BVH with RTW_OPT_MESH_LIST_MAX = 0 (rtw_shim.hip: tri_view, mesh_top_view)
    DevTris T{};
    T.list = m.list.data(); T.leaf = m.tree.leaf; T.n = n_tris; T.n_nodes = m.tree.n_nodes;
    T.t_bound = std::fmax(std::fabs(mint), std::fabs(maxt));
    const bool range_ok = std::isfinite(mint) && std::isfinite(maxt) && T.t_bound <= RTW_TRI_COORD_MAX;
    T.nodes = (!m.tree.list_walk && range_ok) ? m.tree.nodes : nullptr;
    const TriNode *top = (T.nodes != nullptr && !m.top.list_walk) ? (const TriNode *)m.packed.data() : nullptr;
    const uint32_t n_top = (uint32_t)m.top.nodes.size();
    unsigned long long tests = 0, visits = 0;
    for (uint32_t i = 0; i < n_rays; i++) {
        const float *r = rays + 6 * (size_t)i;
        float t;
        int j;
        uint32_t n_tests = 0, n_nodes = 0;
        const int k = mesh_closest(T, m.rows.data(), n, top, n_top, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), mint, maxt, false, 0.0f, j, t, n_tests, n_nodes);
        tests += n_tests; visits += n_nodes;
        t_out[i] = k >= 0 ? t : INFINITY;
        placement_out[i] = k;
        tri_out[i] = k >= 0 ? j : -1;
        if (normal_out) {
            float *o = normal_out + 3 * (size_t)i;
            o[0] = o[1] = o[2] = 0.0f;
            if (k >= 0) {
                const f4 a = m.rows[2 * (size_t)k];
                quat_rotate_n(qmk(a.x, a.y, a.z, a.w), m.list[j].normal[0], m.list[j].normal[1], m.list[j].normal[2], o[0], o[1], o[2]);
            }
        }
    }
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->quad_tests = tests; stats->node_tests = visits; }
    return RTW_OK;
}

// The any-hit host forms (rtw_occl.h): the triangle and the placement group of rtw_ctx_scene_occluded's kernel, the same source,
// under the views a context forms with RTW_ACCEL_BVH (and RTW_OPT_MESH_LIST_MAX = 0): the trees where the device would take them, else the lists
int rtw_triangle_occluded(const RtwTriangle *tris, uint32_t n, const float *rays, uint32_t n_rays, float mint, float maxt, uint8_t *occluded_out,
                          RtwStats *stats) {
    if ((n && !tris) || !rays || !occluded_out || n_rays == 0) return RTW_E_INVALID;
    std::vector<DevTri> list;
    try { list.resize(n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    tri_prepare(tris, n, list.data());
    TriBuild tree;
    if (n && !tri_build(list.data(), n, tree)) return RTW_E_NOMEM;
    DevTris T{};
    T.list = list.data(); T.leaf = tree.leaf; T.n = n; T.n_nodes = tree.n_nodes;
    T.t_bound = std::fmax(std::fabs(mint), std::fabs(maxt));
    const bool range_ok = std::isfinite(mint) && std::isfinite(maxt) && T.t_bound <= RTW_TRI_COORD_MAX;
    T.nodes = (n && !tree.list_walk && range_ok) ? tree.nodes : nullptr;
    unsigned long long tests = 0, visits = 0;
    for (uint32_t i = 0; i < n_rays; i++) {
        const float *r = rays + 6 * (size_t)i;
        uint32_t n_tests = 0, n_nodes = 0;
        occluded_out[i] = tri_any(T, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), mint, maxt, true, n_tests, n_nodes) ? 1 : 0;
        tests += n_tests; visits += n_nodes;
    }
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->segments = n_rays; stats->quad_tests = tests; stats->node_tests = visits; }
    return RTW_OK;
}

int rtw_mesh_instance_occluded(const RtwTriangle *tris, uint32_t n_tris, const RtwMeshInstance *p, uint32_t n, const float *rays, uint32_t n_rays,
                               float mint, float maxt, uint8_t *occluded_out, RtwStats *stats) {
    if (!rays || !occluded_out || n_rays == 0 || n == 0) return RTW_E_INVALID;
    HostMesh m;
    if (const int rc = host_mesh(tris, n_tris, p, n, m)) return rc;
    try { m.packed = m.top.packed(); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    DevTris T{};                                                   // (the views of rtw_mesh_instance_hits_tree)
    T.list = m.list.data(); T.leaf = m.tree.leaf; T.n = n_tris; T.n_nodes = m.tree.n_nodes;
    T.t_bound = std::fmax(std::fabs(mint), std::fabs(maxt));
    const bool range_ok = std::isfinite(mint) && std::isfinite(maxt) && T.t_bound <= RTW_TRI_COORD_MAX;
    T.nodes = (!m.tree.list_walk && range_ok) ? m.tree.nodes : nullptr;
    const TriNode *top = (T.nodes != nullptr && !m.top.list_walk) ? (const TriNode *)m.packed.data() : nullptr;
    const uint32_t n_top = (uint32_t)m.top.nodes.size();
    unsigned long long tests = 0, visits = 0;
    for (uint32_t i = 0; i < n_rays; i++) {
        const float *r = rays + 6 * (size_t)i;
        uint32_t n_tests = 0, n_nodes = 0;
        occluded_out[i] = mesh_any(T, m.rows.data(), n, top, n_top, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), mint, maxt, true, n_tests, n_nodes) ? 1 : 0;
        tests += n_tests; visits += n_nodes;
    }
    if (stats) { std::memset(stats, 0, sizeof *stats); stats->segments = n_rays; stats->quad_tests = tests; stats->node_tests = visits; }
    return RTW_OK;
}

int rtw_triangle_bvh_validate(const RtwTriangle *tris, uint32_t n, uint32_t *n_nodes, uint32_t *depth, uint32_t *list_walk) {
    if ((n && !tris) || n == 0) return RTW_E_INVALID;
    std::vector<DevTri> list(n);
    tri_prepare(tris, n, list.data());
    TriBuild b;
    if (!tri_build(list.data(), n, b)) return RTW_E_NOMEM;
    std::vector<TriBox> box(n);
    for (uint32_t i = 0; i < n; i++) tri_box(list[i], box[i]);
    std::vector<uint8_t> seen(n, 0);
    uint32_t leaf_slots = 0;
    bool ok = b.n_nodes > 0;
    // every node: a leaf with its triangles inside its box, or an inner node whose children (i + 1 and the left child's skip) lie inside
    // it and end where it says (skip)
    auto inside = [](const TriNode &o, const float *lo, const float *hi) {
        for (int k = 0; k < 3; k++) if (!(o.lo[k] <= lo[k] && hi[k] <= o.hi[k])) return false;
        return true;
    };
    std::vector<uint32_t> todo{ 0 };
    uint32_t visited = 0;
    while (ok && !todo.empty()) {
        const uint32_t i = todo.back(); todo.pop_back();
        if (i >= b.n_nodes || ++visited > b.n_nodes) { ok = false; break; }
        const TriNode &nd = b.nodes[i];
        if (nd.skip <= i || nd.skip > b.n_nodes) { ok = false; break; }
        if (nd.leaf) {
            const uint32_t first = nd.leaf >> 3, cnt = nd.leaf & 7u;
            if (cnt == 0 || cnt > 4 || nd.skip != i + 1 || first + cnt > n) { ok = false; break; }
            for (uint32_t j = first; j < first + cnt; j++) {
                const uint32_t t = b.leaf[j].index;
                if (t >= n || seen[t]) { ok = false; break; }
                seen[t] = 1; leaf_slots++;
                if (std::memcmp(&b.leaf[j], &list[t], sizeof(DevTri)) != 0) { ok = false; break; }
                if (!b.list_walk) {
                    for (int k = 0; k < 3; k++)
                        if (!((double)nd.lo[k] <= box[t].lo[k] && box[t].hi[k] <= (double)nd.hi[k])) ok = false;
                }
            }
        } else {
            const uint32_t l = i + 1;
            if (l >= b.n_nodes) { ok = false; break; }
            const uint32_t r = b.nodes[l].skip;
            if (r >= b.n_nodes || b.nodes[r].skip != nd.skip) { ok = false; break; }
            if (!b.list_walk && (!inside(nd, b.nodes[l].lo, b.nodes[l].hi) || !inside(nd, b.nodes[r].lo, b.nodes[r].hi))) { ok = false; break; }
            todo.push_back(r); todo.push_back(l);
        }
    }
    if (ok && (b.nodes[0].skip != b.n_nodes || leaf_slots != n || visited != b.n_nodes)) ok = false;
    if (n_nodes) *n_nodes = b.n_nodes;
    if (depth) *depth = b.depth;
    if (list_walk) *list_walk = b.list_walk ? 1u : 0u;
    return ok ? RTW_OK : RTW_E_INVALID;
}

// The tree rtw_ctx_set_triangles builds, and its refit, without a context
int rtw_triangle_bvh_dump(const RtwTriangle *tris, uint32_t n, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes, uint32_t *order_out,
                          uint32_t *depth, uint32_t *list_walk) {
    if (!tris || n == 0) return RTW_E_INVALID;
    std::vector<DevTri> list;
    try { list.resize(n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    tri_prepare(tris, n, list.data());
    TriBuild b;
    if (!tri_build(list.data(), n, b)) return RTW_E_NOMEM;
    if (n_nodes) *n_nodes = b.n_nodes;
    if (depth) *depth = b.depth;
    if (list_walk) *list_walk = b.list_walk ? 1u : 0u;
    if (nodes_out) {
        if (node_cap < b.n_nodes) return RTW_E_INVALID;
        std::memcpy(nodes_out, b.nodes, b.n_nodes * sizeof(TriNode));
    }
    if (order_out) for (uint32_t j = 0; j < n; j++) order_out[j] = b.leaf[j].index;
    return RTW_OK;
}

int rtw_triangle_bvh_refit(const RtwTriangle *tris, uint32_t n, const float *ouv, RtwTriNode *nodes_out, uint32_t node_cap, uint32_t *n_nodes,
                           uint32_t *list_walk) {
    if (!tris || n == 0 || !ouv) return RTW_E_INVALID;
    std::vector<DevTri> list;
    try { list.resize(n); } catch (const std::bad_alloc &) { return RTW_E_NOMEM; }
    tri_prepare(tris, n, list.data());
    TriBuild b;
    RefitSchedule s;
    if (!tri_build(list.data(), n, b) || !tri_refit_schedule(b.nodes, b.n_nodes, s)) return RTW_E_NOMEM;
    if (n_nodes) *n_nodes = b.n_nodes;
    if (nodes_out && node_cap < b.n_nodes) return RTW_E_INVALID;
    const uint32_t bad = tri_refit_host(b.nodes, b.leaf, list.data(), ouv, s);
    if (list_walk) *list_walk = bad ? 1u : 0u;
    if (nodes_out) std::memcpy(nodes_out, b.nodes, b.n_nodes * sizeof(TriNode));
    return RTW_OK;
}

} // extern "C"
