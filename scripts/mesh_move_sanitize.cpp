// mesh_move_sanitize.cpp -- a stand-alone driver for the refit of the top-level tree over mesh placements under AddressSanitizer + UBSan (host
// code only, no GPU): rtw_mesh_top_refit -- mesh_pose_rows, placement_box, mesh_top_refit_leaf and refit_inner_node over the tree's height
// schedule, the functions the device runs -- at 1, 5, 1024 and 65 536 placements of an icosphere of 80 triangles, with every motion (turn and
// shift, permute, identity, shrink to a point), with the mesh refitted as well, with invalid poses and with a placement beyond the reach.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc mesh-move-asan
#include "rtw.h"
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

typedef std::array<double, 3> P3;
static P3 unit(P3 a) { const double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); return { a[0] / l, a[1] / l, a[2] / l }; }

// A subdivided icosahedron (20 * 4^level faces), as the Python package's mesh_icosphere
static std::vector<RtwTriangle> icosphere(int level) {
    const double t = (1.0 + std::sqrt(5.0)) / 2.0;
    std::vector<P3> v = { { -1, t, 0 }, { 1, t, 0 }, { -1, -t, 0 }, { 1, -t, 0 }, { 0, -1, t }, { 0, 1, t }, { 0, -1, -t }, { 0, 1, -t },
                          { t, 0, -1 }, { t, 0, 1 }, { -t, 0, -1 }, { -t, 0, 1 } };
    for (P3 &p : v) p = unit(p);
    std::vector<std::array<int, 3>> f = { { 0, 11, 5 }, { 0, 5, 1 }, { 0, 1, 7 }, { 0, 7, 10 }, { 0, 10, 11 }, { 1, 5, 9 }, { 5, 11, 4 }, { 11, 10, 2 },
                                          { 10, 7, 6 }, { 7, 1, 8 }, { 3, 9, 4 }, { 3, 4, 2 }, { 3, 2, 6 }, { 3, 6, 8 }, { 3, 8, 9 }, { 4, 9, 5 },
                                          { 2, 4, 11 }, { 6, 2, 10 }, { 8, 6, 7 }, { 9, 8, 1 } };
    for (int l = 0; l < level; l++) {
        std::map<std::pair<int, int>, int> cache;
        auto mid = [&](int a, int b) {
            const std::pair<int, int> key(a < b ? a : b, a < b ? b : a);
            auto it = cache.find(key);
            if (it != cache.end()) return it->second;
            v.push_back(unit({ v[a][0] + v[b][0], v[a][1] + v[b][1], v[a][2] + v[b][2] }));
            return cache[key] = (int)v.size() - 1;
        };
        std::vector<std::array<int, 3>> nf;
        for (const auto &q : f) {
            const int ab = mid(q[0], q[1]), bc = mid(q[1], q[2]), ca = mid(q[2], q[0]);
            nf.push_back({ q[0], ab, ca }); nf.push_back({ q[1], bc, ab }); nf.push_back({ q[2], ca, bc }); nf.push_back({ ab, bc, ca });
        }
        f = nf;
    }
    std::vector<RtwTriangle> out(f.size());
    for (size_t k = 0; k < f.size(); k++) {
        float o[3], e1[3], e2[3];
        const float col[3] = { 0.7f, 0.6f, 0.5f };
        for (int c = 0; c < 3; c++) {
            o[c] = (float)v[f[k][0]][c];
            e1[c] = (float)v[f[k][1]][c] - o[c]; e2[c] = (float)v[f[k][2]][c] - o[c];
        }
        rtw_triangle_new(o, e1, e2, nullptr, nullptr, col, -1, &out[k]);
    }
    return out;
}

static int failures = 0;
static void expect(const char *what, int got, int want) {
    std::printf("%-72s %d %s\n", what, got, got == want ? "ok" : "FAILED");
    failures += got != want;
}

// splitmix64: the placements and motions are seeded, the same on every run
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}

int main() {
    std::vector<RtwTriangle> tris = icosphere(1);
    const uint32_t nt = (uint32_t)tris.size();
    // the mesh moved as well: every triangle scaled by 1.5 and shifted
    std::vector<float> ouv(9 * (size_t)nt);
    for (uint32_t k = 0; k < nt; k++)
        for (int c = 0; c < 3; c++) {
            ouv[9 * (size_t)k + c] = 1.5f * tris[k].origin[c] + 0.25f; ouv[9 * (size_t)k + 3 + c] = 1.5f * tris[k].u[c]; ouv[9 * (size_t)k + 6 + c] = 1.5f * tris[k].v[c];
        }
    const uint32_t sizes[] = { 1u, 5u, 1024u, 65536u };
    for (uint32_t n : sizes) {
        // a square grid, spacing 3, y jittered, a general un-normalised quaternion each
        const uint32_t g = (uint32_t)std::ceil(std::sqrt((double)n));
        std::vector<RtwMeshInstance> pl(n);
        for (uint32_t k = 0; k < n; k++) {
            pl[k].position[0] = 3.0f * (float)(k % g) - 1.5f * (float)(g - 1); pl[k].position[1] = (float)(1.6 * uniform() - 0.8);
            pl[k].position[2] = 6.0f + 3.0f * (float)(k / g) - 1.5f * (float)(g - 1);
            for (int c = 0; c < 4; c++) pl[k].quat[c] = (float)(4.0 * uniform() - 2.0) + (c == 0 ? 0.25f : 0.0f);
        }
        std::vector<float> same(7 * (size_t)n);
        std::memcpy(same.data(), pl.data(), same.size() * sizeof(float));
        std::vector<RtwTriNode> built(2 * (size_t)n), nodes(2 * (size_t)n), again(2 * (size_t)n);
        std::vector<float> rows(8 * (size_t)n), rows2(8 * (size_t)n);
        uint32_t n_built = 0, n_nodes = 0, list_walk = 9, invalid = 9;
        char what[128];
        std::snprintf(what, sizeof what, "n = %u: dump", n);
        expect(what, rtw_mesh_top_dump(tris.data(), nt, pl.data(), n, built.data(), 2 * n, &n_built, nullptr, nullptr, nullptr), RTW_OK);
        // the motions
        const char *names[] = { "identity", "turn and shift", "permute", "shrink to a point" };
        for (int m = 0; m < 4; m++) {
            std::vector<float> moved = same;
            for (uint32_t k = 0; k < n; k++) {
                float *p = &moved[7 * (size_t)k];
                if (m == 1) {
                    for (int c = 0; c < 3; c++) p[c] += (float)(2.0 * uniform() - 1.0);
                    for (int c = 0; c < 4; c++) p[3 + c] = (float)(4.0 * uniform() - 2.0) + (c == 1 ? 0.25f : 0.0f);
                } else if (m == 2) {
                    const uint32_t j = (uint32_t)(uniform() * n) % n;
                    for (int c = 0; c < 7; c++) std::swap(p[c], moved[7 * (size_t)j + c]);
                } else if (m == 3) {
                    for (int c = 0; c < 3; c++) p[c] = same[c];
                }
            }
            list_walk = invalid = 9;
            std::snprintf(what, sizeof what, "  %s: refit", names[m]);
            expect(what, rtw_mesh_top_refit(tris.data(), nt, pl.data(), n, moved.data(), nullptr, nodes.data(), 2 * n, &n_nodes, rows.data(), &list_walk, &invalid), RTW_OK);
            expect("    node count, list_walk, invalid", (int)(n_nodes != n_built) + (int)list_walk + (int)invalid, 0);
            int bad = 0;
            for (uint32_t i = 0; i < n_nodes; i++) {
                if (nodes[i].skip != built[i].skip || nodes[i].leaf != built[i].leaf) bad++;
                if (!nodes[i].leaf) {                                            // an inner node holds both children
                    const RtwTriNode &l = nodes[i + 1], &r = nodes[nodes[i + 1].skip];
                    for (int c = 0; c < 3; c++) if (!(nodes[i].lo[c] <= l.lo[c] && nodes[i].lo[c] <= r.lo[c] && nodes[i].hi[c] >= l.hi[c] && nodes[i].hi[c] >= r.hi[c])) bad++;
                }
            }
            expect("    topology kept, every inner box holds its children", bad, 0);
            if (m == 0) expect("    the same poses: the builder's bytes", std::memcmp(nodes.data(), built.data(), n_nodes * sizeof(RtwTriNode)) != 0, 0);
            // ... with the mesh refitted as well, and the mesh alone
            expect("    with ouv", rtw_mesh_top_refit(tris.data(), nt, pl.data(), n, moved.data(), ouv.data(), again.data(), 2 * n, nullptr, rows2.data(), &list_walk, &invalid), RTW_OK);
            expect("    ... list_walk, invalid, the same rows", (int)list_walk + (int)invalid + (std::memcmp(rows.data(), rows2.data(), rows.size() * sizeof(float)) != 0), 0);
            if (m == 0) expect("    ouv alone", rtw_mesh_top_refit(tris.data(), nt, pl.data(), n, nullptr, ouv.data(), again.data(), 2 * n, nullptr, nullptr, nullptr, nullptr), RTW_OK);
        }
        // invalid poses at the first, the middle and the last index: their rows stay, the count is right
        {
            std::vector<float> moved = same;
            for (uint32_t k = 0; k < n; k++) moved[7 * (size_t)k + 1] += 0.5f;
            const uint32_t where[3] = { 0u, n / 2, n - 1u };
            uint32_t distinct = 0;
            for (int j = 0; j < 3; j++) {
                bool fresh = true;
                for (int i = 0; i < j; i++) if (where[i] == where[j]) fresh = false;
                distinct += fresh;
                float *p = &moved[7 * (size_t)where[j]];
                if (j == 0) p[1] = NAN;
                else if (j == 1) p[5] = INFINITY;
                else for (int c = 3; c < 7; c++) p[c] = 0.0f;
            }
            expect("  invalid poses: refit", rtw_mesh_top_refit(tris.data(), nt, pl.data(), n, moved.data(), nullptr, nodes.data(), 2 * n, nullptr, rows.data(), &list_walk, &invalid), RTW_OK);
            expect("    counted", (int)invalid, (int)distinct);
            rtw_mesh_top_refit(tris.data(), nt, pl.data(), n, nullptr, nullptr, again.data(), 2 * n, nullptr, rows2.data(), nullptr, nullptr);
            int bad = 0;
            for (int j = 0; j < 3; j++) bad += std::memcmp(&rows[8 * (size_t)where[j]], &rows2[8 * (size_t)where[j]], 8 * sizeof(float)) != 0;
            expect("    their rows stay", bad, 0);
        }
        // a placement beyond the reach, and back
        {
            std::vector<float> moved = same;
            moved[7 * (size_t)(n / 2)] = 0x1p39f;
            expect("  a position of 2^39: refit", rtw_mesh_top_refit(tris.data(), nt, pl.data(), n, moved.data(), nullptr, nodes.data(), 2 * n, nullptr, nullptr, &list_walk, &invalid), RTW_OK);
            expect("    list_walk bit 1", (int)list_walk, 2);
            std::vector<RtwMeshInstance> far(n);
            std::memcpy(far.data(), moved.data(), moved.size() * sizeof(float));
            expect("  ... and back from a list built beyond the reach", rtw_mesh_top_refit(tris.data(), nt, far.data(), n, same.data(), nullptr, nodes.data(), 2 * n, nullptr, nullptr, &list_walk, &invalid), RTW_OK);
            expect("    list_walk", (int)list_walk, 0);
        }
        expect("  too small a node buffer is refused", rtw_mesh_top_refit(tris.data(), nt, pl.data(), n, same.data(), nullptr, nodes.data(), n_built - 1, nullptr, nullptr, nullptr, nullptr), RTW_E_INVALID);
    }
    expect("no placements", rtw_mesh_top_refit(tris.data(), nt, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr), RTW_E_INVALID);
    expect("no triangles", rtw_mesh_top_refit(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr), RTW_E_INVALID);
    std::printf("%s\n", failures ? "FAILED" : "all ok");
    return failures ? 1 : 0;
}
