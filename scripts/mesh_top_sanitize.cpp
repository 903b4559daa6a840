// mesh_top_sanitize.cpp -- a stand-alone driver for the top-level tree over mesh placements under AddressSanitizer + UBSan (host code only, no
// GPU): the builder and rtw_mesh_top_dump, and both host walks -- rtw_mesh_instance_hits (list order) and rtw_mesh_instance_hits_tree (the
// kernels' walk, compiled for the host) -- at 1, 5, 1024 and 65 536 placements of an icosphere of 80 triangles; the two walks must agree on
// the bits.  Prints the builder's time at each size.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc mesh-top-asan
#include "rtw.h"
#include <array>
#include <chrono>
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
    std::printf("%-58s %d %s\n", what, got, got == want ? "ok" : "FAILED");
    failures += got != want;
}

// splitmix64: the placements and rays are seeded, the same on every run
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}

int main() {
    std::vector<RtwTriangle> tris = icosphere(1);
    const uint32_t nt = (uint32_t)tris.size();
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
        // rays aimed at placements, plus a NaN ray, a zero direction and an origin beyond the reach
        const uint32_t nr = n > 1024u ? 64u : 512u;
        std::vector<float> rays(6 * (size_t)nr);
        for (uint32_t i = 0; i < nr; i++) {
            const RtwMeshInstance &p = pl[(size_t)(uniform() * n) % n];
            float *r = &rays[6 * (size_t)i];
            const double o[3] = { p.position[0] + 40.0 * (uniform() - 0.5), 12.0 + 6.0 * uniform(), p.position[2] + 40.0 * (uniform() - 0.5) };
            for (int c = 0; c < 3; c++) { r[c] = (float)o[c]; r[3 + c] = (float)(p.position[c] + 0.8 * (uniform() - 0.5) - o[c]); }
        }
        rays[3] = NAN;
        for (int c = 0; c < 3; c++) rays[6 + 3 + c] = 0.0f;
        rays[12] = 0x1p39f;
        std::vector<RtwTriNode> nodes(2 * (size_t)n);
        std::vector<uint32_t> order(n);
        uint32_t n_nodes = 0, depth = 0, list_walk = 9;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = rtw_mesh_top_dump(tris.data(), nt, pl.data(), n, nodes.data(), 2 * n, &n_nodes, order.data(), &depth, &list_walk);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        char what[96];
        std::snprintf(what, sizeof what, "n = %u: dump (%u nodes, depth %u, %.1f ms with both builds)", n, n_nodes, depth, ms);
        expect(what, rc, RTW_OK);
        expect("  list_walk", (int)list_walk, 0);
        std::vector<uint8_t> seen(n, 0);
        int bad = 0;
        for (uint32_t i = 0; i < n; i++) { if (order[i] >= n || seen[order[i]]) bad++; else seen[order[i]] = 1; }
        for (uint32_t i = 0; i < n_nodes; i++) if (nodes[i].skip <= i || nodes[i].skip > n_nodes) bad++;
        expect("  order is a permutation, skip links increase", bad, 0);
        expect("  too small a node buffer is refused", rtw_mesh_top_dump(tris.data(), nt, pl.data(), n, nodes.data(), n_nodes - 1, nullptr, nullptr, nullptr, nullptr), RTW_E_INVALID);
        expect("  sizes alone", rtw_mesh_top_dump(tris.data(), nt, pl.data(), n, nullptr, 0, &n_nodes, nullptr, nullptr, nullptr), RTW_OK);
        std::vector<float> t0v(nr), t1v(nr), n0(3 * (size_t)nr), n1(3 * (size_t)nr);
        std::vector<int32_t> p0(nr), p1(nr), i0(nr), i1(nr);
        RtwStats st;
        expect("  list walk", rtw_mesh_instance_hits(tris.data(), nt, pl.data(), n, rays.data(), nr, 1e-4f, 1e4f, t0v.data(), p0.data(), i0.data(), n0.data()), RTW_OK);
        expect("  tree walk", rtw_mesh_instance_hits_tree(tris.data(), nt, pl.data(), n, rays.data(), nr, 1e-4f, 1e4f, t1v.data(), p1.data(), i1.data(), n1.data(), &st), RTW_OK);
        int differ = 0, hits = 0;
        for (uint32_t i = 0; i < nr; i++) {
            const bool both_nan = t0v[i] != t0v[i] && t1v[i] != t1v[i];
            if (!both_nan && std::memcmp(&t0v[i], &t1v[i], 4) != 0) differ++;
            if (p0[i] != p1[i] || i0[i] != i1[i]) differ++;
            if (!both_nan && std::memcmp(&n0[3 * (size_t)i], &n1[3 * (size_t)i], 12) != 0) differ++;
            hits += p0[i] >= 0;
        }
        std::snprintf(what, sizeof what, "  tree == list on %u rays (%d hit; %.1f node visits per ray)", nr, hits, (double)st.node_tests / nr);
        expect(what, differ, 0);
        expect("  tree walk without normals or stats", rtw_mesh_instance_hits_tree(tris.data(), nt, pl.data(), n, rays.data(), nr, 1e-4f, 1e4f, t1v.data(), p1.data(), i1.data(), nullptr, nullptr), RTW_OK);
        // a placement beyond the reach: the context's list walk, the same bits
        if (n >= 5u) {
            pl[n / 2].position[0] = 1e30f;
            expect("  a placement at 1e30: dump", rtw_mesh_top_dump(tris.data(), nt, pl.data(), n, nullptr, 0, nullptr, nullptr, nullptr, &list_walk), RTW_OK);
            expect("  ... sets list_walk", (int)list_walk, 1);
            if (n <= 1024u) {
                rtw_mesh_instance_hits(tris.data(), nt, pl.data(), n, rays.data(), 16, 1e-4f, 1e4f, t0v.data(), p0.data(), i0.data(), nullptr);
                rtw_mesh_instance_hits_tree(tris.data(), nt, pl.data(), n, rays.data(), 16, 1e-4f, 1e4f, t1v.data(), p1.data(), i1.data(), nullptr, &st);
                differ = 0;
                for (uint32_t i = 0; i < 16; i++) if (p0[i] != p1[i] || i0[i] != i1[i]) differ++;
                expect("  ... and the walks agree", differ, 0);
            }
        }
    }
    expect("no placements", rtw_mesh_top_dump(tris.data(), nt, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr), RTW_E_INVALID);
    std::printf("%s\n", failures ? "FAILED" : "all ok");
    return failures ? 1 : 0;
}
