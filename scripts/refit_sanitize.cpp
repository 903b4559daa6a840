// refit_sanitize.cpp -- a stand-alone driver for the host side of the triangle tree's refit under AddressSanitizer + UBSan (host code only, no
// GPU): rtw_triangle_bvh_dump and rtw_triangle_bvh_refit -- the functions and the schedule the device runs, compiled for the host -- on the
// meshes of tests/refit_common.py and on a terrain of 65 536 triangles.  A refit to the same vertices must return the builder's bytes; a
// refit to moved vertices must keep the topology and bound every triangle; a degenerate triangle must set list_walk.
//
// And the shared roundings against the library forms they replaced in the builder: box_down / box_up against (float)x stepped by
// std::nextafter, box_min / box_max against std::min / std::max, over 2 x 10^7 doubles (random bit patterns, random numbers of every f32
// exponent and beyond both ends) and the edges: zeros, the denormal range, FLT_MAX, the infinities.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc refit-asan
#include "rtw.h"
#include "rtw_refit.h"                     // box_down / box_up / box_min / box_max: the shared definitions themselves
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

typedef std::array<double, 3> P3;
struct Mesh { std::vector<P3> v; std::vector<std::array<int, 3>> f; };
static P3 unit(P3 a) { const double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); return { a[0] / l, a[1] / l, a[2] / l }; }

// A subdivided icosahedron (20 * 4^level faces), as the Python package's mesh_icosphere
static Mesh icosphere(int level) {
    const double t = (1.0 + std::sqrt(5.0)) / 2.0;
    Mesh m;
    m.v = { { -1, t, 0 }, { 1, t, 0 }, { -1, -t, 0 }, { 1, -t, 0 }, { 0, -1, t }, { 0, 1, t }, { 0, -1, -t }, { 0, 1, -t },
            { t, 0, -1 }, { t, 0, 1 }, { -t, 0, -1 }, { -t, 0, 1 } };
    for (P3 &p : m.v) p = unit(p);
    m.f = { { 0, 11, 5 }, { 0, 5, 1 }, { 0, 1, 7 }, { 0, 7, 10 }, { 0, 10, 11 }, { 1, 5, 9 }, { 5, 11, 4 }, { 11, 10, 2 },
            { 10, 7, 6 }, { 7, 1, 8 }, { 3, 9, 4 }, { 3, 4, 2 }, { 3, 2, 6 }, { 3, 6, 8 }, { 3, 8, 9 }, { 4, 9, 5 },
            { 2, 4, 11 }, { 6, 2, 10 }, { 8, 6, 7 }, { 9, 8, 1 } };
    for (int l = 0; l < level; l++) {
        std::map<std::pair<int, int>, int> cache;
        auto mid = [&](int a, int b) {
            const std::pair<int, int> key(a < b ? a : b, a < b ? b : a);
            auto it = cache.find(key);
            if (it != cache.end()) return it->second;
            m.v.push_back(unit({ m.v[a][0] + m.v[b][0], m.v[a][1] + m.v[b][1], m.v[a][2] + m.v[b][2] }));
            return cache[key] = (int)m.v.size() - 1;
        };
        std::vector<std::array<int, 3>> nf;
        for (const auto &q : m.f) {
            const int ab = mid(q[0], q[1]), bc = mid(q[1], q[2]), ca = mid(q[2], q[0]);
            nf.push_back({ q[0], ab, ca }); nf.push_back({ q[1], bc, ab }); nf.push_back({ q[2], ca, bc }); nf.push_back({ ab, bc, ca });
        }
        m.f = nf;
    }
    return m;
}
// A height field over an nx x nz grid (2 nx nz faces)
static Mesh terrain(int nx, int nz) {
    Mesh m;
    for (int j = 0; j <= nz; j++) for (int i = 0; i <= nx; i++) {
        const double x = 20.0 * i / nx - 10.0, z = 20.0 * j / nz - 10.0;
        m.v.push_back({ x, 0.5 * std::sin(0.7 * x) * std::cos(0.5 * z) + 0.3 * std::sin(0.23 * x + 0.31 * z), z });
    }
    for (int j = 0; j < nz; j++) for (int i = 0; i < nx; i++) {
        const int a = j * (nx + 1) + i;
        m.f.push_back({ a, a + nx + 1, a + 1 }); m.f.push_back({ a + 1, a + nx + 1, a + nx + 2 });
    }
    return m;
}
static Mesh row(int k) {
    Mesh m;
    for (int i = 0; i < k; i++) {
        m.v.push_back({ 2.0 * i, 0, 0 }); m.v.push_back({ 2.0 * i + 1, 0, 0 }); m.v.push_back({ 2.0 * i, 1, 0.5 });
        m.f.push_back({ 3 * i, 3 * i + 1, 3 * i + 2 });
    }
    return m;
}
static Mesh coincident(int k) {
    Mesh m;
    m.v = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0.25 } };
    for (int i = 0; i < k; i++) m.f.push_back({ 0, 1, 2 });
    return m;
}
static Mesh uneven(int k) {
    Mesh m;
    for (int j = 0; j < k; j++) {
        const double x = std::pow(1.6, j);
        m.v.push_back({ x, 0, 0 }); m.v.push_back({ 1.1 * x, 0, 0 }); m.v.push_back({ x, 0.1 * x, 0 });
        m.f.push_back({ 3 * j, 3 * j + 1, 3 * j + 2 });
    }
    return m;
}
// v A^T + (5, -2, 1), then y += 0.3 sin(4 x): the first deformation of the tests
static Mesh sine_wave(const Mesh &m) {
    Mesh o = m;
    for (P3 &p : o.v) {
        const P3 q = { 3.0 * p[0] + 0.5 * p[1] + 5.0, p[1] + 0.25 * p[2] - 2.0, 0.5 * p[2] + 1.0 };
        p = { q[0], q[1] + 0.3 * std::sin(4.0 * q[0]), q[2] };
    }
    return o;
}

// origin, u, v in f32 (Triangle.from_mesh's arithmetic)
static std::vector<float> ouv_of(const Mesh &m) {
    std::vector<float> out(9 * m.f.size());
    for (size_t k = 0; k < m.f.size(); k++)
        for (int c = 0; c < 3; c++) {
            const float o = (float)m.v[m.f[k][0]][c];
            out[9 * k + c] = o; out[9 * k + 3 + c] = (float)m.v[m.f[k][1]][c] - o; out[9 * k + 6 + c] = (float)m.v[m.f[k][2]][c] - o;
        }
    return out;
}
static std::vector<RtwTriangle> triangles_of(const std::vector<float> &ouv) {
    std::vector<RtwTriangle> out(ouv.size() / 9);
    const float col[3] = { 0.7f, 0.6f, 0.5f };
    for (size_t k = 0; k < out.size(); k++) rtw_triangle_new(&ouv[9 * k], &ouv[9 * k + 3], &ouv[9 * k + 6], nullptr, nullptr, col, -1, &out[k]);
    return out;
}

static int failures = 0;
static void expect(const char *what, long got, long want) {
    std::printf("%-74s %ld %s\n", what, got, got == want ? "ok" : "FAILED");
    failures += got != want;
}

static void run(const char *name, const Mesh &m) {
    const std::vector<float> ouv = ouv_of(m), moved = ouv_of(sine_wave(m));
    const std::vector<RtwTriangle> tris = triangles_of(ouv);
    const uint32_t n = (uint32_t)tris.size();
    std::vector<RtwTriNode> built(2 * (size_t)n), same(2 * (size_t)n), refit(2 * (size_t)n);
    std::vector<uint32_t> order(n);
    uint32_t n_nodes = 0, depth = 0, walk = 9, nn = 0;
    char what[128];
    auto t0 = std::chrono::steady_clock::now();
    int rc = rtw_triangle_bvh_dump(tris.data(), n, built.data(), 2 * n, &n_nodes, order.data(), &depth, &walk);
    const double ms_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::snprintf(what, sizeof what, "%s: %u triangles, dump (%u nodes, depth %u, %.1f ms)", name, n, n_nodes, depth, ms_build);
    expect(what, rc, RTW_OK);
    expect("  list_walk", walk, 0);
    std::vector<uint8_t> seen(n, 0);
    long bad = 0;
    for (uint32_t i = 0; i < n; i++) { if (order[i] >= n || seen[order[i]]) bad++; else seen[order[i]] = 1; }
    for (uint32_t i = 0; i < n_nodes; i++) if (built[i].skip <= i || built[i].skip > n_nodes) bad++;
    expect("  order is a permutation, skip links increase", bad, 0);
    expect("  too small a node buffer is refused (dump)", rtw_triangle_bvh_dump(tris.data(), n, built.data(), n_nodes - 1, nullptr, nullptr, nullptr, nullptr), RTW_E_INVALID);
    expect("  too small a node buffer is refused (refit)", rtw_triangle_bvh_refit(tris.data(), n, ouv.data(), same.data(), n_nodes - 1, nullptr, nullptr), RTW_E_INVALID);
    expect("  sizes alone", rtw_triangle_bvh_refit(tris.data(), n, ouv.data(), nullptr, 0, &nn, nullptr) == RTW_OK && nn == n_nodes, 1);
    // the same vertices: the builder's bytes
    t0 = std::chrono::steady_clock::now();
    rc = rtw_triangle_bvh_refit(tris.data(), n, ouv.data(), same.data(), 2 * n, &nn, &walk);
    const double ms_both = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::snprintf(what, sizeof what, "  refit to the same vertices (%.1f ms with the build)", ms_both);
    expect(what, rc, RTW_OK);
    expect("  ... returns the builder's bytes", nn == n_nodes && walk == 0 && std::memcmp(same.data(), built.data(), n_nodes * sizeof(RtwTriNode)) == 0, 1);
    // moved vertices: the topology stays, every triangle and every child lies inside
    expect("  refit to the sine wave", rtw_triangle_bvh_refit(tris.data(), n, moved.data(), refit.data(), 2 * n, &nn, &walk), RTW_OK);
    expect("  list_walk", walk, 0);
    bad = 0;
    for (uint32_t i = 0; i < n_nodes; i++) {
        const RtwTriNode &nd = refit[i];
        if (nd.skip != built[i].skip || nd.leaf != built[i].leaf) { bad++; continue; }
        if (nd.leaf) {
            for (uint32_t j = nd.leaf >> 3; j < (nd.leaf >> 3) + (nd.leaf & 7u); j++) {
                const float *s = &moved[9 * (size_t)order[j]];
                for (int c = 0; c < 3; c++) {
                    const double a = s[c], p = a + (double)s[3 + c], q = a + (double)s[6 + c];
                    if (!(nd.lo[c] < std::fmin(a, std::fmin(p, q)) && std::fmax(a, std::fmax(p, q)) < nd.hi[c])) bad++;
                }
            }
        } else {
            const RtwTriNode &l = refit[i + 1], &r = refit[l.skip];
            for (int c = 0; c < 3; c++) if (!(nd.lo[c] <= l.lo[c] && nd.lo[c] <= r.lo[c] && l.hi[c] <= nd.hi[c] && r.hi[c] <= nd.hi[c])) bad++;
        }
    }
    expect("  topology kept, triangles and children inside their boxes", bad, 0);
    // a degenerate triangle among the moved ones (u == v): the list must answer
    if (n >= 2) {
        std::vector<float> deg = moved;
        for (int c = 0; c < 3; c++) deg[9 * (size_t)(n / 2) + 6 + c] = deg[9 * (size_t)(n / 2) + 3 + c];
        expect("  a degenerate triangle: refit", rtw_triangle_bvh_refit(tris.data(), n, deg.data(), refit.data(), 2 * n, nullptr, &walk), RTW_OK);
        expect("  ... sets list_walk", walk, 1);
    }
}

// The roundings as the builder had them before they moved to rtw_refit.h
static float old_down(double x) { float f = (float)x; if ((double)f > x) f = std::nextafter(f, -INFINITY); return f; }
static float old_up(double x) { float f = (float)x; if ((double)f < x) f = std::nextafter(f, INFINITY); return f; }
static uint64_t sweep_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64() {
    uint64_t z = (sweep_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
static void sweep() {
    long differ = 0, checked = 0;
    double prev = 1.0;
    auto check = [&](double x) {
        const float a = old_down(x), b = rtw::box_down(x), c = old_up(x), d = rtw::box_up(x);
        const bool nan = x != x;
        if (nan ? !(b != b && d != d) : (std::memcmp(&a, &b, 4) != 0 || std::memcmp(&c, &d, 4) != 0)) differ++;
        if (!nan && prev == prev) {
            const double m0 = std::min(prev, x), m1 = rtw::box_min(prev, x), M0 = std::max(prev, x), M1 = rtw::box_max(prev, x);
            if (std::memcmp(&m0, &m1, 8) != 0 || std::memcmp(&M0, &M1, 8) != 0) differ++;
        }
        prev = x; checked++;
    };
    const double edges[] = { 0.0, -0.0, 1e-50, -1e-50, 1e-46, -1e-46, 0x1p-149, -0x1p-149, 0x1.8p-149, -0x1.8p-149, 0x1p-150, -0x1p-150, 0x1p-126, -0x1p-126,
                             3.5e38, -3.5e38, 3.4028234663852886e38, -3.4028234663852886e38, 0x1.fffffe0000001p127, -0x1.fffffe0000001p127,
                             0x1.ffffffp127, 1e300, -1e300, INFINITY, -INFINITY, NAN, 1.0, -1.0, 1.0 + 1e-12, 1.0 - 1e-12, -1.0 - 1e-12, -1.0 + 1e-12 };
    for (double x : edges) check(x);
    for (int i = 0; i < 10000000; i++) { const uint64_t b = next64(); double x; std::memcpy(&x, &b, 8); check(x); }
    for (int i = 0; i < 10000000; i++) {
        const double m = (double)(next64() >> 11) * 0x1p-53 + 0.5;
        check(std::ldexp((next64() & 1) ? m : -m, (int)(next64() % 340) - 190));          // 2^-191 .. 2^149: past both ends of f32
    }
    char what[96];
    std::snprintf(what, sizeof what, "roundings and selections against the library forms, %ld doubles: differing", checked);
    expect(what, differ, 0);
}

int main() {
    sweep();
    run("row of 1", row(1));
    run("row of 4", row(4));
    run("row of 5", row(5));
    run("icosphere(1)", icosphere(1));
    run("icosphere(2)", icosphere(2));
    run("terrain 12 x 12", terrain(12, 12));
    run("33 coincident", coincident(33));
    run("40 at 1.6^k", uneven(40));
    run("terrain 256 x 128", terrain(256, 128));
    const Mesh m = row(2);
    const std::vector<float> ouv = ouv_of(m);
    const std::vector<RtwTriangle> tris = triangles_of(ouv);
    expect("no triangles (dump)", rtw_triangle_bvh_dump(tris.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr), RTW_E_INVALID);
    expect("no triangles (refit)", rtw_triangle_bvh_refit(nullptr, 2, ouv.data(), nullptr, 0, nullptr, nullptr), RTW_E_INVALID);
    expect("no vertices (refit)", rtw_triangle_bvh_refit(tris.data(), 2, nullptr, nullptr, 0, nullptr, nullptr), RTW_E_INVALID);
    std::printf("%s\n", failures ? "FAILED" : "all ok");
    return failures ? 1 : 0;
}
