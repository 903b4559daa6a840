// mesh_instances_sanitize.cpp -- a stand-alone driver for the host side of mesh placements under AddressSanitizer + UBSan (host code only,
// no GPU): rtw_mesh_instances_validate and rtw_mesh_instance_hits on the inputs of tests/test_mesh_instances_cpu.py -- an icosphere of 80
// triangles, the six standard placements, rays aimed, missing, from inside, with zero components, NaN and a zero direction.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc mesh-asan
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
    std::printf("%-58s %d %s\n", what, got, got == want ? "ok" : "FAILED");
    failures += got != want;
}

int main() {
    std::vector<RtwTriangle> tris = icosphere(1);
    const float s = std::sin(0.39269908f), c = std::cos(0.39269908f);
    std::vector<RtwMeshInstance> pl = {
        { { 0.0f, 0.0f, 0.0f }, { 1.0f, 0.0f, 0.0f, 0.0f } }, { { 3.0f, 0.0f, 0.5f }, { 1.0f, 0.0f, 0.0f, 0.0f } },
        { { 0.4f, 0.3f, 3.2f }, { c, 0.0f, s, 0.0f } },       { { -3.0f, 0.5f, 1.0f }, { 0.6f, 0.2f, -1.4f, 0.9f } },
        { { 1.1f, 0.5f, 2.9f }, { 1.0f, 0.0f, 0.0f, 0.0f } }, { { 1.1f, 0.5f, 2.9f }, { 1.0f, 0.0f, 0.0f, 0.0f } } };
    const uint32_t nt = (uint32_t)tris.size(), np = (uint32_t)pl.size();
    // ---- every status of the validation ----
    expect("the standard placements", rtw_mesh_instances_validate(tris.data(), nt, pl.data(), np), RTW_OK);
    expect("NULL / 0 clears", rtw_mesh_instances_validate(tris.data(), nt, nullptr, 0), RTW_OK);
    expect("no triangles", rtw_mesh_instances_validate(nullptr, 0, pl.data(), np), RTW_E_NO_SCENE);
    expect("NULL triangles with a count", rtw_mesh_instances_validate(nullptr, nt, pl.data(), np), RTW_E_INVALID);
    expect("NULL placements with a count", rtw_mesh_instances_validate(tris.data(), nt, nullptr, 3), RTW_E_INVALID);
    expect("placements with a count of 0", rtw_mesh_instances_validate(tris.data(), nt, pl.data(), 0), RTW_E_INVALID);
    {
        std::vector<RtwMeshInstance> big(RTW_MAX_MESH_INSTANCES + 1u, pl[0]);
        expect("RTW_MAX_MESH_INSTANCES", rtw_mesh_instances_validate(tris.data(), nt, big.data(), RTW_MAX_MESH_INSTANCES), RTW_OK);
        expect("RTW_MAX_MESH_INSTANCES + 1", rtw_mesh_instances_validate(tris.data(), nt, big.data(), RTW_MAX_MESH_INSTANCES + 1u), RTW_E_INVALID);
    }
    for (float bad : { NAN, INFINITY, -INFINITY }) {
        std::vector<RtwMeshInstance> q = pl;
        q[5].position[1] = bad;
        expect("a position that is not finite", rtw_mesh_instances_validate(tris.data(), nt, q.data(), np), RTW_E_INVALID);
        q = pl; q[3].quat[2] = bad;
        expect("a quaternion that is not finite", rtw_mesh_instances_validate(tris.data(), nt, q.data(), np), RTW_E_INVALID);
    }
    {
        std::vector<RtwMeshInstance> q = pl;
        std::memset(q[2].quat, 0, sizeof q[2].quat);
        expect("len == 0", rtw_mesh_instances_validate(tris.data(), nt, q.data(), np), RTW_E_INVALID);
        q[2].quat[0] = q[2].quat[1] = 3e38f;
        expect("len overflows", rtw_mesh_instances_validate(tris.data(), nt, q.data(), np), RTW_E_INVALID);
        std::vector<RtwTriangle> tx = tris;
        tx[nt - 1].tex = 0;
        expect("a textured triangle", rtw_mesh_instances_validate(tx.data(), nt, pl.data(), np), RTW_E_INVALID);
    }
    // ---- the list walk: 4096 rays of every kind, with and without normals; the outputs' own invariants ----
    const uint32_t n = 4096;
    std::vector<float> rays(6 * (size_t)n);
    uint32_t x = 2463534242u;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (float)(x >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    for (uint32_t k = 0; k < n; k++) {
        float *r = &rays[6 * (size_t)k];
        const RtwMeshInstance &p = pl[k % np];
        const uint32_t kind = (k / np) % 4;
        if (kind == 0) { for (int a = 0; a < 3; a++) { r[a] = p.position[a] + 8.0f * rnd(); r[3 + a] = p.position[a] + 0.4f * rnd() - r[a]; } }
        else if (kind == 1) { for (int a = 0; a < 3; a++) { r[a] = p.position[a] + 0.5f * rnd(); r[3 + a] = 6.0f + rnd(); } r[1] += 6.0f; }
        else if (kind == 2) { for (int a = 0; a < 3; a++) { r[a] = p.position[a] + 0.3f * rnd(); r[3 + a] = rnd(); } }
        else { for (int a = 0; a < 3; a++) { r[a] = p.position[a] + 0.6f * rnd(); r[3 + a] = 0.0f; } r[3 + k % 3] = 1.5f; r[k % 3] -= 6.0f; }
    }
    const float nan_ray[6] = { 0, 0, -5, NAN, 0, 1 }, zero_ray[6] = { 0, 0, -5, 0, 0, 0 };
    std::memcpy(&rays[6 * (size_t)(n - 2)], nan_ray, sizeof nan_ray);
    std::memcpy(&rays[6 * (size_t)(n - 1)], zero_ray, sizeof zero_ray);
    std::vector<float> t(n), t2(n), nrm(3 * (size_t)n);
    std::vector<int32_t> pi(n), ti(n), pi2(n), ti2(n);
    expect("rtw_mesh_instance_hits", rtw_mesh_instance_hits(tris.data(), nt, pl.data(), np, rays.data(), n, 1e-4f, 1e4f, t.data(), pi.data(), ti.data(), nrm.data()), RTW_OK);
    expect("... without normals", rtw_mesh_instance_hits(tris.data(), nt, pl.data(), np, rays.data(), n, 1e-4f, 1e4f, t2.data(), pi2.data(), ti2.data(), nullptr), RTW_OK);
    uint32_t hits = 0, bad = 0, later = 0;
    for (uint32_t k = 0; k < n; k++) {
        const bool hit = pi[k] >= 0;
        hits += hit;
        later += pi[k] == 5;
        bad += hit ? !(pi[k] < (int32_t)np && ti[k] >= 0 && ti[k] < (int32_t)nt) : !(ti[k] == -1 && std::isinf(t[k]) && nrm[3 * k] == 0.0f);
        bad += pi[k] != pi2[k] || ti[k] != ti2[k] || std::memcmp(&t[k], &t2[k], sizeof(float)) != 0;
    }
    expect("inconsistent outputs", (int)bad, 0);
    expect("the later of the coincident pair wins", (int)later, 0);
    expect("hits between a quarter and three quarters", hits >= n / 4 && hits <= 3 * n / 4, 1);
    expect("the NaN ray is the first placement's first triangle", pi[n - 2] == 0 && ti[n - 2] == 0 && std::isnan(t[n - 2]), 1);
    expect("the zero direction misses", pi[n - 1], -1);
    expect("no rays", rtw_mesh_instance_hits(tris.data(), nt, pl.data(), np, rays.data(), 0, 1e-4f, 1e4f, t.data(), pi.data(), ti.data(), nullptr), RTW_E_INVALID);
    expect("no placements", rtw_mesh_instance_hits(tris.data(), nt, nullptr, 0, rays.data(), n, 1e-4f, 1e4f, t.data(), pi.data(), ti.data(), nullptr), RTW_E_INVALID);
    // the identity placement alone is the triangle group
    std::vector<int32_t> ti0(n);
    std::vector<float> t0(n);
    rtw_triangle_hits(tris.data(), nt, rays.data(), n, 1e-4f, 1e4f, t0.data(), ti0.data());
    rtw_mesh_instance_hits(tris.data(), nt, pl.data(), 1, rays.data(), n, 1e-4f, 1e4f, t.data(), pi.data(), ti.data(), nullptr);
    uint32_t differ = 0;
    for (uint32_t k = 0; k + 2 < n; k++) {
        bool zero = false;
        for (int a = 0; a < 6; a++) zero |= rays[6 * (size_t)k + a] == 0.0f;
        if (!zero) differ += ti[k] != ti0[k] || std::memcmp(&t[k], &t0[k], sizeof(float)) != 0;
    }
    expect("identity placement against rtw_triangle_hits", (int)differ, 0);
    std::printf(failures ? "%d FAILED\n" : "all ok\n", failures);
    return failures != 0;
}
