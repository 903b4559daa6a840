// bvh_builder_sanitize.cpp -- a stand-alone driver for the sphere-BVH builder under AddressSanitizer + UBSan (host code only, no GPU):
// builds the scenes of tests/test_bvh_builder_cpu.py, runs the library's own self-check on each tree and a few host queries over it.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc builder-asan
#include "rtw_host.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
using namespace rtw;

static RtwSphere sph(float x, float y, float z, float r, float vy = 0.0f) {
    RtwSphere s; const float o[3] = { x, y, z }, v[3] = { 0, vy, 0 };
    rtw_sphere_new(o, r, nullptr, nullptr, v, &s);
    return s;
}
static int failures = 0;
static void run(const char *name, std::vector<RtwSphere> sp, float t0, float t1, bool finite = true) {
    RtwScene sc; std::memset(&sc, 0, sizeof sc);
    sc.spheres = sp.data(); sc.n_spheres = (uint32_t)sp.size();
    uint32_t nn = 0, depth = 0, nbig = 0, f16 = 0;
    const int rc = rtw_bvh_validate(&sc, t0, t1, &nn, &depth, &nbig, &f16);
    BvhBuild a, b;
    build_bvh(sp.data(), (uint32_t)sp.size(), t0, t1, a);
    build_bvh(sp.data(), (uint32_t)sp.size(), t0, t1, b);
    const bool same = a.nodes.size() == b.nodes.size() && (a.nodes.empty() || !std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(BvhNode)));
    unsigned mism = 0;
    for (int k = 0; k < 200 && finite; k++) {
        const float o[3] = { 13.0f - 0.1f * k, 2.0f, 3.0f }, d[3] = { -13.0f + 0.05f * k, -2.0f + 0.01f * k, -3.0f + 0.02f * k };
        const HostHit h = bvh_closest_host(a, sp.data(), (uint32_t)sp.size(), o, d, t0, 0.001f, 1e5f, true), l = bvh_closest_host(a, sp.data(), (uint32_t)sp.size(), o, d, t0, 0.001f, 1e5f, false);
        mism += h.sphere != l.sphere || (h.sphere >= 0 && h.t != l.t);
    }
    const bool ok = (finite ? rc == RTW_OK : (rc == RTW_OK || rc == RTW_E_INVALID)) && depth <= a.depth_cap && a.depth_cap <= RTW_BVH_STACK && same && !mism;
    std::printf("%-28s n %5zu nodes %5u depth %2u cap %2u big %2u f16 %u validate %d %s\n", name, sp.size(), nn, depth, a.depth_cap, nbig, f16, rc, ok ? "ok" : "FAILED");
    failures += !ok;
}
static std::vector<RtwSphere> field(uint32_t n_small, uint32_t n_large, bool moving = false) {
    std::vector<RtwSphere> sp;
    uint32_t side = (uint32_t)std::ceil(std::sqrt((double)n_small)), x = 12345u;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (float)(x >> 8) * (1.0f / 16777216.0f); };
    for (uint32_t i = 0; i < n_small; i++)
        sp.push_back(sph((float)(i % side) - side / 2 + 0.9f * rnd(), 0.2f, (float)(i / side) - side / 2 + 0.9f * rnd(), 0.2f, moving && i % 3 == 0 ? 15.0f * rnd() : 0.0f));
    for (uint32_t k = 0; k < n_large; k++) sp.push_back(sph(-4.0f + 4.0f * k, 1.0f, 0.0f, 1.0f));
    return sp;
}
int main() {
    run("n = 1", { sph(0, 0, -1, 0.5f) }, 0, 0);
    run("n = 2", { sph(0, 0, -1, 0.5f), sph(1, 0, -1, 0.5f) }, 0, 0);
    run("n = 3", { sph(0, 0, -1, 0.5f), sph(1, 0, -1, 0.5f), sph(2, 0, -1, 0.25f) }, 0, 0);
    { std::vector<RtwSphere> s; for (int i = 0; i < 100; i++) s.push_back(sph(1, 2, 3, 0.1f + 0.01f * (i % 5))); run("all centres equal", s, 0, 0); }
    { std::vector<RtwSphere> s; for (int i = 0; i < 400; i++) s.push_back(sph(std::pow(1.2f, (float)i), 0, -5, 0.01f)); run("x = 1.2^i, n = 400", s, 0, 0); }
    { std::vector<RtwSphere> s; for (int i = 0; i < 500; i++) s.push_back(sph(std::pow(1.02f, (float)i), 0, -5, 0.01f)); run("x = 1.02^i, n = 500", s, 0, 0); }
    { std::vector<RtwSphere> s; for (int i = 0; i < 300; i++) s.push_back(sph(0.37f * i, 1, -2, 0.1f)); run("collinear", s, 0, 0); }
    run("480 small + 3 of 5x", field(480, 3), 0, 0);
    for (uint32_t n : { RTW_LDS_NODES_MAX, RTW_LDS_NODES_MAX + 1, RTW_LDS_NODES_MAX + 2, RTW_LDS_GEOM_MAX - 1, RTW_LDS_GEOM_MAX, RTW_LDS_GEOM_MAX + 1 }) {
        char nm[64]; std::snprintf(nm, sizeof nm, "field of %u", n); run(nm, field(n, 0), 0, 0);
    }
    run("moving, shutter 1/30", field(300, 3, true), 0, 1.0f / 30.0f);
    run("many (binned path)", field(RTW_BVH_OPTIMISE_MAX + 50, 0), 0, 0);
    for (float bad : { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 1e30f, 3e38f }) {
        std::vector<RtwSphere> s = field(200, 3);
        s[5].center[0] = bad; s[17].center[1] = bad; s[40].center[2] = bad; s[60].radius = bad; s[61].velocity[1] = bad;
        run("non-finite members", s, 0, 0.5f, false);
    }
    {   // a finite centre, a huge velocity, t_begin < 0 < t_end: ends of -inf and +inf, a centroid that is not a number
        std::vector<RtwSphere> s = field(200, 3);
        for (int i : { 3, 50, 120 }) s[i].velocity[0] = 3e38f;
        run("infinite box, finite centre", s, -2.0f, 2.0f, false);
    }
    {   // the reinsertion pass where it cannot prune: 1024 coincident centres, 1024 spheres at x = 1.01^i (the work budget ends it)
        std::vector<RtwSphere> s; for (int i = 0; i < 1024; i++) s.push_back(sph(1, 2, 3, 0.1f + 0.01f * (i % 5))); run("1024 coincident", s, 0, 0);
        s.clear(); for (int i = 0; i < 1024; i++) s.push_back(sph(std::pow(1.01f, (float)i), 0, -5, 0.01f)); run("x = 1.01^i, n = 1024", s, 0, 0);
    }
    std::printf(failures ? "%d FAILED\n" : "all ok\n", failures);
    return failures != 0;
}
