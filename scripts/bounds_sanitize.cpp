// bounds_sanitize.cpp -- a stand-alone driver for the host forms of the neighbourhood colour bounds and of the bounded temporal accumulation
// under AddressSanitizer + UBSan (host code only, no GPU): rtw_colour_bounds and rtw_temporal_accumulate_bounded on frames of 1 x 1, 7 x 1,
// 1 x 7, 5 x 4, 3 x 9 and 67 x 35 pixels, every buffer a heap block of exactly the documented size (idx NULL without same_object, out_clamped
// given and NULL): the bounds at radius 1 to 3, k of 0, 1 and 1e38 and the four combinations of same_object and exclude_centre over NaN,
// infinite, overflowing and denormal pixels and ids of -1, INT32_MIN and INT32_MAX; the accumulation under a static and a moved camera with
// the bounds of the new frame, open, NaN and cur itself, out_clipped given and NULL.  Checked: lo <= hi or a bound that is not finite; a
// constant frame gives lo == hi == the constant; out_clamped lies inside the box or is the input; open and NaN bounds give the bytes of
// rtw_temporal_accumulate_points; lo == hi == cur gives cur; every refusal writes nothing.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc bounds-asan
#include "rtw.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

// splitmix64: the frames are seeded, the same on every run
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static float uniform() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (float)((double)(z >> 11) * 0x1p-53);
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); failures++; } } while (0)

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (std::memcmp(&a[i], &b[i], 4) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
    return true;
}

static bool all_seven(const std::vector<float> &a) {
    for (float v : a) if (v != 7.0f) return false;
    return true;
}

struct Frame {
    uint32_t w, h;
    std::vector<float> rgb, depth, normal;
    std::vector<int32_t> idx;
};

static Frame make_frame(uint32_t w, uint32_t h, bool specials) {
    Frame f{ w, h, {}, {}, {}, {} };
    const size_t n = (size_t)w * h;
    f.rgb.resize(3 * n); f.depth.assign(n, 4.0f); f.normal.resize(3 * n); f.idx.resize(n);
    for (size_t p = 0; p < n; p++) {
        f.idx[p] = (int32_t)((p % w) / 3) - 1;
        for (int c = 0; c < 3; c++) {
            f.rgb[3 * p + c] = 0.1f + 0.2f * uniform();
            f.normal[3 * p + c] = c == 2 ? 1.0f : 0.0f;
        }
    }
    if (specials && n >= 7) {
        f.rgb[3 * 1] = NaN;
        f.rgb[3 * 2 + 1] = Inf;
        f.rgb[3 * 3 + 2] = -Inf;
        f.rgb[3 * 4] = 3e38f; f.rgb[3 * 4 + 1] = -3e38f;
        f.rgb[3 * 5] = 1e-45f; f.rgb[3 * 5 + 1] = -0.0f;
        f.rgb[3 * 6] = 1e4f;
        f.idx[0] = std::numeric_limits<int32_t>::min(); f.idx[n - 1] = std::numeric_limits<int32_t>::max();
    }
    return f;
}

static RtwCamera camera(uint32_t w, uint32_t h, float ox) {
    RtwCamera c;
    std::memset(&c, 0, sizeof c);
    const float a = 1.0f / 64.0f;
    c.origin[0] = ox;
    c.pixel00[0] = -(float)w * 0.5f * a + ox; c.pixel00[1] = (float)h * 0.5f * a; c.pixel00[2] = -1.0f;
    c.delta_u[0] = a; c.delta_v[1] = -a;
    return c;
}

int main() {
    const uint32_t shapes[6][2] = { { 1, 1 }, { 7, 1 }, { 1, 7 }, { 5, 4 }, { 3, 9 }, { 67, 35 } };
    int calls = 0;
    for (const auto &s : shapes) {
        const Frame f = make_frame(s[0], s[1], true);
        const size_t n = (size_t)f.w * f.h;
        // the bounds
        for (uint32_t radius = 1; radius <= RTW_BOUNDS_MAX_RADIUS; radius++)
            for (float k : { 0.0f, 1.0f, 1e38f })
                for (int flags = 0; flags < 8; flags++) {
                    const RtwColourBounds p = { radius, k, flags & 1 ? 1u : 0u, flags & 2 ? 1u : 0u };
                    std::vector<float> lo(3 * n, 7.0f), hi(3 * n, 7.0f), cl(3 * n, 7.0f);
                    RtwFilterStats st;
                    CHECK(rtw_colour_bounds(f.rgb.data(), f.w, f.h, flags & 1 ? f.idx.data() : nullptr, &p, lo.data(), hi.data(),
                                            flags & 4 ? cl.data() : nullptr, &st) == RTW_OK, "call");
                    CHECK(st.taps >= n && st.taps <= n * (2 * radius + 1) * (2 * radius + 1), "taps");
                    CHECK(flags & 4 ? true : all_seven(cl), "out_clamped NULL was written");
                    for (size_t i = 0; i < 3 * n; i++) {
                        CHECK(lo[i] <= hi[i] || !std::isfinite(lo[i]) || !std::isfinite(hi[i]), "%u x %u: lo %a > hi %a at %zu", f.w, f.h, lo[i], hi[i], i);
                        if (flags & 4) {
                            const float x = f.rgb[i];
                            const bool inside = cl[i] >= lo[i] && cl[i] <= hi[i];
                            CHECK(inside || std::memcmp(&cl[i], &x, 4) == 0 || (std::isnan(cl[i]) && std::isnan(x)), "out_clamped %a of %a at %zu", cl[i], x, i);
                        }
                    }
                    calls++;
                }
        {   // a constant frame
            std::vector<float> flat(3 * n, 0.75f), lo(3 * n), hi(3 * n);
            const RtwColourBounds p = { 3, 3.0f, 0u, 0u };
            CHECK(rtw_colour_bounds(flat.data(), f.w, f.h, nullptr, &p, lo.data(), hi.data(), nullptr, nullptr) == RTW_OK, "flat");
            CHECK(same_bits(lo, flat) && same_bits(hi, flat), "%u x %u: a constant frame", f.w, f.h);
            calls++;
        }
        // the bounded accumulation: a first frame, then a second under a static and under a moved camera
        const Frame g = make_frame(s[0], s[1], true);
        const RtwTemporal tp = { 0.2f, 0.2f, 32, 0.05f, 0.9f, 1u, { 0.5f, 0.5f } };
        const RtwCamera c0 = camera(f.w, f.h, 0.0f);
        std::vector<float> hc(3 * n), hm(2 * n), hl(n), hv(n), hcl(n, 7.0f);
        CHECK(rtw_temporal_accumulate_bounded(f.rgb.data(), f.w, f.h, &c0, f.depth.data(), f.normal.data(), f.idx.data(), nullptr, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, nullptr, &tp, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, hc.data(),
                                              hm.data(), hl.data(), hv.data(), nullptr, hcl.data(), nullptr) == RTW_OK, "first frame");
        for (float v : hcl) CHECK(v == 0.0f, "clipped %a on a first frame", v);
        calls++;
        for (float shift : { 0.0f, 1.0f / 32.0f }) {
            const RtwCamera c1 = camera(f.w, f.h, shift);
            std::vector<float> pc(3 * n), pm(2 * n), pl(n), pv(n), pxy(2 * n);
            CHECK(rtw_temporal_accumulate_points(g.rgb.data(), g.w, g.h, &c1, g.depth.data(), g.normal.data(), g.idx.data(), &c0, hc.data(), hm.data(),
                                                 hl.data(), f.depth.data(), f.normal.data(), f.idx.data(), &tp, nullptr, 0, 0, nullptr, nullptr,
                                                 pc.data(), pm.data(), pl.data(), pv.data(), pxy.data(), nullptr) == RTW_OK, "points");
            std::vector<float> box_lo(3 * n), box_hi(3 * n);
            const RtwColourBounds bp = { 1, 0.5f, 0u, 0u };
            CHECK(rtw_colour_bounds(g.rgb.data(), g.w, g.h, nullptr, &bp, box_lo.data(), box_hi.data(), nullptr, nullptr) == RTW_OK, "box");
            for (int kind = 0; kind < 4; kind++) {                                       // the frame's box, open, NaN, cur itself
                std::vector<float> lo(box_lo), hi(box_hi);
                if (kind == 1) { lo.assign(3 * n, -Inf); hi.assign(3 * n, Inf); }
                if (kind == 2) { lo.assign(3 * n, NaN); hi.assign(3 * n, NaN); }
                if (kind == 3) { lo = g.rgb; hi = g.rgb; }
                for (int with_clipped = 0; with_clipped < 2; with_clipped++) {
                    std::vector<float> oc(3 * n, 7.0f), om(2 * n), ol(n), ov(n), oxy(2 * n), ocl(n, 7.0f);
                    CHECK(rtw_temporal_accumulate_bounded(g.rgb.data(), g.w, g.h, &c1, g.depth.data(), g.normal.data(), g.idx.data(), &c0, hc.data(),
                                                          hm.data(), hl.data(), f.depth.data(), f.normal.data(), f.idx.data(), &tp, nullptr, 0, 0,
                                                          nullptr, nullptr, lo.data(), hi.data(), oc.data(), om.data(), ol.data(), ov.data(),
                                                          oxy.data(), with_clipped ? ocl.data() : nullptr, nullptr) == RTW_OK, "bounded");
                    calls++;
                    CHECK(same_bits(om, pm) && same_bits(ol, pl) && same_bits(ov, pv) && same_bits(oxy, pxy), "the bounds moved the moments or the length");
                    CHECK(with_clipped || all_seven(ocl), "out_clipped NULL was written");
                    if (kind == 1 || kind == 2) {
                        CHECK(same_bits(oc, pc), "%u x %u kind %d: not the _points call's bytes", f.w, f.h, kind);
                        if (with_clipped) for (float v : ocl) CHECK(v == 0.0f, "clipped %a under an open box", v);
                    }
                    if (kind == 3)
                        for (size_t q = 0; q < n; q++) {
                            const float *x = &g.rgb[3 * q];
                            if (ol[q] > 1.0f && std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]))
                                CHECK(oc[3 * q] == x[0] && oc[3 * q + 1] == x[1] && oc[3 * q + 2] == x[2], "lo == hi == cur at %zu", q);     // (-0 comes back as +0)
                        }
                    if (with_clipped) for (float v : ocl) CHECK(v >= 0.0f || std::isnan(v), "clipped %a", v);
                }
            }
        }
    }
    {   // the refusals: nothing is written
        const Frame f = make_frame(5, 4, false);
        const size_t n = 20;
        std::vector<float> lo(3 * n, 7.0f), hi(3 * n, 7.0f), cl(3 * n, 7.0f);
        const float *in = f.rgb.data();
        const int32_t *i = f.idx.data();
        const RtwColourBounds ok = { 2, 1.0f, 1u, 0u };
        auto refused = [&](const float *in_, uint32_t w, uint32_t h, const int32_t *i_, const RtwColourBounds *p, float *l, float *u, float *c) {
            CHECK(rtw_colour_bounds(in_, w, h, i_, p, l, u, c, nullptr) == RTW_E_INVALID, "not refused");
            CHECK(all_seven(lo) && all_seven(hi) && all_seven(cl), "a refused call wrote");
        };
        refused(nullptr, 5, 4, i, &ok, lo.data(), hi.data(), cl.data());
        refused(in, 5, 4, i, nullptr, lo.data(), hi.data(), cl.data());
        refused(in, 5, 4, i, &ok, nullptr, hi.data(), cl.data());
        refused(in, 5, 4, i, &ok, lo.data(), nullptr, cl.data());
        refused(in, 0, 4, i, &ok, lo.data(), hi.data(), cl.data());
        refused(in, 5, 0, i, &ok, lo.data(), hi.data(), cl.data());
        refused(in, 65536, 65536, i, &ok, lo.data(), hi.data(), cl.data());
        refused(in, RTW_ATROUS_MAX_SIDE + 1, 1, i, &ok, lo.data(), hi.data(), cl.data());
        refused(in, 5, 4, nullptr, &ok, lo.data(), hi.data(), cl.data());
        RtwColourBounds p = ok; p.radius = 0; refused(in, 5, 4, i, &p, lo.data(), hi.data(), cl.data());
        p = ok; p.radius = RTW_BOUNDS_MAX_RADIUS + 1; refused(in, 5, 4, i, &p, lo.data(), hi.data(), cl.data());
        for (float v : { -1.0f, NaN, Inf }) { p = ok; p.k = v; refused(in, 5, 4, i, &p, lo.data(), hi.data(), cl.data()); }
        p = ok; p.same_object = 2; refused(in, 5, 4, i, &p, lo.data(), hi.data(), cl.data());
        p = ok; p.exclude_centre = 2; refused(in, 5, 4, i, &p, lo.data(), hi.data(), cl.data());
        refused(in, 5, 4, i, &ok, lo.data(), lo.data(), cl.data());
        refused(in, 5, 4, i, &ok, lo.data(), hi.data(), lo.data());
        refused(in, 5, 4, i, &ok, lo.data(), hi.data(), hi.data());
        {   // an output that is `in`
            std::vector<float> in2(f.rgb);
            CHECK(rtw_colour_bounds(in2.data(), 5, 4, i, &ok, in2.data(), hi.data(), cl.data(), nullptr) == RTW_E_INVALID, "out_lo == in");
            CHECK(rtw_colour_bounds(in2.data(), 5, 4, i, &ok, lo.data(), in2.data(), cl.data(), nullptr) == RTW_E_INVALID, "out_hi == in");
            CHECK(rtw_colour_bounds(in2.data(), 5, 4, i, &ok, lo.data(), hi.data(), in2.data(), nullptr) == RTW_E_INVALID, "out_clamped == in");
            CHECK(same_bits(in2, f.rgb) && all_seven(lo) && all_seven(hi) && all_seven(cl), "a refused call wrote");
        }
        // the bounded accumulation's own
        const RtwTemporal tp = { 0.2f, 0.2f, 32, 0.05f, 0.9f, 1u, { 0.5f, 0.5f } };
        const RtwCamera c0 = camera(5, 4, 0.0f);
        std::vector<float> hc(f.rgb), hm(2 * n, 0.5f), hl(n, 1.0f), bl(3 * n, 0.0f), bh(3 * n, 1.0f);
        std::vector<float> oc(3 * n, 7.0f), om(2 * n, 7.0f), ol(n, 7.0f), ov(n, 7.0f), oxy(2 * n, 7.0f), ocl(n, 7.0f);
        auto t_refused = [&](const float *l, const float *u, float *clipped) {
            CHECK(rtw_temporal_accumulate_bounded(in, 5, 4, &c0, f.depth.data(), f.normal.data(), i, &c0, hc.data(), hm.data(), hl.data(), f.depth.data(),
                                                  f.normal.data(), i, &tp, nullptr, 0, 0, nullptr, nullptr, l, u, oc.data(), om.data(), ol.data(),
                                                  ov.data(), oxy.data(), clipped, nullptr) == RTW_E_INVALID, "not refused");
            CHECK(all_seven(oc) && all_seven(om) && all_seven(ol) && all_seven(ov) && all_seven(oxy) && all_seven(ocl), "a refused call wrote");
        };
        t_refused(bl.data(), nullptr, ocl.data());
        t_refused(nullptr, bh.data(), ocl.data());
        for (float *o : { oc.data(), om.data(), ol.data(), ov.data(), oxy.data() }) {
            t_refused(o, bh.data(), ocl.data());
            t_refused(bl.data(), o, ocl.data());
            t_refused(bl.data(), bh.data(), o);
        }
        {
            std::vector<float> b2(bl);
            CHECK(rtw_temporal_accumulate_bounded(in, 5, 4, &c0, f.depth.data(), f.normal.data(), i, &c0, hc.data(), hm.data(), hl.data(), f.depth.data(),
                                                  f.normal.data(), i, &tp, nullptr, 0, 0, nullptr, nullptr, b2.data(), bh.data(), oc.data(), om.data(),
                                                  ol.data(), ov.data(), oxy.data(), b2.data(), nullptr) == RTW_E_INVALID, "out_clipped == hist_lo");
            CHECK(rtw_temporal_accumulate_bounded(in, 5, 4, &c0, f.depth.data(), f.normal.data(), i, &c0, hc.data(), hm.data(), hl.data(), f.depth.data(),
                                                  f.normal.data(), i, &tp, nullptr, 0, 0, nullptr, nullptr, bl.data(), b2.data(), oc.data(), om.data(),
                                                  ol.data(), ov.data(), oxy.data(), b2.data(), nullptr) == RTW_E_INVALID, "out_clipped == hist_hi");
            CHECK(same_bits(b2, bl) && all_seven(oc), "a refused call wrote");
        }
    }
    std::printf("bounds_sanitize: %d calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
