// atrous_sanitize.cpp -- a stand-alone driver for the a-trous filter's host form under AddressSanitizer + UBSan (host code only, no GPU):
// rtw_atrous_filter on frames of 1 x 1, 5 x 3, 17 x 9 and 67 x 35 pixels with 1, 3 and 8 levels, each term alone and all together, with
// and without albedo and emission, every buffer a heap block of exactly the documented size (a guide whose term is off is NULL), NaN and
// infinite pixels, a NaN depth and miss pixels among them.  Checked: out == in gives the bytes of the separate call; a constant frame comes
// back within a rounding of the sum; a NaN pixel stays NaN and reaches no other pixel while the colour term is on; every refusal writes nothing.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc atrous-asan
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

struct Frame {
    uint32_t w, h;
    std::vector<float> rgb, depth, normal, albedo, emitted;
    std::vector<int32_t> idx;
};

static Frame make_frame(uint32_t w, uint32_t h, bool specials) {
    Frame f{ w, h, {}, {}, {}, {}, {}, {} };
    const size_t n = (size_t)w * h;
    f.rgb.resize(3 * n); f.depth.resize(n); f.normal.resize(3 * n); f.albedo.resize(3 * n); f.emitted.resize(3 * n); f.idx.resize(n);
    for (size_t p = 0; p < n; p++) {
        const int id = (int)((p % w) * 3 / w) - ((p / w) * 2 / h ? 1 : 0);           // -1 (miss), 0, 1, 2 in blocks
        f.idx[p] = id;
        f.depth[p] = id < 0 ? 1600.0f : 4.0f + 3.0f * (float)id + 0.05f * uniform();
        for (int c = 0; c < 3; c++) {
            f.normal[3 * p + c] = id < 0 ? 0.0f : (c == id ? 1.0f : 0.1f * uniform());
            f.albedo[3 * p + c] = id < 0 ? 0.0f : 0.2f + 0.7f * uniform();
            f.emitted[3 * p + c] = id == 2 ? uniform() : 0.0f;
            f.rgb[3 * p + c] = f.albedo[3 * p + c] * (0.5f + 0.5f * uniform()) + f.emitted[3 * p + c] + (id < 0 ? 0.7f : 0.0f);
        }
    }
    if (specials && n >= 15) {
        f.rgb[3 * 4] = std::numeric_limits<float>::quiet_NaN();
        f.rgb[3 * 7 + 1] = std::numeric_limits<float>::infinity();
        f.depth[9] = std::numeric_limits<float>::quiet_NaN();
        f.albedo[3 * 11] = std::nextafter(0.05f, 0.0f); f.albedo[3 * 11 + 1] = 0.05f;
    }
    return f;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (std::memcmp(&a[i], &b[i], 4) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
    return true;
}

int main() {
    const uint32_t shapes[4][2] = { { 1, 1 }, { 5, 3 }, { 17, 9 }, { 67, 35 } };
    const uint32_t levels[3] = { 1, 3, 8 };
    int calls = 0;
    for (const auto &s : shapes) {
        const Frame f = make_frame(s[0], s[1], true);
        for (uint32_t lv : levels)
            for (int terms = 0; terms < 16; terms++)
                for (int alb = 0; alb < 3; alb++) {                                  // no albedo; albedo; albedo + emission
                    const RtwAtrous p = { lv, terms & 1 ? 0.75f : 0.0f, terms & 2 ? 0.5f : 0.0f, terms & 4 ? 0.6f : 0.0f, terms & 8 ? 1u : 0u, 0.05f };
                    const float *depth = terms & 2 ? f.depth.data() : nullptr, *normal = terms & 4 ? f.normal.data() : nullptr;
                    const int32_t *idx = terms & 8 ? f.idx.data() : nullptr;
                    const float *albedo = alb ? f.albedo.data() : nullptr, *emitted = alb == 2 ? f.emitted.data() : nullptr;
                    std::vector<float> out(f.rgb.size(), 7.0f), inplace(f.rgb);
                    RtwFilterStats st;
                    CHECK(rtw_atrous_filter(f.rgb.data(), f.w, f.h, depth, normal, idx, albedo, emitted, &p, out.data(), &st) == RTW_OK, "call");
                    CHECK(rtw_atrous_filter(inplace.data(), f.w, f.h, depth, normal, idx, albedo, emitted, &p, inplace.data(), nullptr) == RTW_OK, "in place");
                    CHECK(same_bits(out, inplace), "%u x %u levels %u terms %d albedo %d: out == in gives other bytes", f.w, f.h, lv, terms, alb);
                    CHECK(st.taps >= (uint64_t)f.w * f.h * lv, "taps");
                    if ((terms & 1) && f.rgb.size() >= 45) {
                        CHECK(std::isnan(out[3 * 4]), "a NaN centre keeps its value");
                        size_t nans = 0;
                        for (size_t i = 0; i < out.size(); i++) nans += std::isnan(out[i]) ? 1 : 0;
                        CHECK(nans <= 3, "%u x %u levels %u terms %d: %zu NaNs came out of one NaN channel", f.w, f.h, lv, terms, nans);
                    }
                    calls += 2;
                }
    }
    {   // a constant frame is a fixed point up to the rounding of the weighted mean
        Frame f = make_frame(33, 17, false);
        for (float &v : f.rgb) v = 0.25f;
        const RtwAtrous p = { 8, 1.0f, 0.0f, 0.0f, 0u, 0.0f };
        std::vector<float> out(f.rgb.size());
        CHECK(rtw_atrous_filter(f.rgb.data(), f.w, f.h, nullptr, nullptr, nullptr, nullptr, nullptr, &p, out.data(), nullptr) == RTW_OK, "constant");
        for (float v : out) CHECK(std::fabs(v - 0.25f) <= 0x1p-24f, "constant frame: %a", v);
    }
    {   // the refusals: nothing is written
        const Frame f = make_frame(17, 9, false);
        std::vector<float> out(f.rgb.size(), 7.0f);
        const RtwAtrous ok = { 3, 0.5f, 0.5f, 0.5f, 1u, 0.05f };
        auto refused = [&](const float *in, uint32_t w, uint32_t h, const float *d, const float *n, const int32_t *i, const float *a, const RtwAtrous *p,
                           float *o) {
            CHECK(rtw_atrous_filter(in, w, h, d, n, i, a, f.emitted.data(), p, o, nullptr) == RTW_E_INVALID, "not refused");
            for (float v : out) if (v != 7.0f) { CHECK(false, "a refused call wrote"); break; }
        };
        const float *in = f.rgb.data(), *d = f.depth.data(), *n = f.normal.data(), *a = f.albedo.data();
        const int32_t *i = f.idx.data();
        refused(nullptr, 17, 9, d, n, i, a, &ok, out.data());
        refused(in, 17, 9, d, n, i, a, &ok, nullptr);
        refused(in, 17, 9, d, n, i, a, nullptr, out.data());
        refused(in, 0, 9, d, n, i, a, &ok, out.data());
        refused(in, 17, 0, d, n, i, a, &ok, out.data());
        refused(in, 65536, 65536, d, n, i, a, &ok, out.data());
        refused(in, 17, 9, nullptr, n, i, a, &ok, out.data());
        refused(in, 17, 9, d, nullptr, i, a, &ok, out.data());
        refused(in, 17, 9, d, n, nullptr, a, &ok, out.data());
        const float bad[5] = { -1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), 1e-30f, -1e-30f };
        for (float v : bad) {
            RtwAtrous p = ok; p.sigma_color = v; refused(in, 17, 9, d, n, i, a, &p, out.data());
            p = ok; p.sigma_depth = v; refused(in, 17, 9, d, n, i, a, &p, out.data());
            p = ok; p.sigma_normal = v; refused(in, 17, 9, d, n, i, a, &p, out.data());
        }
        RtwAtrous p = ok; p.levels = 0; refused(in, 17, 9, d, n, i, a, &p, out.data());
        p = ok; p.levels = RTW_ATROUS_MAX_LEVELS + 1; refused(in, 17, 9, d, n, i, a, &p, out.data());
        p = ok; p.levels = 8; p.sigma_color = 1e-18f; refused(in, 17, 9, d, n, i, a, &p, out.data());
        p = ok; p.same_object = 2; refused(in, 17, 9, d, n, i, a, &p, out.data());
        p = ok; p.albedo_floor = 0.0f; refused(in, 17, 9, d, n, i, a, &p, out.data());
        p = ok; p.albedo_floor = std::numeric_limits<float>::quiet_NaN(); refused(in, 17, 9, d, n, i, a, &p, out.data());
    }
    std::printf("atrous_sanitize: %d filter calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
