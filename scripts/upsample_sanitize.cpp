// upsample_sanitize.cpp -- a stand-alone driver for the host form of the guide-steered upsampling and for rtw_camera_scaled under
// AddressSanitizer + UBSan (host code only, no GPU): rtw_upsample_filter over output sizes of 1 x 1, 5 x 4, 13 x 7 and 33 x 17 pixels, scales
// 1, 2, 3, 4 and 8, both radii and the sixteen on/off combinations of the depth, normal, id and albedo/emission terms, every buffer a heap
// block of exactly the documented size (a guide whose term is off, and albedo and emission without their term, NULL; wsum_out given and
// NULL); the edge values NaN, +-inf, 3e38, a denormal and -0 in low pixels at the corners, on the edges and inside; every refusal.
// Checked: without terms a constant frame gives the constant; wsum_out is 0 exactly where out is the covering low pixel's bytes; the taps
// counted lie between one and (2 radius)^2 a pixel; a refusal writes nothing; rtw_camera_scaled scales the two deltas alone.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc upsample-asan
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

static bool all_seven(const std::vector<float> &a) {
    for (float v : a) if (v != 7.0f) return false;
    return true;
}

// One size's guides, each vector of exactly the documented length.
struct Side {
    uint32_t w, h;
    std::vector<float> depth, normal, albedo, emitted;
    std::vector<int32_t> idx;
    RtwGuides pod(int terms) const {         // bit 0 depth, 1 normal, 2 idx, 3 albedo + emission
        return RtwGuides{ terms & 1 ? depth.data() : nullptr, terms & 2 ? normal.data() : nullptr, terms & 4 ? idx.data() : nullptr,
                          terms & 8 ? albedo.data() : nullptr, terms & 8 ? emitted.data() : nullptr };
    }
};

static Side make_side(uint32_t w, uint32_t h, uint32_t step) {
    Side s{ w, h, {}, {}, {}, {}, {} };
    const size_t n = (size_t)w * h;
    s.depth.resize(n); s.normal.resize(3 * n); s.albedo.resize(3 * n); s.emitted.assign(3 * n, 0.0f); s.idx.resize(n);
    for (uint32_t j = 0; j < h; j++)
        for (uint32_t i = 0; i < w; i++) {
            const size_t p = (size_t)j * w + i;
            const uint32_t x = i * step + step / 2, y = j * step + step / 2;
            s.idx[p] = (int32_t)((x / 5) % 3) - 1;
            s.depth[p] = 1.0f + 0.02f * (float)x + 0.4f * (float)(s.idx[p] + 1);
            s.normal[3 * p] = (float)s.idx[p]; s.normal[3 * p + 1] = 0.5f; s.normal[3 * p + 2] = 0.25f * (float)(y % 3);
            s.albedo[3 * p] = 0.2f + 0.1f * (float)(x % 4); s.albedo[3 * p + 1] = 0.04f; s.albedo[3 * p + 2] = 0.05f;
            if (s.idx[p] == 1) s.emitted[3 * p + 2] = 2.0f;
        }
    if (n > 2) { s.idx[0] = std::numeric_limits<int32_t>::min(); s.idx[n - 1] = std::numeric_limits<int32_t>::max(); }
    return s;
}

int main() {
    const uint32_t sizes[4][2] = { { 1, 1 }, { 5, 4 }, { 13, 7 }, { 33, 17 } };
    const uint32_t scales[5] = { 1, 2, 3, 4, 8 };
    const float edge[6][3] = { { NaN, 0.5f, 0.5f }, { 0.5f, Inf, 0.5f }, { 0.5f, 0.5f, -Inf }, { 3e38f, 0.5f, -3e38f }, { 1e-45f, -1e-45f, -0.0f },
                               { -0.0f, -0.0f, -0.0f } };
    int calls = 0;
    for (const auto &sz : sizes)
        for (uint32_t scale : scales) {
            const uint32_t w = sz[0], h = sz[1], w_lo = (w + scale - 1) / scale, h_lo = (h + scale - 1) / scale;
            const size_t n = (size_t)w * h, n_lo = (size_t)w_lo * h_lo;
            const Side lo = make_side(w_lo, h_lo, scale), hi = make_side(w, h, 1);
            for (int which = -1; which < 6; which++) {
                std::vector<float> fr(3 * n_lo);
                for (float &v : fr) v = 2.0f * uniform();
                if (which >= 0) {
                    const size_t places[5] = { 0, n_lo - 1, w_lo - 1, n_lo / 2, n_lo - w_lo };
                    for (size_t q : places) std::memcpy(&fr[3 * q], edge[which], 12);
                }
                for (uint32_t radius = 1; radius <= RTW_UPSAMPLE_MAX_RADIUS; radius++)
                    for (int terms = 0; terms < 16; terms++) {
                        if (which >= 0 && terms != 0 && terms != 15 && terms != 8) continue;
                        const RtwUpsample p = { scale, radius, terms & 1 ? 0.5f : 0.0f, terms & 2 ? 0.6f : 0.0f, terms & 4 ? 1u : 0u, 0.05f };
                        const RtwGuides gl = lo.pod(terms), gh = hi.pod(terms);
                        for (int with_wsum = 0; with_wsum < 2; with_wsum++) {
                            std::vector<float> out(3 * n, 7.0f), ws(n, 7.0f);
                            RtwFilterStats st;
                            CHECK(rtw_upsample_filter(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &p, out.data(), with_wsum ? ws.data() : nullptr, &st) == RTW_OK,
                                  "call %u x %u scale %u radius %u terms %d", w, h, scale, radius, terms);
                            CHECK(st.taps >= n && st.taps <= n * 4 * radius * radius, "taps %llu", (unsigned long long)st.taps);
                            CHECK(with_wsum || all_seven(ws), "wsum_out NULL was written");
                            if (with_wsum && !(terms & 8))
                                for (size_t q = 0; q < n; q++) {
                                    CHECK(ws[q] >= 0.0f, "wsum %a", ws[q]);
                                    if (ws[q] == 0.0f) {          // the fallback: the covering low pixel's bytes
                                        const size_t c = (size_t)((q / w) / scale) * w_lo + (q % w) / scale;
                                        CHECK(std::memcmp(&out[3 * q], &fr[3 * c], 12) == 0 || std::isnan(out[3 * q]) || std::isnan(out[3 * q + 1]) ||
                                              std::isnan(out[3 * q + 2]), "fallback at %zu", q);
                                    }
                                }
                            calls++;
                        }
                    }
            }
            {   // a constant frame without terms
                std::vector<float> flat(3 * n_lo, 0.75f), out(3 * n);
                for (uint32_t radius = 1; radius <= RTW_UPSAMPLE_MAX_RADIUS; radius++) {
                    const RtwUpsample p = { scale, radius, 0.0f, 0.0f, 0u, 0.0f };
                    CHECK(rtw_upsample_filter(flat.data(), w_lo, h_lo, nullptr, w, h, nullptr, &p, out.data(), nullptr, nullptr) == RTW_OK, "flat");
                    for (float v : out) CHECK(std::fabs(v - 0.75f) <= 4.0f * 0.75f * 0x1p-24f * (float)(4 * radius * radius + 2), "flat gives %a", v);
                    calls++;
                }
            }
        }

    {   // every refusal: nothing is written
        const uint32_t w = 5, h = 4, s = 2, w_lo = 3, h_lo = 2;
        const Side lo = make_side(w_lo, h_lo, s), hi = make_side(w, h, 1);
        std::vector<float> fr(3 * w_lo * h_lo, 0.5f), out(3 * w * h, 7.0f), ws(w * h, 7.0f);
        const RtwGuides gl = lo.pod(15), gh = hi.pod(15);
        const RtwUpsample ok = { s, 1, 0.5f, 0.6f, 1, 0.05f };
        int refusals = 0;
        auto refused = [&](const float *f, uint32_t wl, uint32_t hl, const RtwGuides *a, uint32_t ww, uint32_t hh, const RtwGuides *b, const RtwUpsample *p,
                           float *o, float *x) {
            CHECK(rtw_upsample_filter(f, wl, hl, a, ww, hh, b, p, o, x, nullptr) == RTW_E_INVALID, "refusal %d accepted", refusals);
            CHECK(all_seven(out) && all_seven(ws), "refusal %d wrote", refusals);
            refusals++;
        };
        refused(nullptr, w_lo, h_lo, &gl, w, h, &gh, &ok, out.data(), ws.data());
        refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &ok, nullptr, ws.data());
        refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, nullptr, out.data(), ws.data());
        refused(fr.data(), w_lo, h_lo, &gl, 0, h, &gh, &ok, out.data(), ws.data());
        refused(fr.data(), w_lo, h_lo, &gl, w, 0, &gh, &ok, out.data(), ws.data());
        refused(fr.data(), 0, h_lo, &gl, w, h, &gh, &ok, out.data(), ws.data());
        refused(fr.data(), w_lo + 1, h_lo, &gl, w, h, &gh, &ok, out.data(), ws.data());
        refused(fr.data(), w_lo, h_lo - 1, &gl, w, h, &gh, &ok, out.data(), ws.data());
        refused(fr.data(), w / s, h_lo, &gl, w, h, &gh, &ok, out.data(), ws.data());
        { RtwUpsample p = ok; p.scale = 1; refused(fr.data(), 0x7FFFFC01u, 1, &gl, 0x7FFFFC01u, 1, &gh, &p, out.data(), ws.data()); }
        for (uint32_t bad : { 0u, RTW_UPSAMPLE_MAX_SCALE + 1 }) { RtwUpsample p = ok; p.scale = bad; refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &p, out.data(), ws.data()); }
        for (uint32_t bad : { 0u, RTW_UPSAMPLE_MAX_RADIUS + 1 }) { RtwUpsample p = ok; p.radius = bad; refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &p, out.data(), ws.data()); }
        for (float bad : { -0.5f, NaN, Inf, -Inf, 1e-30f }) {
            RtwUpsample p = ok; p.sigma_depth = bad; refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &p, out.data(), ws.data());
            p = ok; p.sigma_normal = bad; refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &p, out.data(), ws.data());
        }
        { RtwUpsample p = ok; p.same_object = 2; refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &p, out.data(), ws.data()); }
        for (int term = 0; term < 3; term++) {
            const RtwGuides ml = lo.pod(15 & ~(1 << term)), mh = hi.pod(15 & ~(1 << term));
            refused(fr.data(), w_lo, h_lo, &ml, w, h, &gh, &ok, out.data(), ws.data());
            refused(fr.data(), w_lo, h_lo, &gl, w, h, &mh, &ok, out.data(), ws.data());
            refused(fr.data(), w_lo, h_lo, nullptr, w, h, &gh, &ok, out.data(), ws.data());
            refused(fr.data(), w_lo, h_lo, &gl, w, h, nullptr, &ok, out.data(), ws.data());
        }
        for (float bad : { 0.0f, -1.0f, NaN, Inf }) {
            RtwUpsample p = ok; p.albedo_floor = bad;
            const RtwGuides one = lo.pod(7);
            refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &p, out.data(), ws.data());
            refused(fr.data(), w_lo, h_lo, &one, w, h, &gh, &p, out.data(), ws.data());
        }
        refused(fr.data(), w_lo, h_lo, &gl, w, h, &gh, &ok, out.data(), out.data());
        std::printf("upsample_sanitize: %d refusals, nothing written\n", refusals);
    }

    {   // rtw_camera_scaled
        RtwCamera c, o;
        float *f = (float *)&c;
        for (size_t i = 0; i < sizeof c / 4; i++) f[i] = 0.125f + (float)i;
        for (uint32_t s = 1; s <= RTW_UPSAMPLE_MAX_SCALE; s++) {
            CHECK(rtw_camera_scaled(&c, s, &o) == RTW_OK, "camera scale %u", s);
            RtwCamera want = c;
            for (int k = 0; k < 3; k++) { want.delta_u[k] = c.delta_u[k] * (float)s; want.delta_v[k] = c.delta_v[k] * (float)s; }
            CHECK(std::memcmp(&o, &want, sizeof o) == 0, "camera scale %u", s);
        }
        CHECK(rtw_camera_scaled(&c, 3, &c) == RTW_OK && c.delta_u[0] == o.delta_u[0] / 8.0f * 3.0f, "in place");
        CHECK(rtw_camera_scaled(nullptr, 2, &o) == RTW_E_INVALID && rtw_camera_scaled(&c, 2, nullptr) == RTW_E_INVALID, "NULL");
        CHECK(rtw_camera_scaled(&c, 0, &o) == RTW_E_INVALID && rtw_camera_scaled(&c, RTW_UPSAMPLE_MAX_SCALE + 1, &o) == RTW_E_INVALID, "scale range");
    }
    std::printf("upsample_sanitize: %d calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
