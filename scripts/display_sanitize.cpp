// display_sanitize.cpp -- a stand-alone driver for the host forms of the display stage under AddressSanitizer + UBSan (host code only, no
// GPU): rtw_luminance_histogram, rtw_exposure_from_histogram and rtw_display over frames of 1 x 1, 3 x 1, 5 x 3, 64 x 48 and 257 x 3 pixels,
// every tone x transfer x quantise x dither x format combination, every buffer a heap block of exactly the documented size (hist 256 and
// counts 2 uint32; out 3, 4 or 12 bytes a pixel); the special values NaN, +-inf, +-FLT_MAX, subnormals, +-0, negatives, the sRGB knee in every
// channel; white tiny and huge; every refusal.
// Checked: sum(hist) + counts == w * h; RGBA8 is RGB8 plus 255; plain RGB8 is rtw_quantize_u8's rule; the level metered from a frame's
// histogram lies in [0, 256] and its exposure is finite and positive; a refusal writes nothing.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc display-asan
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
static const float FMax = std::numeric_limits<float>::max();

static size_t pixel_bytes(uint32_t fmt) { return fmt == RTW_DISPLAY_F32 ? 12 : (fmt == RTW_DISPLAY_RGBA8 ? 4 : 3); }

template <class T> static bool all_are(const std::vector<T> &a, T v) {
    for (T x : a) if (x != v) return false;
    return true;
}

static std::vector<float> make_frame(uint32_t w, uint32_t h, bool specials) {
    std::vector<float> f((size_t)w * h * 3);
    for (float &v : f) v = std::exp2(-14.0f + 16.0f * uniform());
    if (specials) {
        const float s[] = { NaN, Inf, -Inf, FMax, -FMax, 1e-45f, -1e-45f, 1e-38f, 0.0f, -0.0f, -1.0f, 1.0f, 0.0031308f, 0.00313081f, 0.00313079f,
                            65536.0f, 1.52587890625e-05f, 3e-8f };
        const size_t ns = sizeof s / sizeof s[0];
        for (size_t k = 0; k < f.size(); k += 2) f[k] = s[(k / 2) % ns];
    }
    return f;
}

int main() {
    const uint32_t sizes[5][2] = { { 1, 1 }, { 3, 1 }, { 5, 3 }, { 64, 48 }, { 257, 3 } };
    int calls = 0;
    for (const auto &sz : sizes)
        for (int specials = 0; specials < 2; specials++) {
            const uint32_t w = sz[0], h = sz[1];
            const size_t n = (size_t)w * h;
            const std::vector<float> frame = make_frame(w, h, specials != 0);
            // -- the histogram and the metering
            std::vector<uint32_t> hist(256, 9u), counts(2, 9u);
            RtwFilterStats st;
            CHECK(rtw_luminance_histogram(frame.data(), w, h, hist.data(), counts.data(), &st) == RTW_OK, "histogram %u x %u", w, h);
            calls++;
            uint64_t total = (uint64_t)counts[0] + counts[1];
            for (uint32_t c : hist) total += c;
            CHECK(total == n && st.taps == n, "histogram %u x %u counts %llu pixels", w, h, (unsigned long long)total);
            const RtwMetering meterings[4] = { { 50, 50, 0.18f, 1.0f, 0.0f, 256.0f }, { 0, 0, 1.0f, 0.5f, 0.0f, 256.0f },
                                               { 999, 0, 0.18f, 0.0f, 100.0f, 101.0f }, { 0, 999, 5.0f, 1.0f, 256.0f, 256.0f } };
            const double prevs[4] = { std::numeric_limits<double>::quiet_NaN(), 0.0, 131.5, 256.0 };
            for (const RtwMetering &m : meterings)
                for (double prev : prevs) {
                    double level = -1.0;
                    float exposure = -1.0f;
                    CHECK(rtw_exposure_from_histogram(hist.data(), &m, prev, 0.5f, &level, &exposure) == RTW_OK, "exposure");
                    calls++;
                    const bool nothing = total == (uint64_t)counts[0] + counts[1];
                    if (!(nothing && prev != prev))
                        CHECK(level >= 0.0 && level <= 256.0 && exposure > 0.0f && std::isfinite(exposure), "level %g exposure %g", level, (double)exposure);
                }
            // -- the display transform
            for (uint32_t tone = 0; tone < 4; tone++)
                for (uint32_t transfer = 0; transfer < 2; transfer++)
                    for (uint32_t quantise = 0; quantise < 2; quantise++)
                        for (uint32_t dither = 0; dither < 2; dither++) {
                            std::vector<uint8_t> out[3];
                            for (uint32_t fmt = 0; fmt < 3; fmt++) {
                                const float whites[3] = { 4.0f, 1e-30f, 1e30f };
                                for (int wi = 0; wi < ((tone == 1 || tone == 2) ? 3 : 1); wi++) {
                                    const RtwDisplay prm = { 0.8f, tone, whites[wi], transfer, 2.2f, quantise, dither, fmt };
                                    std::vector<uint8_t> o(n * pixel_bytes(fmt), 7);
                                    CHECK(rtw_display(frame.data(), w, h, &prm, o.data(), &st) == RTW_OK, "display %u x %u tone %u fmt %u", w, h, tone, fmt);
                                    calls++;
                                    if (wi == 0) out[fmt] = o;
                                }
                            }
                            for (size_t p = 0; p < n; p++) {
                                CHECK(std::memcmp(&out[0][3 * p], &out[1][4 * p], 3) == 0 && out[1][4 * p + 3] == 255, "RGBA8 is not RGB8 plus 255 at %zu", p);
                            }
                        }
            {   // plain: rtw_quantize_u8's bytes
                const RtwDisplay prm = { 1.0f, RTW_TONE_NONE, 1.0f, RTW_TRANSFER_GAMMA, 1.0f, RTW_QUANTISE_RUST, 0, RTW_DISPLAY_RGB8 };
                std::vector<uint8_t> o(3 * n, 7), q(3 * n, 9);
                CHECK(rtw_display(frame.data(), w, h, &prm, o.data(), nullptr) == RTW_OK, "plain display");
                rtw_quantize_u8(frame.data(), 3 * n, q.data());
                CHECK(o == q, "plain display is not rtw_quantize_u8 at %u x %u", w, h);
                calls++;
            }
        }

    // -- refusals: nothing written
    {
        const uint32_t w = 5, h = 3;
        std::vector<float> frame = make_frame(w, h, false);
        std::vector<uint32_t> hist(256, 7u), counts(2, 7u);
        auto hist_refused = [&](const float *in, uint32_t ww, uint32_t hh, uint32_t *hi, uint32_t *co) {
            CHECK(rtw_luminance_histogram(in, ww, hh, hi, co, nullptr) == RTW_E_INVALID, "histogram not refused");
            CHECK(all_are(hist, 7u) && all_are(counts, 7u), "a refused histogram wrote");
            calls++;
        };
        hist_refused(nullptr, w, h, hist.data(), counts.data());
        hist_refused(frame.data(), w, h, nullptr, counts.data());
        hist_refused(frame.data(), w, h, hist.data(), nullptr);
        hist_refused(frame.data(), 0, h, hist.data(), counts.data());
        hist_refused(frame.data(), w, 0, hist.data(), counts.data());
        hist_refused(frame.data(), RTW_ATROUS_MAX_SIDE + 1, 1, hist.data(), counts.data());
        hist_refused(frame.data(), 0x10000u, 0x10000u, hist.data(), counts.data());
        std::vector<float> big(20 * 20 * 3, 0.5f);
        hist_refused(big.data(), 20, 20, (uint32_t *)(big.data() + 16), counts.data());
        hist_refused(big.data(), 20, 20, hist.data(), (uint32_t *)(big.data() + 1198));
        CHECK(all_are(big, 0.5f), "a refused histogram wrote into the frame");

        std::vector<uint8_t> out((size_t)w * h * 12, 7);
        const RtwDisplay ok = { 1.0f, RTW_TONE_ACES_FIT, 4.0f, RTW_TRANSFER_SRGB, 2.2f, RTW_QUANTISE_RUST, 0, RTW_DISPLAY_RGB8 };
        auto refused = [&](const float *in, uint32_t ww, uint32_t hh, const RtwDisplay *p, void *o) {
            CHECK(rtw_display(in, ww, hh, p, o, nullptr) == RTW_E_INVALID, "display not refused");
            CHECK(all_are(out, (uint8_t)7), "a refused display wrote");
            calls++;
        };
        refused(nullptr, w, h, &ok, out.data());
        refused(frame.data(), w, h, nullptr, out.data());
        refused(frame.data(), w, h, &ok, nullptr);
        refused(frame.data(), 0, h, &ok, out.data());
        refused(frame.data(), w, 0, &ok, out.data());
        refused(frame.data(), RTW_ATROUS_MAX_SIDE + 1, 1, &ok, out.data());
        refused(frame.data(), 0x10000u, 0x10000u, &ok, out.data());
        auto with = [&](auto set) { RtwDisplay p = ok; set(p); refused(frame.data(), w, h, &p, out.data()); };
        for (float e : { -1.0f, NaN, Inf }) with([&](RtwDisplay &p) { p.exposure = e; });
        for (float g : { 0.0f, -2.0f, NaN, Inf, 1e-40f }) with([&](RtwDisplay &p) { p.gamma = g; });
        for (uint32_t tone : { 1u, 2u })
            for (float wh : { 0.0f, -1.0f, NaN, Inf }) with([&](RtwDisplay &p) { p.tone = tone; p.white = wh; });
        with([](RtwDisplay &p) { p.tone = 4; });
        with([](RtwDisplay &p) { p.transfer = 2; });
        with([](RtwDisplay &p) { p.quantise = 2; });
        with([](RtwDisplay &p) { p.out_format = 3; });
        with([](RtwDisplay &p) { p.dither = 2; });
        for (uint32_t fmt = 0; fmt < 3; fmt++) {           // out overlapping in: in place, a byte in, the last byte
            std::vector<float> buf((size_t)w * h * 3 + 64, 0.5f);
            RtwDisplay p = ok;
            p.out_format = fmt;
            for (size_t off : { (size_t)0, (size_t)1, (size_t)w * h * 12 - 1 }) {
                CHECK(rtw_display(buf.data(), w, h, &p, (uint8_t *)buf.data() + off, nullptr) == RTW_E_INVALID, "overlap not refused");
                calls++;
            }
            CHECK(all_are(buf, 0.5f), "a refused display wrote into its frame");
        }

        double level = 7.0;
        float exposure = 7.0f;
        const RtwMetering good = { 50, 50, 0.18f, 1.0f, 0.0f, 256.0f };
        std::vector<uint32_t> hh(256, 3u);
        auto m_refused = [&](const uint32_t *hi, const RtwMetering *m, double prev, double *lv, float *ex) {
            CHECK(rtw_exposure_from_histogram(hi, m, prev, 1.0f, lv, ex) == RTW_E_INVALID, "metering not refused");
            CHECK(level == 7.0 && exposure == 7.0f, "a refused metering wrote");
            calls++;
        };
        const double first = std::numeric_limits<double>::quiet_NaN();
        m_refused(nullptr, &good, first, &level, &exposure);
        m_refused(hh.data(), nullptr, first, &level, &exposure);
        m_refused(hh.data(), &good, first, nullptr, &exposure);
        m_refused(hh.data(), &good, first, &level, nullptr);
        const RtwMetering bad[] = { { 500, 500, 0.18f, 1.0f, 0.0f, 256.0f }, { 0xFFFFFFFFu, 2, 0.18f, 1.0f, 0.0f, 256.0f }, { 50, 50, 0.0f, 1.0f, 0.0f, 256.0f },
                                    { 50, 50, NaN, 1.0f, 0.0f, 256.0f }, { 50, 50, Inf, 1.0f, 0.0f, 256.0f }, { 50, 50, 0.18f, -0.1f, 0.0f, 256.0f },
                                    { 50, 50, 0.18f, 1.5f, 0.0f, 256.0f }, { 50, 50, 0.18f, NaN, 0.0f, 256.0f }, { 50, 50, 0.18f, 1.0f, -1.0f, 256.0f },
                                    { 50, 50, 0.18f, 1.0f, 0.0f, 257.0f }, { 50, 50, 0.18f, 1.0f, NaN, 256.0f }, { 50, 50, 0.18f, 1.0f, 10.0f, 9.0f } };
        for (const RtwMetering &m : bad) m_refused(hh.data(), &m, first, &level, &exposure);
        for (double prev : { -1.0, 256.5, (double)Inf, -(double)Inf }) m_refused(hh.data(), &good, prev, &level, &exposure);
    }

    std::printf("display_sanitize: %d calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
