// temporal_motion_sanitize.cpp -- a stand-alone driver for the host forms of temporal accumulation with moving objects under
// AddressSanitizer + UBSan (host code only, no GPU): rtw_mesh_instance_motion and rtw_temporal_accumulate_motion into heap blocks of
// exactly the documented sizes -- the table n_rows * 128 bytes, out_prev_xy 2 * w * h floats -- on frames of 1 x 1, 31 x 7, 33 x 9 and
// 67 x 35 pixels that hold every id class about the table in one frame (-1, first - 1, first, first + n_rows - 1, first + n_rows, INT32_MIN,
// INT32_MAX), with first = 0, first > 0, first + n_rows = 2^31 and n_rows = 1, static and moved cameras, every set of tests, rows that stand
// still, rows of NaN, invalid poses, out_color == cur, and every refusal.  Checked: without rows, with rows that do not move and with a
// table that covers no id the bytes of rtw_temporal_accumulate; a NaN row leaves its object without a history and every other pixel's
// bytes alone; a refusal writes nothing.  An id outside the table that formed an address would read outside the table's block: that is
// what the sanitizer is here to see.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc temporal-motion-asan
#include "rtw.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static float uniform() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (float)((double)(z >> 11) * 0x1p-53);
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); failures++; } } while (0)

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

static RtwCamera make_camera(uint32_t w, uint32_t h, float ox, float angle) {
    RtwCamera c;
    std::memset(&c, 0, sizeof c);
    const float a = 0x1p-6f, cs = std::cos(angle), sn = std::sin(angle);
    auto turn = [&](float x, float y, float z, float *o) { o[0] = cs * x + sn * z; o[1] = y; o[2] = -sn * x + cs * z; };
    c.origin[0] = ox;
    turn(-(float)w / 2 * a, (float)h / 2 * a, -1.0f, c.pixel00);
    turn(a, 0.0f, 0.0f, c.delta_u);
    turn(0.0f, -a, 0.0f, c.delta_v);
    return c;
}

// A heap block of exactly n elements (never a vector's capacity), so that one element past it is the sanitizer's
template <class T> struct Block {
    std::unique_ptr<T[]> p;
    size_t n;
    explicit Block(size_t n_) : p(n_ ? new T[n_] : nullptr), n(n_) {}
    Block(size_t n_, T v) : Block(n_) { for (size_t i = 0; i < n; i++) p[i] = v; }
    T *data() const { return p.get(); }
    T &operator[](size_t i) const { return p[i]; }
    bool same(const Block &o) const {
        if (n != o.n) return false;
        for (size_t i = 0; i < n; i++) {
            uint32_t a, b;
            std::memcpy(&a, &p[i], 4); std::memcpy(&b, &o.p[i], 4);
            if (a != b && !(p[i] != p[i] && o.p[i] != o.p[i])) return false;
        }
        return true;
    }
};

struct Frame {
    uint32_t w, h;
    RtwCamera cam;
    Block<float> rgb, depth, normal;
    Block<int32_t> idx;
    Frame(uint32_t w_, uint32_t h_, const RtwCamera &c, const std::vector<int32_t> &ids)
        : w(w_), h(h_), cam(c), rgb(3 * (size_t)w_ * h_), depth((size_t)w_ * h_), normal(3 * (size_t)w_ * h_), idx((size_t)w_ * h_) {
        for (size_t p = 0; p < (size_t)w * h; p++) {
            idx[p] = ids[(p % w / 3 + p / w / 2) % ids.size()];
            depth[p] = 3.5f + 0.3f * uniform();
            for (int c2 = 0; c2 < 3; c2++) { normal[3 * p + c2] = c2 == 2 ? 1.0f : 0.05f * uniform(); rgb[3 * p + c2] = 2.0f * uniform(); }
        }
    }
};

struct Outs {
    Block<float> color, moments, len, variance, xy;
    explicit Outs(size_t n) : color(3 * n, 7.0f), moments(2 * n, 7.0f), len(n, 7.0f), variance(n, 7.0f), xy(2 * n, 7.0f) {}
    bool untouched() const {
        for (const Block<float> *b : { &color, &moments, &len, &variance, &xy })
            for (size_t i = 0; i < b->n; i++) if ((*b)[i] != 7.0f) return false;
        return true;
    }
};

static int calls = 0;

// The second frame of a sequence onto the first's history, through the call with motion.  terms: 1 depth, 2 normal, 4 idx.
static int second(const Frame &f0, const Frame &f1, const Outs &h0, int terms, const RtwMotionRow *rows, uint32_t n_rows, uint32_t first, Outs &o,
                  bool want_xy, bool in_place = false) {
    RtwTemporal p = { 0.2f, 0.2f, 32u, terms & 1 ? 0.05f : 0.0f, terms & 2 ? 0.9f : 0.0f, terms & 4 ? 1u : 0u, { 0.5f, 0.5f } };
    const bool need_idx = (terms & 4) || rows;
    if (in_place) std::memcpy(o.color.data(), f1.rgb.data(), o.color.n * sizeof(float));
    calls++;
    return rtw_temporal_accumulate_motion(in_place ? o.color.data() : f1.rgb.data(), f1.w, f1.h, &f1.cam, f1.depth.data(),
                                          terms & 2 ? f1.normal.data() : nullptr, need_idx ? f1.idx.data() : nullptr, &f0.cam, h0.color.data(),
                                          h0.moments.data(), h0.len.data(), terms & 1 ? f0.depth.data() : nullptr, terms & 2 ? f0.normal.data() : nullptr,
                                          terms & 4 ? f0.idx.data() : nullptr, &p, rows, n_rows, first, o.color.data(), o.moments.data(), o.len.data(),
                                          o.variance.data(), want_xy ? o.xy.data() : nullptr, nullptr);
}

int main() {
    // ---- rtw_mesh_instance_motion: exactly n rows, random, equal, one bit apart and invalid poses -------------------------------------------
    for (uint32_t n : { 1u, 5u, 257u, 65536u }) {
        Block<float> prev(7 * (size_t)n), cur(7 * (size_t)n);
        for (size_t k = 0; k < 7 * (size_t)n; k++) { prev[k] = 20.0f * uniform() - 10.0f; cur[k] = k % 5 ? 20.0f * uniform() - 10.0f : prev[k]; }
        uint32_t want_bad = 0;
        for (uint32_t k = 0; k < n; k += 3) for (int c = 0; c < 7; c++) cur[7 * (size_t)k + c] = prev[7 * (size_t)k + c];      // stand still
        if (n >= 5) {
            cur[7 * 1 + 2] = NaN; prev[7 * 2 + 4] = Inf; for (int c = 3; c < 7; c++) cur[7 * 4 + c] = 0.0f;
            want_bad = 3;
        }
        Block<RtwMotionRow> rows(n);
        uint32_t bad = 99;
        CHECK(rtw_mesh_instance_motion(prev.data(), cur.data(), n, rows.data(), &bad) == RTW_OK, "mesh motion n = %u", n);
        CHECK(bad == want_bad, "n = %u: %u invalid poses, expected %u", n, bad, want_bad);
        for (uint32_t k = 0; k < n; k++) {
            CHECK(rows[k].moving == (k % 3 ? 1u : 0u), "n = %u: row %u moving %u", n, k, rows[k].moving);
            const bool invalid = n >= 5 && (k == 1 || k == 2 || k == 4);
            for (int c = 0; c < 9; c++) CHECK((rows[k].a[c] != rows[k].a[c]) == invalid, "n = %u: row %u a[%d] %a", n, k, c, rows[k].a[c]);
        }
        CHECK(rtw_mesh_instance_motion(prev.data(), cur.data(), n, rows.data(), nullptr) == RTW_OK, "n_invalid NULL");
    }
    {
        Block<float> p(7, 1.0f);
        Block<RtwMotionRow> r(1);
        std::memset(r.data(), 0x55, sizeof(RtwMotionRow));
        const RtwMotionRow before = r[0];
        CHECK(rtw_mesh_instance_motion(nullptr, p.data(), 1, r.data(), nullptr) == RTW_E_INVALID, "prev NULL");
        CHECK(rtw_mesh_instance_motion(p.data(), nullptr, 1, r.data(), nullptr) == RTW_E_INVALID, "cur NULL");
        CHECK(rtw_mesh_instance_motion(p.data(), p.data(), 1, nullptr, nullptr) == RTW_E_INVALID, "rows NULL");
        CHECK(rtw_mesh_instance_motion(p.data(), p.data(), 0, r.data(), nullptr) == RTW_E_INVALID, "n 0");
        CHECK(rtw_mesh_instance_motion(p.data(), p.data(), RTW_MAX_MESH_INSTANCES + 1, r.data(), nullptr) == RTW_E_INVALID, "n beyond the limit");
        CHECK(std::memcmp(&before, r.data(), sizeof before) == 0, "a refused call wrote");
    }

    // ---- rtw_temporal_accumulate_motion: every id class, table shape, camera and set of tests -----------------------------------------------
    const uint32_t shapes[4][2] = { { 1, 1 }, { 31, 7 }, { 33, 9 }, { 67, 35 } };
    const uint32_t tables[4][2] = { { 0u, 5u }, { 3u, 5u }, { 7u, 1u }, { 0x80000000u - 4u, 4u } };          // first, n_rows
    for (const auto &s : shapes)
        for (const auto &t : tables) {
            const uint32_t w = s[0], h = s[1], first = t[0], n_rows = t[1];
            const size_t n = (size_t)w * h;
            const int64_t f = first;
            std::vector<int32_t> ids = { -1, (int32_t)(f - 1), (int32_t)f, (int32_t)(f + n_rows - 1), std::numeric_limits<int32_t>::min(),
                                         std::numeric_limits<int32_t>::max(), 0, (int32_t)(f + n_rows / 2) };
            if (f + n_rows < 0x80000000ll) ids.push_back((int32_t)(f + n_rows));
            // the table, exactly n_rows rows: small motions about (0, 0, -3.5) from the host form, the last row of a longer table stands still
            Block<float> prev(7 * (size_t)n_rows), cur(7 * (size_t)n_rows);
            for (uint32_t k = 0; k < n_rows; k++) {
                const float q[7] = { 0.0f, 0.0f, -3.5f, 1.0f, 0.1f * uniform(), 0.1f * uniform(), 0.1f * uniform() };
                for (int c = 0; c < 7; c++) {
                    prev[7 * k + c] = q[c];
                    cur[7 * k + c] = (n_rows > 1 && k == n_rows - 1) ? q[c] : q[c] + (c < 3 ? 0.1f : 0.05f) * (uniform() - 0.5f);
                }
            }
            Block<RtwMotionRow> rows(n_rows), still(n_rows), nan_rows(n_rows);
            CHECK(rtw_mesh_instance_motion(prev.data(), cur.data(), n_rows, rows.data(), nullptr) == RTW_OK, "rows");
            CHECK(rtw_mesh_instance_motion(prev.data(), prev.data(), n_rows, still.data(), nullptr) == RTW_OK, "rows that stand still");
            for (uint32_t k = 0; k < n_rows; k++) { nan_rows[k] = rows[k]; }
            nan_rows[0].moving = 1u; nan_rows[0].a[4] = NaN;
            for (int moved = 0; moved < 2; moved++) {
                const RtwCamera A = make_camera(w, h, 0.0f, 0.0f), B = moved ? make_camera(w, h, 0.02f, 0.01f) : A;
                const Frame f0(w, h, A, ids), f1(w, h, B, ids);
                Outs h0(n);
                {   // the first frame: no history, prev_xy NaN
                    RtwTemporal p = { 0.2f, 0.2f, 32u, 0.05f, 0.9f, 1u, { 0.5f, 0.5f } };
                    CHECK(rtw_temporal_accumulate_motion(f0.rgb.data(), w, h, &A, f0.depth.data(), f0.normal.data(), f0.idx.data(), nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, nullptr, nullptr, &p, rows.data(), n_rows, first, h0.color.data(),
                                                         h0.moments.data(), h0.len.data(), h0.variance.data(), h0.xy.data(), nullptr) == RTW_OK, "first frame");
                    for (size_t q = 0; q < 2 * n; q++) CHECK(h0.xy[q] != h0.xy[q], "first frame: prev_xy %a", h0.xy[q]);
                    for (size_t q = 0; q < n; q++) CHECK(h0.len[q] == 1.0f, "first frame: length %a", h0.len[q]);
                    calls++;
                }
                for (int terms = 0; terms < 8; terms++) {
                    Outs old(n), none(n), stood(n), beyond(n), got(n), place(n), bad(n);
                    RtwTemporal p = { 0.2f, 0.2f, 32u, terms & 1 ? 0.05f : 0.0f, terms & 2 ? 0.9f : 0.0f, terms & 4 ? 1u : 0u, { 0.5f, 0.5f } };
                    CHECK(rtw_temporal_accumulate(f1.rgb.data(), w, h, &B, f1.depth.data(), terms & 2 ? f1.normal.data() : nullptr,
                                                  terms & 4 ? f1.idx.data() : nullptr, &A, h0.color.data(), h0.moments.data(), h0.len.data(),
                                                  terms & 1 ? f0.depth.data() : nullptr, terms & 2 ? f0.normal.data() : nullptr,
                                                  terms & 4 ? f0.idx.data() : nullptr, &p, old.color.data(), old.moments.data(), old.len.data(),
                                                  old.variance.data(), nullptr) == RTW_OK, "the existing call");
                    CHECK(second(f0, f1, h0, terms, nullptr, 0, 0, none, false) == RTW_OK, "no rows");
                    CHECK(second(f0, f1, h0, terms, still.data(), n_rows, first, stood, true) == RTW_OK, "rows that stand still");
                    // a table that covers no id of the frame: one row, at an id no pixel carries
                    const uint32_t away = (uint32_t)(f + n_rows + 1 < 0x80000000ll ? f + n_rows + 1 : 1);
                    CHECK(second(f0, f1, h0, terms, nan_rows.data(), 1, away, beyond, true) == RTW_OK, "a table beyond the ids");
                    for (const Outs *o : { &none, &stood, &beyond })
                        CHECK(o->color.same(old.color) && o->moments.same(old.moments) && o->len.same(old.len) && o->variance.same(old.variance),
                              "%u x %u first %u terms %d moved %d: other bytes than the existing call", w, h, first, terms, moved);
                    CHECK(second(f0, f1, h0, terms, rows.data(), n_rows, first, got, true) == RTW_OK, "rows");
                    CHECK(second(f0, f1, h0, terms, rows.data(), n_rows, first, place, true, true) == RTW_OK, "rows, out_color == cur");
                    CHECK(got.color.same(place.color) && got.len.same(place.len) && got.xy.same(place.xy), "out_color == cur gives other bytes");
                    CHECK(second(f0, f1, h0, terms, nan_rows.data(), n_rows, first, bad, true) == RTW_OK, "a NaN row");
                    for (size_t q = 0; q < n; q++) {
                        if (f1.idx[q] == (int32_t)f) {
                            CHECK(bad.len[q] == 1.0f && (bad.xy[2 * q] != bad.xy[2 * q] || bad.xy[2 * q + 1] != bad.xy[2 * q + 1]),
                                  "a NaN row kept a history at %zu: length %a", q, bad.len[q]);
                        } else {
                            uint32_t x, y;
                            std::memcpy(&x, &bad.len[q], 4); std::memcpy(&y, &got.len[q], 4);
                            CHECK(x == y, "a NaN row changed pixel %zu of another object", q);
                        }
                        CHECK(got.len[q] >= 1.0f && got.len[q] <= 2.0f, "length %a", got.len[q]);
                        if (!moved) {                                                 // the shortcut holds per pixel
                            const int64_t k = (int64_t)f1.idx[q] - f;
                            const bool has_row = k >= 0 && k < (int64_t)n_rows && rows[k].moving;
                            if (!has_row) CHECK(got.xy[2 * q] == (float)(q % w) && got.xy[2 * q + 1] == (float)(q / w), "static, no row: prev_xy at %zu", q);
                        }
                    }
                }
            }
        }

    {   // ---- the refusals of the calls with motion: nothing is written ------------------------------------------------------------------------
        const uint32_t w = 17, h = 9;
        const size_t n = (size_t)w * h;
        const RtwCamera A = make_camera(w, h, 0.0f, 0.0f), B = make_camera(w, h, 0.0f, 0.02f);
        const std::vector<int32_t> ids = { -1, 0, 1, 2 };
        const Frame f0(w, h, A, ids), f1(w, h, B, ids);
        Outs h0(n), o(n);
        RtwTemporal p = { 0.2f, 0.2f, 32u, 0.05f, 0.9f, 0u, { 0.5f, 0.5f } };
        CHECK(rtw_temporal_accumulate(f0.rgb.data(), w, h, &A, f0.depth.data(), f0.normal.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, &p, h0.color.data(), h0.moments.data(), h0.len.data(), nullptr, nullptr) == RTW_OK, "history");
        Block<RtwMotionRow> rows(2);
        Block<float> pose(14, 1.0f);
        CHECK(rtw_mesh_instance_motion(pose.data(), pose.data(), 2, rows.data(), nullptr) == RTW_OK, "rows");
        int refusals = 0;
        auto call = [&](const int32_t *idx, const RtwMotionRow *r, uint32_t n_rows, uint32_t first, float *xy, const RtwTemporal *prm) {
            return rtw_temporal_accumulate_motion(f1.rgb.data(), w, h, &B, f1.depth.data(), f1.normal.data(), idx, &A, h0.color.data(), h0.moments.data(),
                                                  h0.len.data(), f0.depth.data(), f0.normal.data(), nullptr, prm, r, n_rows, first, o.color.data(),
                                                  o.moments.data(), o.len.data(), o.variance.data(), xy, nullptr);
        };
        auto refused = [&](int rc, const char *what) {
            CHECK(rc == RTW_E_INVALID, "not refused: %s", what);
            CHECK(o.untouched(), "a refused call wrote: %s", what);
            refusals++;
        };
        refused(call(nullptr, rows.data(), 2, 0, o.xy.data(), &p), "rows without idx (same_object off)");
        refused(call(f1.idx.data(), rows.data(), 0, 0, o.xy.data(), &p), "n_rows 0");
        refused(call(f1.idx.data(), rows.data(), 2, 0x80000000u - 1u, o.xy.data(), &p), "first + n_rows beyond 2^31");
        refused(call(f1.idx.data(), rows.data(), 1, 0xFFFFFFFFu, o.xy.data(), &p), "first beyond 2^31");
        refused(call(f1.idx.data(), rows.data(), 2, 0, o.color.data(), &p), "out_prev_xy == out_color");
        refused(call(f1.idx.data(), rows.data(), 2, 0, o.moments.data(), &p), "out_prev_xy == out_moments");
        refused(call(f1.idx.data(), rows.data(), 2, 0, o.len.data(), &p), "out_prev_xy == out_len");
        refused(call(f1.idx.data(), nullptr, 0, 0, o.variance.data(), &p), "out_prev_xy == out_variance, no rows");
        refused(call(f1.idx.data(), rows.data(), 2, 0, o.xy.data(), nullptr), "params NULL (a refusal of the existing call)");
        RtwTemporal q = p; q.alpha = NaN;
        refused(call(f1.idx.data(), rows.data(), 2, 0, o.xy.data(), &q), "alpha NaN (a refusal of the existing call)");
        q = p; q.same_object = 1u;
        refused(call(f1.idx.data(), rows.data(), 2, 0, o.xy.data(), &q), "same_object without prev_idx (a refusal of the existing call)");
        CHECK(call(f1.idx.data(), rows.data(), 2, 0x80000000u - 2u, o.xy.data(), &p) == RTW_OK, "first + n_rows == 2^31 is accepted");
        CHECK(call(nullptr, nullptr, 0, 0xFFFFFFFFu, o.xy.data(), &p) == RTW_OK, "without rows, n_rows and first are not read");
        std::printf("temporal_motion_sanitize: %d refusals\n", refusals);
    }
    std::printf("temporal_motion_sanitize: %d accumulate calls, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
