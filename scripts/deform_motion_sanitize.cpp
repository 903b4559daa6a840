// deform_motion_sanitize.cpp -- a stand-alone driver for the host forms of per-pixel motion under AddressSanitizer + UBSan (host code only,
// no GPU): rtw_tri_bary, rtw_mesh_local_rays, rtw_deform_motion and rtw_temporal_accumulate_points into heap blocks of exactly the
// documented sizes -- prev_ouv exactly n_tris rows, the pose table exactly n_mesh poses, tri n, bary 2 n, prev_point and carried_normal
// 3 * w * h floats -- on frames of 1 x 1, 31 x 7, 33 x 9 and 67 x 35 pixels that hold, in one frame, every class of tri about [0, n_tris)
// and of idx about the pose table (-1, below, first, last, one beyond, INT32_MIN, INT32_MAX), unplaced and placed, with a refused pose, a
// degenerate triangle, points of NaN and of infinities, with and without rows and carried_normal, every set of tests, and every refusal.
// Checked: a pixel without a point holds the quiet NaN in all six floats; a degenerate triangle a finite point and no finite normal; with
// prev_point all NaN or NULL the bytes of rtw_temporal_accumulate_motion; a point that is not finite leaves its pixel without a history; a
// refusal writes nothing.  A tri or idx outside its range that formed an address would read outside its block: that is what the sanitizer
// is here to see.
//
//   build + run:  make -C raytracing-in-a-weekend_amd/csrc deform-motion-asan
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
static const int32_t I_MIN = std::numeric_limits<int32_t>::min(), I_MAX = std::numeric_limits<int32_t>::max();

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
    bool same(const Block &o) const { return n == o.n && (n == 0 || std::memcmp(p.get(), o.p.get(), n * sizeof(T)) == 0); }
    bool all(T v) const { for (size_t i = 0; i < n; i++) if (!(p[i] == v)) return false; return true; }
};

static bool quiet_nan(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b == 0x7fc00000u; }
static bool finite3(const float *x) { return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]); }

struct Outs {
    Block<float> color, moments, len, variance, xy;
    explicit Outs(size_t n) : color(3 * n, 7.0f), moments(2 * n, 7.0f), len(n, 7.0f), variance(n, 7.0f), xy(2 * n, 7.0f) {}
    bool untouched() const { return color.all(7.0f) && moments.all(7.0f) && len.all(7.0f) && variance.all(7.0f) && xy.all(7.0f); }
    bool same(const Outs &o, bool with_xy) const {
        return color.same(o.color) && moments.same(o.moments) && len.same(o.len) && variance.same(o.variance) && (!with_xy || xy.same(o.xy));
    }
};

int main() {
    int deform_calls = 0, accumulate_calls = 0, refusals = 0;
    const uint32_t shapes[4][2] = { { 1, 1 }, { 31, 7 }, { 33, 9 }, { 67, 35 } };
    const uint32_t n_tris = 11, n_mesh = 4, first = 3;
    const int64_t f = first;
    const std::vector<int32_t> tris = { -1, 0, (int32_t)n_tris / 2, (int32_t)n_tris - 1, (int32_t)n_tris, (int32_t)n_tris + 1, I_MIN, I_MAX, -2, 3 };
    const std::vector<int32_t> ids = { -1, (int32_t)(f - 1), (int32_t)f, (int32_t)(f + n_mesh - 2), (int32_t)(f + n_mesh - 1), (int32_t)(f + n_mesh), I_MIN,
                                       I_MAX, 0, (int32_t)(f + 1) };
    // the previous mesh, exactly n_tris rows in front of the cameras; row n_tris / 2 is degenerate (v = 2 u).  The poses, exactly n_mesh:
    // small turns about the origin; the last one is refused (a quaternion of zeros)
    Block<float> ouv(9 * (size_t)n_tris), poses(7 * (size_t)n_mesh);
    for (uint32_t k = 0; k < n_tris; k++) {
        const float row[9] = { uniform() - 0.5f, uniform() - 0.5f, -3.5f + 0.2f * uniform(), 0.3f + 0.2f * uniform(), 0.1f * uniform(), 0.05f * uniform(),
                               0.1f * uniform(), 0.3f + 0.2f * uniform(), 0.05f * uniform() };
        for (int c = 0; c < 9; c++) ouv[9 * k + c] = row[c];
    }
    for (int c = 0; c < 3; c++) ouv[9 * (n_tris / 2) + 6 + c] = 2.0f * ouv[9 * (n_tris / 2) + 3 + c];
    for (uint32_t k = 0; k < n_mesh; k++) {
        const float q[7] = { 0.05f * uniform(), 0.05f * uniform(), 0.05f * uniform(), 1.0f, 0.05f * uniform(), 0.05f * uniform(), 0.05f * uniform() };
        for (int c = 0; c < 7; c++) poses[7 * k + c] = (k == n_mesh - 1 && c >= 3) ? 0.0f : q[c];
    }

    for (const auto &s : shapes) {
        const uint32_t w = s[0], h = s[1];
        const size_t n = (size_t)w * h;
        Block<int32_t> tri(n), idx(n);
        Block<float> bary(2 * n), rays(6 * n), t(n);
        for (size_t p = 0; p < n; p++) {
            tri[p] = tris[(p % w / 2 + p / w) % tris.size()];
            idx[p] = ids[(p % w / 3 + p / w / 2) % ids.size()];
            bary[2 * p] = 1.2f * uniform() - 0.1f; bary[2 * p + 1] = 1.2f * uniform() - 0.1f;
            for (int c = 0; c < 6; c++) rays[6 * p + c] = 2.0f * uniform() - 1.0f;
            t[p] = 4.0f * uniform();
        }
        {   // ---- rtw_tri_bary and rtw_mesh_local_rays ------------------------------------------------------------------------------------------
            Block<float> b(2 * n, 7.0f), local(6 * n, 7.0f);
            CHECK(rtw_tri_bary(ouv.data(), n_tris, rays.data(), (uint32_t)n, t.data(), tri.data(), b.data()) == RTW_OK, "tri_bary");
            for (size_t p = 0; p < n; p++)
                if (tri[p] < 0 || tri[p] >= (int32_t)n_tris) CHECK(b[2 * p] == 0.0f && b[2 * p + 1] == 0.0f, "tri_bary: tri %d gives %a %a", tri[p], b[2 * p], b[2 * p + 1]);
            CHECK(rtw_mesh_local_rays(poses.data(), n_mesh, first, idx.data(), rays.data(), (uint32_t)n, local.data()) == RTW_OK, "local rays");
            for (size_t p = 0; p < n; p++) {
                const int64_t k = (int64_t)idx[p] - f;
                if (k < 0 || k >= (int64_t)n_mesh - 1) CHECK(std::memcmp(&local[6 * p], &rays[6 * p], 24) == 0, "local rays: idx %d is not a copy", idx[p]);
            }
        }
        // ---- rtw_deform_motion, unplaced and placed -----------------------------------------------------------------------------------------
        Block<float> point(3 * n, 7.0f), normal(3 * n, 7.0f), point_w(3 * n, 7.0f), normal_w(3 * n, 7.0f);
        CHECK(rtw_deform_motion(tri.data(), bary.data(), (uint32_t)n, ouv.data(), n_tris, idx.data(), poses.data(), n_mesh, first, point.data(),
                                normal.data()) == RTW_OK, "deform, placed");
        CHECK(rtw_deform_motion(tri.data(), bary.data(), (uint32_t)n, ouv.data(), n_tris, nullptr, nullptr, 0xFFFFFFFFu, 0xFFFFFFFFu, point_w.data(),
                                normal_w.data()) == RTW_OK, "deform, unplaced (idx, n_mesh and first are not read)");
        deform_calls += 2;
        for (size_t p = 0; p < n; p++) {
            const bool in_list = tri[p] >= 0 && tri[p] < (int32_t)n_tris;
            const int64_t k = (int64_t)idx[p] - f;
            const bool posed = k >= 0 && k < (int64_t)n_mesh - 1;
            for (int world = 0; world < 2; world++) {
                const float *x = (world ? point_w : point).data() + 3 * p, *nr = (world ? normal_w : normal).data() + 3 * p;
                const bool has = in_list && (world || posed);
                if (!has) {
                    bool q = true;
                    for (int c = 0; c < 3; c++) q = q && quiet_nan(x[c]) && quiet_nan(nr[c]);
                    CHECK(q, "%u x %u pixel %zu (tri %d idx %d, %s): not the quiet NaN", w, h, p, tri[p], idx[p], world ? "unplaced" : "placed");
                } else if (tri[p] == (int32_t)n_tris / 2) {
                    CHECK(finite3(x) && !std::isfinite(nr[0]) && !std::isfinite(nr[1]) && !std::isfinite(nr[2]), "a degenerate triangle at %zu", p);
                } else CHECK(finite3(x) && finite3(nr) && std::fabs(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2] - 1.0f) < 1e-5f, "a point at %zu", p);
            }
        }

        // ---- rtw_temporal_accumulate_points ------------------------------------------------------------------------------------------------
        Block<RtwMotionRow> rows(n_mesh);
        {
            Block<float> cur_poses(7 * (size_t)n_mesh);
            for (size_t k = 0; k < cur_poses.n; k++) cur_poses[k] = poses[k] + (k % 7 < 3 ? 0.05f * uniform() : 0.0f);
            CHECK(rtw_mesh_instance_motion(poses.data(), cur_poses.data(), n_mesh, rows.data(), nullptr) == RTW_OK, "rows");
        }
        // points with every kind of value: NaN in x (no point), NaN or an infinity in y or z alone, infinities, behind the camera, the origin
        Block<float> wild(3 * n), none(3 * n, NaN);
        const float specials[9][3] = { { NaN, 0, -3 }, { 0, NaN, -3 }, { 0, 0, NaN }, { Inf, 0, -3 }, { 0, -Inf, -3 }, { 0, 0, Inf }, { 0, 0, -Inf },
                                       { 0, 0, 3 }, { 0, 0, 0 } };
        for (size_t p = 0; p < n; p++)
            for (int c = 0; c < 3; c++) wild[3 * p + c] = p % 4 == 1 ? specials[p / 4 % 9][c] : point_w[3 * p + c];
        for (int moved = 0; moved < 2; moved++) {
            const RtwCamera A = make_camera(w, h, 0.0f, 0.0f), B = moved ? make_camera(w, h, 0.02f, 0.01f) : A;
            Block<float> rgb0(3 * n), rgb1(3 * n), depth0(n), depth1(n), nrm0(3 * n), nrm1(3 * n);
            for (size_t p = 0; p < n; p++) {
                depth0[p] = 3.5f + 0.3f * uniform(); depth1[p] = 3.5f + 0.3f * uniform();
                for (int c = 0; c < 3; c++) {
                    rgb0[3 * p + c] = 2.0f * uniform(); rgb1[3 * p + c] = 2.0f * uniform();
                    nrm0[3 * p + c] = nrm1[3 * p + c] = c == 2 ? 1.0f : 0.05f * uniform();
                }
            }
            Outs h0(n);
            RtwTemporal all_on = { 0.2f, 0.2f, 32u, 0.05f, 0.9f, 1u, { 0.5f, 0.5f } };
            CHECK(rtw_temporal_accumulate_points(rgb0.data(), w, h, &A, depth0.data(), nrm0.data(), idx.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr, &all_on, rows.data(), n_mesh, first, point_w.data(), normal_w.data(), h0.color.data(),
                                                 h0.moments.data(), h0.len.data(), h0.variance.data(), h0.xy.data(), nullptr) == RTW_OK, "first frame");
            accumulate_calls++;
            for (size_t q = 0; q < 2 * n; q++) CHECK(h0.xy[q] != h0.xy[q], "first frame: prev_xy %a", h0.xy[q]);
            for (int terms = 0; terms < 8; terms++)
                for (int with_rows = 0; with_rows < 2; with_rows++) {
                    RtwTemporal p = { 0.2f, 0.2f, 32u, terms & 1 ? 0.05f : 0.0f, terms & 2 ? 0.9f : 0.0f, terms & 4 ? 1u : 0u, { 0.5f, 0.5f } };
                    const bool need_idx = (terms & 4) || with_rows;
                    auto call = [&](const float *pt, const float *cn, Outs &o, bool motion_call) {
                        accumulate_calls++;
                        const float *nr = terms & 2 ? nrm1.data() : nullptr, *pd = terms & 1 ? depth0.data() : nullptr, *pn = terms & 2 ? nrm0.data() : nullptr;
                        const int32_t *id = need_idx ? idx.data() : nullptr, *pid = terms & 4 ? idx.data() : nullptr;
                        const RtwMotionRow *r = with_rows ? rows.data() : nullptr;
                        if (motion_call)
                            return rtw_temporal_accumulate_motion(rgb1.data(), w, h, &B, depth1.data(), nr, id, &A, h0.color.data(), h0.moments.data(),
                                                                  h0.len.data(), pd, pn, pid, &p, r, n_mesh, first, o.color.data(), o.moments.data(),
                                                                  o.len.data(), o.variance.data(), o.xy.data(), nullptr);
                        return rtw_temporal_accumulate_points(rgb1.data(), w, h, &B, depth1.data(), nr, id, &A, h0.color.data(), h0.moments.data(),
                                                              h0.len.data(), pd, pn, pid, &p, r, n_mesh, first, pt, cn, o.color.data(), o.moments.data(),
                                                              o.len.data(), o.variance.data(), o.xy.data(), nullptr);
                    };
                    Outs old(n), null_pt(n), nan_pt(n), got(n), bare(n), mixed(n);
                    CHECK(call(nullptr, nullptr, old, true) == RTW_OK, "the call with motion");
                    CHECK(call(nullptr, nullptr, null_pt, false) == RTW_OK, "prev_point NULL");
                    CHECK(call(none.data(), normal_w.data(), nan_pt, false) == RTW_OK, "prev_point all NaN");
                    CHECK(null_pt.same(old, true) && nan_pt.same(old, true), "%u x %u terms %d rows %d moved %d: other bytes than the call with motion", w, h,
                          terms, with_rows, moved);
                    CHECK(call(point_w.data(), normal_w.data(), got, false) == RTW_OK, "points");
                    CHECK(call(point_w.data(), nullptr, bare, false) == RTW_OK, "points without carried_normal");
                    CHECK(call(wild.data(), normal_w.data(), mixed, false) == RTW_OK, "points of every kind");
                    for (size_t q = 0; q < n; q++) {
                        CHECK(got.len[q] >= 1.0f && got.len[q] <= 2.0f && mixed.len[q] >= 1.0f && mixed.len[q] <= 2.0f, "length %a %a", got.len[q], mixed.len[q]);
                        if (q % 4 != 1) continue;
                        const int kind = (int)(q / 4 % 9);
                        if (kind == 0) {                                                 // NaN in x: the pixel of the call with motion
                            uint32_t x, y;
                            std::memcpy(&x, &mixed.len[q], 4); std::memcpy(&y, &old.len[q], 4);
                            CHECK(x == y && std::memcmp(&mixed.xy[2 * q], &old.xy[2 * q], 8) == 0, "NaN in x at %zu: not the pixel of the call with motion", q);
                        } else CHECK(mixed.len[q] == 1.0f, "a point of kind %d kept a history at %zu: length %a", kind, q, mixed.len[q]);
                    }
                }
        }
    }

    {   // ---- the refusals: nothing is written ---------------------------------------------------------------------------------------------------
        const uint32_t n = 6;
        Block<int32_t> tri(n, 1), idx(n, (int32_t)first);
        Block<float> bary(2 * n, 0.25f), point(3 * n, 7.0f), normal(3 * n, 7.0f), rays(6 * n, 1.0f), t(n, 1.0f), b(2 * n, 7.0f), local(6 * n, 7.0f);
        auto deform = [&](const int32_t *tr, const float *ba, uint32_t nn, const float *ov, uint32_t nt, const int32_t *id, const float *po, uint32_t nm,
                          float *pt, float *nr, const char *what) {
            CHECK(rtw_deform_motion(tr, ba, nn, ov, nt, id, po, nm, first, pt, nr) == RTW_E_INVALID, "not refused: %s", what);
            CHECK(point.all(7.0f) && normal.all(7.0f), "a refused call wrote: %s", what);
            refusals++;
        };
        deform(nullptr, bary.data(), n, ouv.data(), n_tris, idx.data(), poses.data(), n_mesh, point.data(), normal.data(), "tri NULL");
        deform(tri.data(), nullptr, n, ouv.data(), n_tris, idx.data(), poses.data(), n_mesh, point.data(), normal.data(), "bary NULL");
        deform(tri.data(), bary.data(), n, nullptr, n_tris, idx.data(), poses.data(), n_mesh, point.data(), normal.data(), "prev_ouv NULL");
        deform(tri.data(), bary.data(), n, ouv.data(), n_tris, idx.data(), poses.data(), n_mesh, nullptr, normal.data(), "prev_point NULL");
        deform(tri.data(), bary.data(), n, ouv.data(), n_tris, idx.data(), poses.data(), n_mesh, point.data(), nullptr, "carried_normal NULL");
        deform(tri.data(), bary.data(), 0, ouv.data(), n_tris, idx.data(), poses.data(), n_mesh, point.data(), normal.data(), "n 0");
        deform(tri.data(), bary.data(), n, ouv.data(), 0, idx.data(), poses.data(), n_mesh, point.data(), normal.data(), "n_tris 0");
        deform(tri.data(), bary.data(), n, ouv.data(), n_tris, nullptr, poses.data(), n_mesh, point.data(), normal.data(), "poses without idx");
        deform(tri.data(), bary.data(), n, ouv.data(), n_tris, idx.data(), poses.data(), 0, point.data(), normal.data(), "poses, n_mesh 0");
        deform(tri.data(), bary.data(), n, ouv.data(), n_tris, idx.data(), poses.data(), RTW_MAX_MESH_INSTANCES + 1, point.data(), normal.data(),
               "n_mesh beyond the limit");
        CHECK(rtw_deform_motion(tri.data(), bary.data(), n, ouv.data(), n_tris, idx.data(), nullptr, 0, first, point.data(), normal.data()) == RTW_OK,
              "idx without poses is accepted");
        CHECK(rtw_tri_bary(nullptr, n_tris, rays.data(), n, t.data(), tri.data(), b.data()) == RTW_E_INVALID, "tri_bary: ouv NULL");
        CHECK(rtw_tri_bary(ouv.data(), 0, rays.data(), n, t.data(), tri.data(), b.data()) == RTW_E_INVALID, "tri_bary: n_tris 0");
        CHECK(rtw_tri_bary(ouv.data(), n_tris, rays.data(), 0, t.data(), tri.data(), b.data()) == RTW_E_INVALID, "tri_bary: n 0");
        CHECK(rtw_tri_bary(ouv.data(), n_tris, rays.data(), n, t.data(), nullptr, b.data()) == RTW_E_INVALID, "tri_bary: tri NULL");
        CHECK(rtw_mesh_local_rays(nullptr, n_mesh, first, idx.data(), rays.data(), n, local.data()) == RTW_E_INVALID, "local rays: poses NULL");
        CHECK(rtw_mesh_local_rays(poses.data(), 0, first, idx.data(), rays.data(), n, local.data()) == RTW_E_INVALID, "local rays: n_mesh 0");
        CHECK(b.all(7.0f) && local.all(7.0f), "a refused call wrote");
        refusals += 6;

        const uint32_t w = 3, h = 2;
        const RtwCamera A = make_camera(w, h, 0.0f, 0.0f), B = make_camera(w, h, 0.0f, 0.02f);
        Block<float> rgb(3 * n, 0.5f), depth(n, 3.5f), nrm(3 * n, 0.0f), pt(3 * n, -3.5f), cn(3 * n, 0.0f);
        Outs h0(n), o(n);
        RtwTemporal p = { 0.2f, 0.2f, 32u, 0.05f, 0.9f, 0u, { 0.5f, 0.5f } };
        CHECK(rtw_temporal_accumulate(rgb.data(), w, h, &A, depth.data(), nrm.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      &p, h0.color.data(), h0.moments.data(), h0.len.data(), nullptr, nullptr) == RTW_OK, "history");
        auto points = [&](const float *point_, const float *carried, float *xy, const RtwTemporal *prm) {
            return rtw_temporal_accumulate_points(rgb.data(), w, h, &B, depth.data(), nrm.data(), nullptr, &A, h0.color.data(), h0.moments.data(),
                                                  h0.len.data(), depth.data(), nrm.data(), nullptr, prm, nullptr, 0, 0, point_, carried, o.color.data(),
                                                  o.moments.data(), o.len.data(), o.variance.data(), xy, nullptr);
        };
        auto refused = [&](int rc, const char *what) {
            CHECK(rc == RTW_E_INVALID, "not refused: %s", what);
            CHECK(o.untouched(), "a refused call wrote: %s", what);
            refusals++;
        };
        for (float *out : { o.color.data(), o.moments.data(), o.len.data(), o.variance.data(), o.xy.data() }) {
            refused(points(out, cn.data(), o.xy.data(), &p), "prev_point is an output");
            refused(points(pt.data(), out, o.xy.data(), &p), "carried_normal is an output");
        }
        refused(points(nullptr, cn.data(), o.xy.data(), &p), "carried_normal without prev_point");
        refused(points(pt.data(), cn.data(), o.color.data(), &p), "out_prev_xy == out_color (a refusal of the call with motion)");
        refused(points(pt.data(), cn.data(), o.xy.data(), nullptr), "params NULL (a refusal of the existing call)");
        CHECK(points(pt.data(), nullptr, nullptr, &p) == RTW_OK, "points alone are accepted");
    }
    std::printf("deform_motion_sanitize: %d deform calls, %d accumulate calls, %d refusals, %d failures\n", deform_calls, accumulate_calls, refusals,
                failures);
    return failures ? 1 : 0;
}
