"""The host forms of the neighbourhood colour bounds and of the bounded temporal accumulation (rtw_colour_bounds,
rtw_temporal_accumulate_bounded, include/rtw.h) against numpy restatements, bit for bit (tests/bounds_common.py), their
known answers, a float64 check with a bound derived from the roundings, the edge values, every refusal, and the two behaviours the feature
is for: a firefly is clamped to its neighbourhood, and a history whose lighting stepped is clipped to the new frame.  No GPU."""
import numpy as np
import pytest

import rtw_amd as R
from tests.bounds_common import (BOUNDED_CASES, BOUNDED_KEYS, F, FLAGS, I32_MAX, I32_MIN, KS, RADII, SHAPES, assert_same_outputs, bounded_case,
                                 case_bounds, check_bounded_refusals, check_bounds_refusals, edge_frame, edge_pixels, host_bounded, host_bounds,
                                 inputs, lighting_step, mismatch, raw_null_bounds_vs_points, restate_bounds, run_bounded, run_bounded_restated,
                                 same_bits, small_places, taps_inside)

SHAPE_IDS = lambda s: f"{s[1]}x{s[0]}"


# ---- 1. the bounds against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_host_form_is_the_restated_rule(shape):
    h, w = shape
    fr, ids = inputs(h, w)
    for radius in RADII:
        for k in KS:
            for same, excl in FLAGS:
                got = host_bounds(h, w, radius, k, same, excl)
                want = restate_bounds(fr, ids, radius, k, same, excl)
                for name, g, x in zip(("lo", "hi", "clamped"), got, want):
                    assert same_bits(g, x), (radius, k, same, excl, name, mismatch(g, x))
                assert got[3] == taps_inside(h, w, radius)


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------------------
def test_a_constant_frame_has_a_box_of_no_width():
    """The sums 0.75 n are exact for every n <= 49, so mu = 0.75, every d = 0 and lo == hi == 0.75, whatever k."""
    fr = np.full((9, 11, 3), 0.75, F)
    for radius in RADII:
        for k in (0.0, 3.0, 1e38):
            for excl in (False, True):
                lo, hi, cl, _ = R.colour_bounds(fr, radius=radius, k=k, exclude_centre=excl, out_clamped=True)
                assert (lo == F(0.75)).all() and (hi == F(0.75)).all() and (cl == F(0.75)).all()


def test_a_constant_frame_at_every_tap_count():
    """Every n from 1 to 49: the pixels of 1 x N and N x 1 strips have 1 .. 7 taps (0 .. 6 with exclude_centre, and 0 gives (-inf, +inf)),
    and pixel (y, x) of a 7 x 7 frame at radius 3 has (min(y, 3) + min(6 - y, 3) + 1) * (min(x, 3) + min(6 - x, 3) + 1) taps -- 16, 20, 24,
    25, 28, 30, 35, 36, 42, 49 -- ; the remaining counts come from an object of exactly n pixels in a 7 x 7 frame under same_object, whose
    centre-most pixel sees all of them."""
    seen = set()
    for shape in ((1, 13), (13, 1), (7, 7)):
        fr = np.full(shape + (3,), 0.75, F)
        for radius in RADII:
            for excl in (False, True):
                lo, hi, _, _ = R.colour_bounds(fr, radius=radius, k=3.0, exclude_centre=excl)
                ones = np.ones(shape, np.int64)
                pad = np.pad(ones, radius)
                n = sum(pad[radius + dy:radius + dy + shape[0], radius + dx:radius + dx + shape[1]] for dy in range(-radius, radius + 1)
                        for dx in range(-radius, radius + 1)) - (1 if excl else 0)
                seen |= set(n.reshape(-1).tolist())
                some = n > 0
                assert (lo[some] == F(0.75)).all() and (hi[some] == F(0.75)).all()
                assert (lo[~some] == -np.inf).all() and (hi[~some] == np.inf).all()
    for n in range(1, 50):                                                # an object of n pixels about the centre of a 7 x 7 frame
        order = sorted(range(49), key=lambda i: (max(abs(i // 7 - 3), abs(i % 7 - 3)), i))
        ids = np.ones(49, np.int32)
        ids[order[:n]] = 5
        fr = np.repeat(np.where(ids == 5, F(0.75), F(0.25))[:, None], 3, 1).astype(F).reshape(7, 7, 3)
        lo, hi, _, _ = R.colour_bounds(fr, ids=ids.reshape(7, 7), radius=3, k=3.0, same_object=True)
        assert (lo[3, 3] == F(0.75)).all() and (hi[3, 3] == F(0.75)).all(), n
        seen.add(n)
    assert set(range(1, 50)) <= seen


def test_one_pixel_frames_and_one_pixel_objects():
    x = np.array([[[0.3, 7.0, -2.5]]], F)
    lo, hi, cl, st = R.colour_bounds(x, radius=3, k=2.0, out_clamped=True)
    assert same_bits(lo, x) and same_bits(hi, x) and same_bits(cl, x) and st.taps == 1
    lo, hi, cl, _ = R.colour_bounds(x, radius=3, k=2.0, exclude_centre=True, out_clamped=True)
    assert (lo == -np.inf).all() and (hi == np.inf).all() and same_bits(cl, x)
    fr, _ = inputs(4, 5)
    ids = np.zeros((4, 5), np.int32)
    ids[2, 2] = 9                                                        # an object of one pixel
    lo, hi, cl, _ = R.colour_bounds(fr, ids=ids, radius=2, k=1.0, same_object=True, exclude_centre=True, out_clamped=True)
    assert (lo[2, 2] == -np.inf).all() and (hi[2, 2] == np.inf).all() and same_bits(cl[2, 2], fr[2, 2])
    assert np.isfinite(lo[0, 0]).all()


# ---- 3. float64 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
def test_bounds_agree_with_float64_within_the_roundings(radius):
    """Frames of the integers 0 .. 255 (M = 255), n <= 49 taps, u = 2^-24 the unit roundoff of float32.  The bound, per pixel:
      s:   exact (49 * 255 < 2^24);   mu = s / nf:  one rounding, |dmu| <= M u
      d = x - mu:  |dd| <= |dmu| + M u = 2 M u;   d*d:  <= 2 M |dd| + |dd|^2 + M^2 u  <=  5.01 M^2 u
      qq: n terms of at most 5.01 M^2 u each, and n additions that each round a partial sum of at most n M^2:  <= (5.01 n + n^2) M^2 u
      v = qq / nf:  |dv| <= (5.01 + n) M^2 u + M^2 u = (n + 6.01) M^2 u
      sd = sqrt(v):  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |dv| / sd64, and <= sqrt(|dv|) always;  plus M u for its rounding
      e = k sd:  k |dsd| + k M u;     lo, hi = mu -+ e:  |dmu| + |de| + (M + k M) u."""
    k = 2.0
    rng = np.random.default_rng(77 + radius)
    h, w = 9, 12
    fr = rng.integers(0, 256, (h, w, 3)).astype(F)
    fr[4, 5:8] = 200.0                                                   # (a run of equal pixels: some windows are nearly flat)
    lo, hi, _, _ = R.colour_bounds(fr, radius=radius, k=k)
    M, u = 255.0, 2.0 ** -24
    f64 = fr.astype(np.float64)
    worst = 0.0
    for y in range(h):
        for x in range(w):
            win = f64[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].reshape(-1, 3)
            n = len(win)
            mu, sd = win.mean(0), win.std(0)
            dv = (n + 6.01) * M * M * u
            dsd = np.minimum(np.sqrt(dv), dv / np.maximum(sd, 1e-300)) + M * u
            bound = M * u + (k * dsd + k * M * u) + (M + k * M) * u
            for got, want in ((lo[y, x], mu - k * sd), (hi[y, x], mu + k * sd)):
                err = np.abs(got.astype(np.float64) - want)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (y, x, got, want, bound)
    print(f"\n[bounds vs float64] radius {radius}: the largest error is {worst:.3f} of its bound")


# ---- 4. edge values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(edge_pixels())), ids=["nan", "+inf", "-inf", "3e38", "denormal", "-0"])
@pytest.mark.parametrize("shape", [(4, 5), (9, 3)], ids=SHAPE_IDS)
def test_edge_values_at_the_centre_in_one_neighbour_and_in_all(shape, which):
    """... with idx -1, INT32_MIN and INT32_MAX under them: the host form is the restated rule."""
    h, w = shape
    for places in small_places(h, w):
        fr, ids = edge_frame(h, w, places, which)
        for radius in (1, 3):
            for same, excl in FLAGS:
                got = host_bounds(h, w, radius, 1.0, same, excl, (places, which))
                want = restate_bounds(fr, ids, radius, 1.0, same, excl)
                for name, g, x in zip(("lo", "hi", "clamped"), got, want):
                    assert same_bits(g, x), (places, radius, same, excl, name, mismatch(g, x))


def test_what_the_edge_values_do():
    h, w = 4, 5
    centre = ((2, 2),)
    # a pixel with a channel that is not finite is no tap: every box is finite; that channel is written as it is, its finite channels (0.5,
    # above the field's 0.1 .. 0.3) are clamped per channel like any other
    for which in (0, 1, 2):
        fr, _ = edge_frame(h, w, centre, which)
        lo, hi, cl, _ = host_bounds(h, w, 1, 1.0, False, False, (centre, which))
        assert np.isfinite(lo).all() and np.isfinite(hi).all()
        bad = ~np.isfinite(fr[2, 2])
        assert bad.sum() == 1 and same_bits(cl[2, 2][bad], fr[2, 2][bad]) and same_bits(cl[2, 2][~bad], hi[2, 2][~bad])
    # 3e38: the squared deviations overflow, the bounds are not finite, out_clamped == in there
    fr, _ = edge_frame(h, w, centre, 3)
    lo, hi, cl, _ = host_bounds(h, w, 1, 1.0, False, False, (centre, 3))
    assert not np.isfinite(lo[1:4, 1:4]).any() and not np.isfinite(hi[1:4, 1:4]).any()
    assert same_bits(cl[1:4, 1:4], fr[1:4, 1:4])
    # idx -1, INT32_MIN, INT32_MAX are ids like any other
    ids = np.array([[-1, -1, I32_MIN, I32_MIN, I32_MAX]], np.int32)
    row = np.arange(15, dtype=F).reshape(1, 5, 3)
    lo, hi, _, _ = R.colour_bounds(row, ids=ids, radius=3, k=0.0, same_object=True)
    assert same_bits(lo[0, 0], (row[0, 0] + row[0, 1]) / F(2)) and same_bits(lo[0, 2], (row[0, 2] + row[0, 3]) / F(2)) and same_bits(lo[0, 4], row[0, 4])
    assert same_bits(lo, hi)


# ---- 5. the firefly ----------------------------------------------------------------------------------------------------------------------------
def test_a_firefly_is_clamped_to_its_neighbourhood():
    """One pixel of 1e4 in a field of values in [0.1, 0.2], exclude_centre, k = 3: the neighbours' mean is at most 0.2 and their standard
    deviation at most 0.05 (half the range), so the pixel ends at or below 0.2 + 3 * 0.05.  The field is a checkerboard of 0.1 and 0.2, so
    that every other pixel has both values among its neighbours, in a corner too (two of the other, one of its own: sigma 0.047), and lies
    within 3 sigma of their mean -- or has the firefly among them, and a sigma in the thousands -- and stays.  Without exclude_centre the
    box around a neighbour includes the firefly and contains that neighbour."""
    h, w = 9, 11
    jj, ii = np.mgrid[0:h, 0:w]
    fr = np.repeat(np.where((ii + jj) % 2 == 0, F(0.1), F(0.2))[..., None], 3, -1).astype(F)
    fr[4, 5] = 1e4
    for radius in RADII:
        lo, hi, cl, _ = R.colour_bounds(fr, radius=radius, k=3.0, exclude_centre=True, out_clamped=True)
        assert (cl[4, 5] <= F(0.2 + 3 * 0.05)).all() and (cl[4, 5] >= F(0.1)).all(), cl[4, 5]
        others = np.ones((h, w), bool)
        others[4, 5] = False
        assert same_bits(cl[others], fr[others])
        lo, hi, _, _ = R.colour_bounds(fr, radius=radius, k=3.0)
        assert (lo[4, 4] <= fr[4, 4]).all() and (fr[4, 4] <= hi[4, 4]).all() and (hi[4, 4] > 100.0).all()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_error_paths_host():
    check_bounds_refusals(R.lib().rtw_colour_bounds, ())
    check_bounded_refusals(R.lib().rtw_temporal_accumulate_bounded, ())


# ---- 7. the bounded accumulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box", "open", "nan", "cur", None])
@pytest.mark.parametrize("name", BOUNDED_CASES)
def test_bounded_host_form_is_the_restated_rule(name, kind):
    got, want = host_bounded(name, kind), run_bounded_restated(name, kind)
    assert_same_outputs(got, {k: want[k] for k in BOUNDED_KEYS}, (name, kind))
    if name == "first":
        assert (got["clipped"] == 0.0).all()
    elif kind == "box":
        assert (got["clipped"] > 0).mean() > 0.25, name                   # (the box is narrow: the clamp was at work)


@pytest.mark.parametrize("name", BOUNDED_CASES)
def test_open_and_nan_bounds_give_the_bytes_of_the_points_call(name):
    plain = run_bounded(R.temporal_accumulate, name, None, clipped=False)            # (all three new arguments None: the _points call)
    assert "clipped" not in plain
    for kind in ("open", "nan", None):
        got = host_bounded(name, kind)
        assert_same_outputs(got, plain, (name, kind))
        assert (got["clipped"] == 0.0).all()


@pytest.mark.parametrize("name", BOUNDED_CASES)
def test_the_c_call_with_the_three_new_pointers_null_is_the_points_call(name):
    """rtw_temporal_accumulate_bounded itself, through ctypes, hist_lo = hist_hi = out_clipped = NULL, against rtw_temporal_accumulate_points
    on the same inputs: the five outputs byte for byte."""
    got, want = raw_null_bounds_vs_points(R.lib().rtw_temporal_accumulate_bounded, R.lib().rtw_temporal_accumulate_points, (), name)
    for k, (g, x) in enumerate(zip(got, want)):
        assert same_bits(g, x), (name, k, mismatch(g, x))
        assert not (g == F(-77.0)).all(), (name, k)                      # (the call wrote)


@pytest.mark.parametrize("name", [n for n in BOUNDED_CASES if n != "first"])
def test_a_box_of_no_width_at_cur_gives_cur(name):
    """lo = hi = cur: out_color == cur exactly where cur is finite and the pixel has a history (h' = cur, cur + (cur - cur) a = cur), and
    out_clipped == sum |h - cur| with h the history's colour, which the open box leaves in out_color where cur does not enter -- and which
    the restatement gives everywhere."""
    frames, _, _ = bounded_case(name)
    cur = frames[-1]["cur"]
    got, open_ = host_bounded(name, "cur"), host_bounded(name, "open")
    fin = np.isfinite(cur).all(-1)
    hist = got["len"] > 1.0                                               # (a blended pixel: n_ = hlen + 1 > 1)
    assert hist.mean() > 0.5
    assert same_bits(got["color"][fin], cur[fin])
    want = run_bounded_restated(name, "cur")["clipped"]
    assert same_bits(got["clipped"], want) and (got["clipped"][hist & fin] > 0).any()
    for k in ("moments", "len", "variance"):
        assert same_bits(got[k], open_[k]), k                             # the bounds touch neither the moments nor the length


def test_a_lighting_step_is_followed_at_once():
    """Static camera, flat guides, eight flat frames of 0.25, then 0.75, alpha = 0: without bounds the ninth colour is 0.25 + 0.5 / 9; with
    the ninth frame's bounds (a flat frame: lo == hi == 0.75 for any k and radius) it is exactly 0.75 and out_clipped is 1.5 per pixel."""
    for radius, k in ((1, 0.0), (2, 1.0), (3, 1e38)):
        plain, bounded, clipped = lighting_step(R.temporal_accumulate, R.colour_bounds, radius=radius, k=k)
        assert np.allclose(plain, 0.25 + 0.5 / 9, rtol=0, atol=1e-6) and not np.any(plain == F(0.75))
        assert (bounded == F(0.75)).all(), bounded
        assert (clipped == F(1.5)).all(), clipped
