"""Temporal accumulation on the host (rtw_temporal_accumulate, include/rtw.h) against an independent numpy restatement of the
rule (tests/temporal_common.py), bit for bit or NaN on both sides: the first frame, a static camera (also against the running mean written
out), whole-pixel shifts whose reprojection is exact, turned and moved cameras, each test alone and all together, holes in the history,
non-finite pixels, the history cap, the blend floor, out_color == cur, and every refusal; and the reprojection -- of the host form and
of the restatement -- against float64 geometry (tests/temporal_geometry_common.py, where the measured bounds stand).  No GPU."""
import numpy as np
import pytest

import rtw_amd as R
from tests.temporal_common import (ALL_OFF, CASE_NAMES, F, OFFSET, SENTINEL, SHAPES, TEMPORAL_TEST_DEFAULTS, assert_same_runs, bad_pixel_places, cases, dyadic_camera, frame,
                                   host_answer, raw_call, refusal_calls, run_restated, same_bits)

from tests.temporal_geometry_common import (GEO_CASES, GEO_SHAPES, LEFT_OUT_MOST, POSITION_BOUND, POSITION_MEASURED, S_MEASURED, check_plane,
                                            check_probe, check_static_is_continuous, plane_case, position_error, probe_case, probe_restated,
                                            regions, RENDERED_UNDECIDED_MOST, analytic_guides, rendered_cameras, rendered_sets)
from tests.temporal_common import GEO_POSES

E_INVALID = -1                                                              # rtw.h
shape_ids = lambda s: f"{s[1]}x{s[0]}"


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_host_equals_restatement(shape, name):
    h, w = shape
    frames, params = cases(h, w)[name]
    assert_same_runs(host_answer(h, w, name), run_restated(frames, params), name)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_first_frame(shape):
    h, w = shape
    frames, _ = cases(h, w)["first"]
    o = host_answer(h, w, "first")[0]
    c = frames[0]["cur"]
    L = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
    assert same_bits(o["color"], c) and np.all(o["len"] == 1) and same_bits(o["moments"], np.stack([L, L * L], -1)) and np.all(o["variance"] >= 0)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_static_camera_is_the_running_mean(shape):
    """alpha = 0: after n frames the colour is h + (c - h) * (1 / n), frame by frame, and the length is n."""
    h, w = shape
    frames, _ = cases(h, w)["static3"]
    outs = host_answer(h, w, "static3")
    mean = frames[0]["cur"]
    for n, (fr, o) in enumerate(zip(frames, outs), 1):
        if n > 1:
            mean = mean + (fr["cur"] - mean) * (F(1) / F(n))
        assert same_bits(o["color"], mean) and np.all(o["len"] == n)


@pytest.mark.parametrize("k", [1, 3, -2])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_dyadic_shift_is_exact(shape, k):
    """Every operand of the reprojection is a dyadic rational, so fx == i - k and fy == j with no rounding at all: the history is the
    previous frame moved by k whole pixels, blended; the columns it does not cover start again."""
    h, w = shape
    frames, params = cases(h, w)[f"shift{k}"]
    re = run_restated(frames, params)[1]
    jj, ii = np.mgrid[0:h, 0:w]
    assert np.array_equal(re["fx"], (ii - k).astype(F)) and np.array_equal(re["fy"], jj.astype(F)) and np.all(re["s"] == 4)
    o = host_answer(h, w, f"shift{k}")[1]
    prev, cur = frames[0]["cur"], frames[1]["cur"]
    src = ii - k
    covered = (src >= 0) & (src < w) & (frames[0]["idx"][jj, np.clip(src, 0, w - 1)] == frames[1]["idx"])       # same_object is on
    hist = prev[jj, np.clip(src, 0, w - 1)]
    want = np.where(covered[..., None], hist + (cur - hist) * F(0.5), cur)
    assert same_bits(o["color"], want) and np.array_equal(o["len"], np.where(covered, 2, 1).astype(F))
    if w > abs(k):
        assert not covered[:, (0 if k > 0 else w - 1)].any()
    if w >= 33:
        assert covered.any()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_camera_turned_right_round_resets_everything(shape):
    h, w = shape
    frames, params = cases(h, w)["behind"]
    re = run_restated(frames, params)[1]
    assert np.all(re["s"] <= 0) and not re["cand"].any()
    o = host_answer(h, w, "behind")[1]
    assert np.all(o["len"] == 1) and same_bits(o["color"], frames[1]["cur"])


@pytest.mark.parametrize("shape", SHAPES[2:], ids=shape_ids)
def test_the_moved_cases_keep_some_history_and_lose_some(shape):
    """What the matrix above is worth: the moved cameras land between pixels, and each test rejects taps the others accept."""
    h, w = shape
    for name in ("turned", "dolly"):
        frames, params = cases(h, w)[name]
        re = run_restated(frames, params)[1]
        frac = re["fx"][re["cand"]] % 1
        assert re["cand"].any() and np.any(frac != 0), name
        assert 0 < (host_answer(h, w, name)[1]["len"] > 1).mean(), name
    got = {t: host_answer(h, w, f"terms-{t}")[1] for t in ("depth", "normal", "idx", "all")}
    frames, params = cases(h, w)["terms-all"]
    free = run_restated(frames, dict(params, **ALL_OFF))[1]["color"]
    for t, o in got.items():                                                   # (a rejected tap shows in the colour: the others are renormalised)
        assert 0 < (o["len"] > 1).mean() and not np.array_equal(o["color"], free), t
    assert len({o["color"].tobytes() for o in got.values()}) == 4


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_holes_and_bad_pixels(shape):
    h, w = shape
    o = host_answer(h, w, "holes-static")[1]
    flat = o["len"].reshape(-1)
    assert np.all(flat[::3] == 1) and np.all(np.isfinite(o["color"]))          # a hole starts again, and the NaN colours under it were not read
    b = host_answer(h, w, "bad-cur")
    assert b[0]["len"].reshape(-1)[0] == 0 and np.all(b[0]["moments"].reshape(-1, 2)[0] == 0)       # not finite, no history
    assert b[1]["len"].reshape(-1)[0] == 0                                     # ... never read as history by the next frame
    n = h * w
    if n >= 15:
        for at in bad_pixel_places(n, True)[1:]:                                # not finite, with a history: written back unchanged
            assert b[1]["len"].reshape(-1)[at] == 1 and same_bits(b[1]["color"].reshape(-1, 3)[at], b[0]["color"].reshape(-1, 3)[at])
            assert same_bits(b[1]["moments"].reshape(-1, 2)[at], b[0]["moments"].reshape(-1, 2)[at])
        assert b[1]["len"].reshape(-1)[1] == 2
    assert np.all(np.isfinite(b[2]["color"]))                                  # no bad sample got into what a later frame gathers


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_saturation_and_floor(shape):
    h, w = shape
    assert [float(o["len"].max()) for o in host_answer(h, w, "saturate")] == [1, 2, 2, 2]
    frames, _ = cases(h, w)["floor"]
    outs = host_answer(h, w, "floor")
    acc = frames[0]["cur"]
    for n, fr in enumerate(frames[1:], 2):
        acc = acc + (fr["cur"] - acc) * F(0.5)                                 # 1 / n <= 0.5 from the second frame on
        assert same_bits(outs[n - 1]["color"], acc) and np.all(outs[n - 1]["len"] == n)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_out_color_may_be_cur(shape):
    h, w = shape
    frames, params = cases(h, w)["turned"]
    want = host_answer(h, w, "turned")
    hist = None
    for fr, x in zip(frames, want):
        cur = fr["cur"].copy()
        hist, var, _ = R.temporal_accumulate(cur, fr["cam"], depth=fr["depth"], normal=fr["normal"], ids=fr["idx"], history=hist, out_color=cur,
                                             offset=OFFSET, **params)
        assert hist["color"] is cur and same_bits(cur, x["color"]) and same_bits(var, x["variance"])


def test_variance_may_be_null_and_a_guide_that_is_off():
    rc, outs, _ = raw_call(R.lib().rtw_temporal_accumulate, out_variance=None)
    assert rc == 0 and np.all(outs[3] == SENTINEL) and not np.any(outs[0] == SENTINEL)
    rc, _, _ = raw_call(R.lib().rtw_temporal_accumulate, normal_cos=0.0, same_object=0, depth_tol=0.0, normal=None, idx=None, prev_depth=None,
                        prev_normal=None, prev_idx=None)
    assert rc == 0


@pytest.mark.parametrize("name,change", refusal_calls(), ids=[n for n, _ in refusal_calls()])
def test_refusals(name, change):
    rc, outs, _ = raw_call(R.lib().rtw_temporal_accumulate, **change)
    assert rc == E_INVALID
    assert all(np.all(o == SENTINEL) for o in outs)


def test_python_arguments():
    fr = frame(3, 5, 0, dyadic_camera(3, 5))
    with pytest.raises(TypeError):
        R.temporal_accumulate(fr["cur"], fr["cam"], depth=fr["depth"], sigma=1.0)
    with pytest.raises(ValueError):
        R.temporal_accumulate(fr["cur"], fr["cam"], depth=fr["depth"][:2])
    assert set(R.TEMPORAL_DEFAULTS) == {"alpha", "alpha_moments", "max_history", "depth_tol", "normal_cos", "same_object"}
    hist, var, st = R.temporal_accumulate(fr["cur"], fr["cam"], depth=fr["depth"], **TEMPORAL_TEST_DEFAULTS)
    assert set(hist) == {"color", "moments", "len", "depth", "normal", "idx", "cam"} and var.shape == (3, 5) and st.taps == 60


# ---- the reprojection against float64 geometry (tests/temporal_geometry_common.py) ------------------------------------------------------
geo_ids = lambda c: f"{c[0]}-{c[1]}"


@pytest.mark.parametrize("shape", GEO_SHAPES, ids=shape_ids)
def test_the_restatement_stays_within_the_measured_deviations(shape):
    """What the bounds of the probe are derived from: the numpy restatement alone against the float64 reference, on every case -- positions
    within POSITION_MEASURED, s on the fronto-parallel plane within S_MEASURED of D, and at most 2 % of the pixels left out."""
    h, w = shape
    worst = worst_s = 0.0
    for cam_name, offset_name in GEO_CASES:
        c = probe_case(h, w, cam_name, offset_name)
        color, length, _ = probe_restated(c)
        inside, outside, left_out = regions(c)
        assert left_out.mean() <= LEFT_OUT_MOST and np.all(length[inside] == 1) and np.all(length[outside] == 0), (cam_name, offset_name)
        worst = max(worst, position_error(c, color)[0])
        p = plane_case(h, w, cam_name, offset_name)
        inside = regions(p)[0]
        assert regions(p)[2].mean() <= LEFT_OUT_MOST
        worst_s = max(worst_s, float(np.abs(probe_restated(p)[2].astype(np.float64)[inside] / p["D"] - 1.0).max()))
    print(f"\n[geometry] {w}x{h}: the restatement's largest position error {worst:.3g} px, largest |s / D - 1| {worst_s:.3g}")
    assert worst <= POSITION_MEASURED and worst_s <= S_MEASURED, (worst, worst_s)
    assert any((probe_case(h, w, c, "half")["s"] < 0).any() for c in GEO_POSES)      # (some case has points behind the previous camera)


@pytest.mark.parametrize("case", GEO_CASES, ids=geo_ids)
@pytest.mark.parametrize("shape", GEO_SHAPES, ids=shape_ids)
def test_reprojection_against_float64_geometry(shape, case):
    """fx, fy and the candidate test of the host form, read out through a ramp history, against the float64 solve."""
    h, w = shape
    check_probe(R.temporal_accumulate, probe_case(h, w, *case), f"host {w}x{h} {case}")


@pytest.mark.parametrize("case", GEO_CASES, ids=geo_ids)
@pytest.mark.parametrize("shape", GEO_SHAPES, ids=shape_ids)
def test_s_against_a_fronto_parallel_plane(shape, case):
    """s of the host form through the depth test: against prev_depth = D every candidate keeps its history under depth_tol = S_TOL, against
    D (1 + 8 S_TOL) none does."""
    h, w = shape
    check_plane(R.temporal_accumulate, plane_case(h, w, *case), f"host {w}x{h} {case}")


@pytest.mark.parametrize("cam_name", list(GEO_POSES))
@pytest.mark.parametrize("shape", GEO_SHAPES, ids=shape_ids)
def test_static_shortcut_is_continuous_with_the_general_path(shape, cam_name):
    h, w = shape
    check_static_is_continuous(R.temporal_accumulate, h, w, cam_name, f"host {w}x{h} {cam_name}")
    assert POSITION_BOUND < 1.0 / 64.0


def test_the_rendered_view_decides_most_of_its_pixels():
    """The float64 reference of tests/test_gpu_temporal.py's rendered check alone, on the guides it expects surface_map to write: both of its
    sets are populated and the undecided rest -- silhouettes, disocclusions, the frame's edge -- is at most a quarter of the frame."""
    cam, prev_cam = rendered_cameras()
    depth, idx = analytic_guides(cam, OFFSET)
    keep, reset = rendered_sets(cam, prev_cam, depth, idx, OFFSET)
    assert len(np.unique(idx)) >= 4 and keep.sum() > 100 and reset.sum() >= 8 and not (keep & reset).any()
    assert 1.0 - keep.mean() - reset.mean() <= RENDERED_UNDECIDED_MOST
