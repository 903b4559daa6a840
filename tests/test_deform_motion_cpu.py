"""Per-pixel motion on the host (rtw_tri_bary, rtw_mesh_local_rays, rtw_deform_motion, rtw_temporal_accumulate_points; include/rtw.h
"temporal accumulation with per-pixel motion"): each against a numpy float32 restatement bit for bit; with prev_point all NaN
or NULL the bytes of the _motion call, with and without rows; a pixel with both a row and a point follows the point; the chain held to
float64 geometry that shares nothing with it; a placed sheet that waves and moves end to end; the refusals; the tri and idx classes that
form no address.  What the tests share is tests/deform_motion_common.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.deform_motion_common import (DEFORM_GEO_CASES, DEFORM_NORMAL_MEASURED, DEFORM_NORMAL_TOL, DEFORM_POSITION_BOUND, DEFORM_POSITION_MEASURED,
                                        DEFORM_SIZES, I32_MAX, I32_MIN, MESH_ID, POINT_KEYS, POINT_SHAPES, QNAN, case_points, deform_case,
                                        deform_geo_case, e2e_check, e2e_host_guides, e2e_poses, host, idx_classes, measure_deform_bounds,
                                        normal_error, points_probe, position_error, restate_deform, restate_local_rays, restate_points,
                                        restate_tri_bary, synthetic_points, tri_classes)
from tests.temporal_common import F, OFFSET, SENTINEL, TEMPORAL_TEST_DEFAULTS, dyadic_camera, frame, mismatch, same_bits, turned
from tests.temporal_motion_common import TABLES, TERMS, class_answer, class_case, terms_id

shape_ids = lambda s: f"{s[1]}x{s[0]}"
E_INVALID = -1                                                              # rtw.h
WHICH = ("all", "alternating", "none", "edges")


# ---- 1. the three rules, restated --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in DEFORM_GEO_CASES if c[0] in ("orbit", "far")], ids=lambda c: "-".join(c))
def test_tri_bary_and_local_rays_equal_their_restatements(case):
    c = deform_geo_case(*case)
    g = c["g"]
    h, w = g["tri"].shape
    rays = R.pixel_rays(c["cam"], w, h, c["offset"])
    if c["cur_pose"] is not None:
        ids = g["idx"].ravel().copy()
        ids[::7] = I32_MAX                                                       # (rays without a placement are copied)
        local = R.mesh_local_rays(c["cur_pose"][None], ids, rays, MESH_ID)
        assert same_bits(local, restate_local_rays(c["cur_pose"][None], ids, rays, MESH_ID))
        rays = R.mesh_local_rays(c["cur_pose"][None], g["idx"], rays, MESH_ID)
    t = g["depth"].ravel()
    got = R.tri_bary(g["ouv"], rays, t, g["tri"])
    assert same_bits(got, restate_tri_bary(g["ouv"], rays, t, g["tri"])), mismatch(got, restate_tri_bary(g["ouv"], rays, t, g["tri"]))
    assert same_bits(got.reshape(h, w, 2), g["bary"])
    on = g["tri"].ravel() >= 0
    assert on.mean() > 0.25 and np.all(got[~on] == 0)
    assert np.all(got[on] >= 0) and np.all(got[on].sum(1) <= 1 + 1e-5)             # the hit test accepted these very numbers


def test_tri_bary_forms_no_address_from_a_tri_outside_the_list():
    ouv = np.random.default_rng(1).uniform(-1, 1, (5, 9)).astype(F)                # exactly n_tris rows
    tri = np.array(tri_classes(5), np.int32)
    rays = np.random.default_rng(2).uniform(-1, 1, (len(tri), 6)).astype(F)
    got = R.tri_bary(ouv, rays, np.ones(len(tri), F), tri)
    assert same_bits(got, restate_tri_bary(ouv, rays, np.ones(len(tri), F), tri))
    assert np.all(got[(tri < 0) | (tri >= 5)] == 0) and np.any(got != 0)


@pytest.mark.parametrize("placed", [False, True], ids=["unplaced", "placed"])
@pytest.mark.parametrize("n", DEFORM_SIZES + [35 * 67])
def test_deform_motion_equals_restatement(n, placed):
    c = deform_case(n, placed)
    point, normal = R.deform_motion(**c)
    want_p, want_n = restate_deform(**c)
    assert same_bits(point, want_p), mismatch(point, want_p)
    assert same_bits(normal, want_n), mismatch(normal, want_n)
    none = np.isnan(point[:, 0])
    assert np.all(point.view(np.uint32)[none] == 0x7fc00000) and np.all(normal.view(np.uint32)[none] == 0x7fc00000)
    if n >= 255:
        n_tris = len(c["prev_ouv"])
        assert set(tri_classes(n_tris)) <= set(c["tri"].tolist()) and 0 < none.mean() < 1
        out = (c["tri"] < 0) | (c["tri"] >= n_tris)
        assert np.all(none[out])
        degenerate = c["tri"] == n_tris // 2                                        # a finite point, a normal that is not finite
        if placed:
            assert set(idx_classes(c["first"], len(c["prev_poses"]))) <= set(c["idx"].tolist())
            k = c["idx"].astype(np.int64) - c["first"]
            assert np.all(none[(k < 0) | (k >= len(c["prev_poses"]) - 1)])           # (the last pose is refused)
            degenerate &= ~none
        else:
            assert np.array_equal(none, out)
        assert degenerate.any() and np.all(np.isfinite(point[degenerate])) and not np.any(np.isfinite(normal[degenerate]))


# ---- 2. the points rule of the temporal pass -------------------------------------------------------------------------------------------------
def run_points(accumulate, frames, params, rows, first, points, wrap=None, carried=True, prev_xy=True):
    """The frames through `accumulate` with the table and the points on every call: per frame a dict of POINT_KEYS (numpy)."""
    wrap = wrap or (lambda a: a)
    params = dict(dict(offset=OFFSET), **params)
    hist, outs = None, []
    for fr in frames:
        cur = wrap(fr["cur"].copy())
        hist, var, _ = accumulate(cur, fr["cam"], depth=wrap(fr["depth"]), normal=wrap(fr["normal"]), ids=wrap(fr["idx"]), history=hist, motion=rows,
                                  motion_first=first, out_prev_xy=True if prev_xy else None, prev_point=None if points is None else wrap(points[0]),
                                  carried_normal=wrap(points[1]) if carried and points is not None else None, **params)
        o = dict(color=host(hist["color"]).copy(), moments=host(hist["moments"]).copy(), len=host(hist["len"]).copy(), variance=host(var).copy())
        if prev_xy:
            o["prev_xy"] = host(hist["prev_xy"]).copy()
        outs.append(o)
    return outs


def run_points_restated(frames, params, rows, first, points, carried=True):
    prev, outs = None, []
    params = dict(dict(offset=OFFSET), **params)
    for fr in frames:
        o = restate_points(fr["cur"], fr["cam"], fr["depth"], fr["normal"], fr["idx"], prev, rows, first, points[0], points[1] if carried else None,
                           **params)
        prev = dict(color=o["color"], moments=o["moments"], len=o["len"], depth=fr["depth"], normal=fr["normal"], idx=fr["idx"], cam=fr["cam"])
        outs.append(o)
    return outs


def assert_same_point_runs(got, want, what, keys=POINT_KEYS):
    assert len(got) == len(want)
    for k, (g, x) in enumerate(zip(got, want)):
        for key in keys:
            assert same_bits(g[key], x[key]), (what, f"frame {k}", key, mismatch(g[key], x[key]))


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("moved_cam", [False, True], ids=["static-camera", "moved-camera"])
@pytest.mark.parametrize("shape", POINT_SHAPES, ids=shape_ids)
def test_points_rule_equals_restatement(shape, moved_cam, which):
    h, w = shape
    frames, rows, first = class_case(h, w, "first3", moved_cam)
    points = synthetic_points(h, w, 0, which)
    for tk, terms in enumerate(TERMS):
        params = dict(TEMPORAL_TEST_DEFAULTS, **terms)
        for table in (rows, None):
            for carried in (True, False):
                got = run_points(R.temporal_accumulate, frames, params, table, first, points, carried=carried)
                want = run_points_restated(frames, params, table, first, points, carried)
                assert_same_point_runs(got, want, (terms_id(terms), table is not None, carried))
        assert np.isnan(got[0]["prev_xy"]).all()                                  # the first frame
        if which == "none":
            assert_same_point_runs(got, class_answer(h, w, "first3", moved_cam, tk) if table is not None else got, "no point: the _motion call")
    if h * w >= 200 and which in ("all", "alternating"):
        kept = got[1]["len"] > 1
        has = ~np.isnan(points[0][..., 0])
        assert kept[has].any() and not kept[has].all()


@pytest.mark.parametrize("moved_cam", [False, True], ids=["static-camera", "moved-camera"])
@pytest.mark.parametrize("table", list(TABLES))
def test_without_points_the_bytes_of_the_motion_call(table, moved_cam):
    """prev_point all NaN (carried_normal then never read, whatever it holds) or NULL: rtw_temporal_accumulate_motion's bytes, with rows and
    without."""
    h, w = 35, 67
    frames, rows, first = class_case(h, w, table, moved_cam)
    nan_points = (np.full((h, w, 3), QNAN), np.random.default_rng(3).random((h, w, 3)).astype(F))
    y_and_z_finite = nan_points[0].copy()
    y_and_z_finite[..., 1:] = 1.0                                                # only x decides
    for tk, terms in enumerate(TERMS):
        params = dict(TEMPORAL_TEST_DEFAULTS, **terms)
        want = class_answer(h, w, table, moved_cam, tk)
        for points in (nan_points, (y_and_z_finite, nan_points[1]), None):
            assert_same_point_runs(run_points(R.temporal_accumulate, frames, params, rows, first, points), want, (terms_id(terms), "rows"))
        without = run_points(R.temporal_accumulate, frames, params, None, first, None)
        assert_same_point_runs(run_points(R.temporal_accumulate, frames, params, None, first, nan_points), without, (terms_id(terms), "no rows"))


def test_a_pixel_with_a_row_and_a_point_follows_the_point():
    h, w = 35, 67
    frames, rows, first = class_case(h, w, "first0", True)
    points = synthetic_points(h, w, 1, "all")
    params = dict(TEMPORAL_TEST_DEFAULTS, **TERMS[0])
    with_rows = run_points(R.temporal_accumulate, frames, params, rows, first, points)
    no_rows = run_points(R.temporal_accumulate, frames, params, None, first, points)
    rows_alone = run_points(R.temporal_accumulate, frames, params, rows, first, None)
    assert_same_point_runs(with_rows, no_rows, "the row is ignored")
    assert not same_bits(with_rows[1]["prev_xy"], rows_alone[1]["prev_xy"])
    poisoned = rows.copy()
    poisoned["a"] = np.nan                                                       # (never read for a pixel with a point)
    assert_same_point_runs(run_points(R.temporal_accumulate, frames, params, poisoned, first, points), no_rows, "NaN rows")


def test_points_without_a_history_or_a_camera_move_take_four_taps():
    """Under a static camera a pixel with a point leaves the one-tap shortcut: its prev_xy is the point's projection, not (i, j)."""
    h, w = 9, 33
    frames, _, first = class_case(h, w, "first3", False)
    got = run_points(R.temporal_accumulate, frames, dict(TEMPORAL_TEST_DEFAULTS, **TERMS[0]), None, first, synthetic_points(h, w, 2, "alternating"))
    jj, ii = np.mgrid[0:h, 0:w]
    odd = (ii + jj) % 2 == 1
    grid = np.stack([ii, jj], -1).astype(F)
    assert np.array_equal(got[1]["prev_xy"][odd], grid[odd]) and not np.any(np.all(got[1]["prev_xy"][~odd] == grid[~odd], -1))


# ---- 3. float64 geometry ---------------------------------------------------------------------------------------------------------------------
def test_the_bounds_are_the_measured_ones():
    pos, nrm = measure_deform_bounds()
    assert 0.5 * DEFORM_POSITION_MEASURED < pos <= DEFORM_POSITION_MEASURED, pos
    assert 0.5 * DEFORM_NORMAL_MEASURED < nrm <= DEFORM_NORMAL_MEASURED, nrm


@pytest.mark.parametrize("case", DEFORM_GEO_CASES, ids=lambda c: "-".join(c))
def test_chain_against_float64_geometry(case):
    c = deform_geo_case(*case)
    point, carried = case_points(c)
    color, length, xy = points_probe(R.temporal_accumulate, c, point)
    ramp, direct = position_error(c, color, xy)
    cos = normal_error(c, carried)
    print(f"[deform geometry] {case}: largest position error {ramp:.3g} px by the ramp, {direct:.3g} px by prev_xy (bound "
          f"{DEFORM_POSITION_BOUND:.3g}), normal {cos:.3g} (tolerance {DEFORM_NORMAL_TOL:.3g})")
    assert ramp <= DEFORM_POSITION_BOUND and direct <= DEFORM_POSITION_BOUND, (case, ramp, direct)
    assert cos <= DEFORM_NORMAL_TOL, (case, cos)
    off = c["g"]["tri"] < 0
    assert off.any() and np.all(np.isnan(point[off])) and np.all(np.isnan(carried[off]))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_a_waving_sheet_keeps_its_history():
    """Recorded (deform_motion_common's docstring): 3499 mesh pixels, 3348 interior, all 3348 keep a history with points, 3166 (0.9456)
    without.  e2e_check asserts the conditions; the counts themselves may move by a pixel with the platform's sin and cos."""
    g0, g1 = e2e_host_guides()
    pp, _ = e2e_poses()
    point, carried = R.deform_motion(g1["tri"], g1["bary"], g0["ouv"], g1["idx"], pp, MESH_ID)
    _, counts = e2e_check(R.temporal_accumulate, g0, g1, point, carried, "host forms")
    assert counts["interior"] >= 0.9 * counts["mesh"] and counts["kept_without"] >= 0.5 * counts["interior"]      # (what the record says, loosely)


# ---- 5. the refusals ---------------------------------------------------------------------------------------------------------------------------
def deform_raw_call(fn, head=(), placed=True, **change):
    """One call of rtw_deform_motion (or the context's, after `head`) on 6 pixels, `change` applied: a buffer name -> None (NULL), or n,
    n_tris, n_mesh -> the value.  (status, the two outputs), filled with SENTINEL beforehand."""
    C = R.C
    c = deform_case(6, True)
    buf = dict(tri=c["tri"], bary=c["bary"], prev_ouv=c["prev_ouv"], idx=c["idx"] if placed else None, prev_poses=c["prev_poses"] if placed else None,
               point=np.full((6, 3), SENTINEL), normal=np.full((6, 3), SENTINEL))
    size = dict(n=6, n_tris=len(c["prev_ouv"]), n_mesh=len(c["prev_poses"]) if placed else 0)
    for k, v in change.items():
        if k in size:
            size[k] = v
        else:
            buf[k] = v
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = fn(*head, ptr(buf["tri"]), ptr(buf["bary"]), size["n"], ptr(buf["prev_ouv"]), size["n_tris"], ptr(buf["idx"]), ptr(buf["prev_poses"]),
            size["n_mesh"], c["first"], ptr(buf["point"]), ptr(buf["normal"]))
    return rc, [a for a in (buf["point"], buf["normal"]) if a is not None]


DEFORM_REFUSALS = [(f"{k} is NULL", {k: None}) for k in ("tri", "bary", "prev_ouv", "point", "normal")] + \
                  [("n is 0", dict(n=0)), ("n_tris is 0", dict(n_tris=0)), ("poses without idx", dict(idx=None)), ("poses, n_mesh 0", dict(n_mesh=0)),
                   ("n_mesh beyond RTW_MAX_MESH_INSTANCES", dict(n_mesh=2 ** 31))]
DEFORM_ACCEPTED = [("as it is", {}), ("no poses: idx, n_mesh and first are not read", dict(placed=False, n_mesh=2 ** 31)),
                   ("idx without poses", dict(prev_poses=None))]


@pytest.mark.parametrize("name,change", DEFORM_REFUSALS, ids=[n for n, _ in DEFORM_REFUSALS])
def test_deform_refusals_write_nothing(name, change):
    rc, outs = deform_raw_call(R.lib().rtw_deform_motion, **change)
    assert rc == E_INVALID
    assert all(np.all(o == SENTINEL) for o in outs)


@pytest.mark.parametrize("name,change", DEFORM_ACCEPTED, ids=[n for n, _ in DEFORM_ACCEPTED])
def test_deform_calls_next_to_the_refusals_are_accepted(name, change):
    rc, outs = deform_raw_call(R.lib().rtw_deform_motion, **change)
    assert rc == 0 and not any(np.any(o == SENTINEL) for o in outs)


def points_raw_call(fn, head=(), point="point", carried="carried", prev_xy="xy", rows=True):
    """One call of rtw_temporal_accumulate_points (or the context's, after `head`) on a 5 x 3 frame with a history: point / carried the name
    of the buffer the argument points to (an output's name: aliased) or None.  (status, outputs by name), filled with SENTINEL beforehand."""
    C = R.C
    h, w = 3, 5
    A = dyadic_camera(h, w)
    f0, f1 = frame(h, w, 0, A), frame(h, w, 1, turned(A, 0.4))
    out = dict(color=np.full((h, w, 3), SENTINEL), moments=np.full((h, w, 2), SENTINEL), len=np.full((h, w), SENTINEL),
               variance=np.full((h, w), SENTINEL), xy=np.full((h, w, 2), SENTINEL))
    pt, cn = synthetic_points(h, w, 0, "all")
    named = dict(out, point=pt, carried=cn)
    keep = [np.ones((h, w, 2), F), np.ones((h, w), F), R.motion_rows(4)]
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    p = R.RtwTemporal(0.2, 0.2, 32, 0.05, 0.9, 1, (C.c_float * 2)(*OFFSET))
    st = R.RtwFilterStats()
    rc = fn(*head, ptr(f1["cur"]), w, h, C.byref(f1["cam"]), ptr(f1["depth"]), ptr(f1["normal"]), ptr(f1["idx"]), C.byref(f0["cam"]), ptr(f0["cur"]),
            ptr(keep[0]), ptr(keep[1]), ptr(f0["depth"]), ptr(f0["normal"]), ptr(f0["idx"]), C.byref(p), ptr(keep[2]) if rows else None, 4, 2,
            None if point is None else ptr(named[point]), None if carried is None else ptr(named[carried]), ptr(out["color"]), ptr(out["moments"]),
            ptr(out["len"]), ptr(out["variance"]), None if prev_xy is None else ptr(out[prev_xy]), C.byref(st))
    return rc, out


POINT_OUTPUTS = ("color", "moments", "len", "variance", "xy")
POINT_REFUSALS = [(f"prev_point is out_{k}", dict(point=k)) for k in POINT_OUTPUTS] + \
                 [(f"carried_normal is out_{k}", dict(carried=k)) for k in POINT_OUTPUTS] + \
                 [("carried_normal without prev_point", dict(point=None)), ("out_prev_xy is out_color", dict(prev_xy="color"))]
POINT_ACCEPTED = [("as it is", {}), ("no carried_normal", dict(carried=None)), ("neither", dict(point=None, carried=None)),
                  ("no rows, no prev_xy", dict(rows=False, prev_xy=None))]


@pytest.mark.parametrize("name,change", POINT_REFUSALS, ids=[n for n, _ in POINT_REFUSALS])
def test_points_refusals_write_nothing(name, change):
    rc, out = points_raw_call(R.lib().rtw_temporal_accumulate_points, **change)
    assert rc == E_INVALID
    assert all(np.all(v == SENTINEL) for v in out.values())


@pytest.mark.parametrize("name,change", POINT_ACCEPTED, ids=[n for n, _ in POINT_ACCEPTED])
def test_points_calls_next_to_the_refusals_are_accepted(name, change):
    rc, out = points_raw_call(R.lib().rtw_temporal_accumulate_points, **change)
    assert rc == 0 and not np.any(out["color"] == SENTINEL)


def test_python_wrappers_refuse_what_they_can_see():
    with pytest.raises(ValueError):
        R.deform_motion(np.zeros(4, np.int32), np.zeros((4, 2), F), np.zeros((2, 9), F), prev_poses=np.zeros((1, 7), F))      # poses without idx
    with pytest.raises(ValueError):
        R.deform_motion(np.zeros(4, np.int32), np.zeros((3, 2), F), np.zeros((2, 9), F))                                       # bary of another size
    with pytest.raises(ValueError):
        R.tri_bary(np.zeros((2, 9), F), np.zeros((4, 6), F), np.zeros(3, F), np.zeros(4, np.int32))
