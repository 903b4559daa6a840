"""Temporal accumulation with moving objects on the host (rtw_temporal_accumulate_motion, rtw_mesh_instance_motion; include/rtw.h "temporal
accumulation with moving objects"): without rows, with rows that do not move, with a table that covers no id and with
identity rows the bytes of rtw_temporal_accumulate; a numpy float32 restatement of the rule bit for bit at every id class, table shape,
term combination and camera; rtw_mesh_instance_motion against its own restatement; both held to float64 geometry that shares nothing with
them; two placements of an icosphere end to end; the refusals.  What the tests share is tests/temporal_motion_common.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.temporal_common import (ALL_ON, CASE_NAMES, F, OFFSET, SENTINEL, TEMPORAL_TEST_DEFAULTS, assert_same_runs, cases, dyadic_camera, frame,
                                   host_answer, mismatch, run, same_bits, turned)
from tests.temporal_motion_common import (E2E_FIRST, GEO_MOTION_CASES, I32_MAX, I32_MIN, MOTION_KEYS, MOTION_NORMAL_MEASURED, MOTION_POSITION_BOUND,
                                          MOTION_POSITION_MEASURED, MOTION_SHAPES, TABLES, TERMS, check_motion_geometry, class_answer, class_case,
                                          e2e_cameras, e2e_check, e2e_guides_host, e2e_poses, geo_motion_case, measure_motion_bounds, motion_probe,
                                          motion_regions, quat_axis, restate_mesh_motion, row_lookup, run_motion, run_motion_restated, terms_id,
                                          turned_normal)

shape_ids = lambda s: f"{s[1]}x{s[0]}"
OLD_SHAPE = (17, 33)
E_INVALID = -1                                                              # rtw.h


# ---- 1. the old bytes ----------------------------------------------------------------------------------------------------------------------
def _with_table(rows, first):
    return lambda *a, **k: R.temporal_accumulate(*a, motion=rows, motion_first=first, **k)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_without_moving_rows_the_bytes_of_the_existing_call(name):
    h, w = OLD_SHAPE
    frames, params = cases(h, w)[name]
    want = host_answer(h, w, name)
    ids = np.concatenate([fr["idx"].ravel() for fr in frames])
    assert_same_runs(run(lambda *a, **k: R.temporal_accumulate(*a, out_prev_xy=None, motion=None, **k), frames, params), want, "rows=None")
    assert_same_runs(run(lambda *a, **k: R.temporal_accumulate(*a, out_prev_xy=True, **k), frames, params), want, "prev_xy alone")
    assert_same_runs(run(_with_table(R.motion_rows(int(ids.max()) + 1), 0), frames, params), want, "rows that do not move")
    beyond = R.motion_rows(4)
    beyond["moving"] = 1
    beyond["a"] = np.nan                                                       # (never read: no id of the frame is in the table)
    assert_same_runs(run(_with_table(beyond, int(ids.max()) + 1), frames, params), want, "a table beyond every id")


MOVED_CAMERA_CASES = [n for n in CASE_NAMES if n in ("turned", "dolly", "behind", "holes-turned") or n.startswith(("terms-", "geo-"))]


@pytest.mark.parametrize("name", MOVED_CAMERA_CASES)
def test_identity_rows_that_move_give_the_old_bytes_under_a_moved_camera(name):
    """(P - 0) and 1 * x + 0 * y + 0 * z + 0 are exact for finite P, and under a moved camera every pixel takes the four taps anyway."""
    h, w = OLD_SHAPE
    frames, params = cases(h, w)[name]
    assert all(bytes(a["cam"]) != bytes(b["cam"]) for a, b in zip(frames, frames[1:]))
    ids = np.concatenate([fr["idx"].ravel() for fr in frames])
    rows = R.motion_rows(int(ids.max()) + 1)
    rows["moving"] = 1
    assert_same_runs(run(_with_table(rows, 0), frames, params), host_answer(h, w, name), name)


# ---- 2. the rule, restated -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved_cam", [False, True], ids=["static-camera", "moved-camera"])
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("shape", MOTION_SHAPES, ids=shape_ids)
def test_host_equals_restatement(shape, table, moved_cam):
    h, w = shape
    frames, rows, first = class_case(h, w, table, moved_cam)
    has_row, _ = row_lookup(frames[1]["idx"], rows, first)
    ids = set(frames[1]["idx"].ravel().tolist())
    if h * w >= 200:
        assert {-1, first - 1, first, first + len(rows) - 1, first + len(rows), I32_MIN, I32_MAX} <= ids     # every class in one frame
        assert 0 < has_row.mean() < 1
    for tk, terms in enumerate(TERMS):
        want = run_motion_restated(frames, dict(TEMPORAL_TEST_DEFAULTS, **terms), rows, first)
        got = class_answer(h, w, table, moved_cam, tk)
        for k, (g, x) in enumerate(zip(got, want)):
            for key in MOTION_KEYS:
                assert same_bits(g[key], x[key]), (terms_id(terms), f"frame {k}", key, mismatch(g[key], x[key]))
        assert np.isnan(got[0]["prev_xy"]).all()                                # the first frame
        if not moved_cam:                                                       # the shortcut holds per pixel
            jj, ii = np.mgrid[0:h, 0:w]
            assert np.array_equal(got[1]["prev_xy"][~has_row], np.stack([ii, jj], -1).astype(F)[~has_row])
        if h * w >= 200 and terms["same_object"] == 0 and terms["depth_tol"] == 0:
            assert (got[1]["len"][has_row] > 1).any() and (got[1]["len"][~has_row] > 1).any()


def test_out_color_may_be_cur_with_rows():
    h, w = 35, 67
    frames, rows, first = class_case(h, w, "first3", True)
    got = run_motion(R.temporal_accumulate, frames, dict(TEMPORAL_TEST_DEFAULTS, **TERMS[7]), rows, first, out_color_is_cur=True)
    for g, x in zip(got, class_answer(h, w, "first3", True, 7)):
        for key in MOTION_KEYS:
            assert same_bits(g[key], x[key]), key


@pytest.mark.parametrize("moved_cam", [False, True], ids=["static-camera", "moved-camera"])
@pytest.mark.parametrize("bad_sample", [False, True], ids=["finite", "bad-sample"])
def test_a_nan_row_costs_its_object_the_history_and_nothing_else(moved_cam, bad_sample):
    h, w = 35, 67
    frames, rows, first = class_case(h, w, "first3", moved_cam)
    _, nan_rows, _ = class_case(h, w, "first3", moved_cam, True)
    if bad_sample:
        frames = [frames[0], dict(frames[1], cur=frames[1]["cur"].copy())]
        frames[1]["cur"][::2, ::3, 1] = np.inf
    params = dict(TEMPORAL_TEST_DEFAULTS, **TERMS[0])                          # every term off: without the NaN every pixel in view keeps a history
    clean = run_motion(R.temporal_accumulate, frames, params, rows, first)[1]
    got = run_motion(R.temporal_accumulate, frames, params, nan_rows, first)[1]
    hit = frames[1]["idx"] == first
    fin = np.isfinite(frames[1]["cur"]).all(-1)
    assert hit.any() and (clean["len"][hit] > 1).any()
    assert np.all(got["len"][hit & fin] == 1) and np.all(got["len"][hit & ~fin] == 0)
    assert np.isnan(got["prev_xy"][hit]).any(-1).all()
    for key in MOTION_KEYS:
        assert same_bits(got[key][~hit], clean[key][~hit]), key
    want = run_motion_restated(frames, params, nan_rows, first)[1]
    for key in MOTION_KEYS:
        assert same_bits(got[key], want[key]), key


# ---- 3. rtw_mesh_instance_motion -------------------------------------------------------------------------------------------------------------
def _poses(n, seed):
    rng = np.random.default_rng(seed)
    p = np.empty((n, 7), F)
    p[:, :3] = rng.uniform(-50, 50, (n, 3))
    p[:, 3:] = rng.normal(size=(n, 4)) * rng.choice([1e-3, 1.0, 40.0], (n, 1))             # (unnormalised quaternions)
    return p


def test_mesh_instance_motion_equals_restatement():
    n = 300
    prev, cur = _poses(n, 1), _poses(n, 2)
    cur[10:20] = prev[10:20]                                                    # equal poses
    cur[20:27] = prev[20:27]
    for k in range(7):                                                          # poses that differ in one bit, component by component
        cur[20 + k, k] = np.nextafter(cur[20 + k, k], F(np.inf))
    cur[30, 2], prev[31, 0], cur[32, 4], prev[33, 6] = np.nan, np.inf, np.nan, -np.inf         # invalid on either side
    cur[34, 3:], prev[35, 3:] = 0.0, 0.0                                        # a quaternion of length 0
    cur[36, 3:] = 3e38                                                          # ... and one whose length overflows
    prev[37] = cur[37] = [1, 2, 3, np.nan, 0, 0, 1]                             # invalid, and equal byte for byte
    prev[38, 3:], cur[38, 3:] = (0.0, 0.0, 0.0, 1.0), (-0.0, 0.0, 0.0, 1.0)     # 0 and -0 are different bytes
    rows, bad = R.mesh_instance_motion(prev, cur)
    want, want_bad = restate_mesh_motion(prev, cur)
    assert rows.dtype == R.MOTION_ROW and bad == want_bad == 8
    for key in ("a", "from", "to", "nrm"):
        assert same_bits(rows[key], want[key]), (key, mismatch(rows[key], want[key]))
    assert np.array_equal(rows["moving"], want["moving"]) and not rows["pad"].any()
    still = np.r_[10:20, 37]
    assert not rows["moving"][still].any() and rows["moving"].sum() == n - len(still)
    assert np.array_equal(rows[still], R.motion_rows(len(still)))
    for k in (30, 31, 32, 33, 34, 35, 36):
        assert rows["moving"][k] == 1 and np.isnan(rows["a"][k]).all() and np.array_equal(rows["nrm"][k], np.eye(3, dtype=F))
    # the two matrices are rotations, and not each other's transpose: points and normals of a placement turn by different ones
    ok = np.ones(n, bool)
    ok[np.r_[10:20, 30:38]] = False
    a64, n64 = rows["a"][ok].astype(np.float64), rows["nrm"][ok].astype(np.float64)
    assert np.abs(a64 @ a64.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5 and np.abs(n64 @ n64.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5
    assert np.abs(a64 - n64.transpose(0, 2, 1)).max() > 0.5
    assert same_bits(rows["from"][ok], cur[ok, :3]) and same_bits(rows["to"][ok], prev[ok, :3])


def test_mesh_instance_motion_takes_pairs_and_refuses():
    prev = [((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)), ((1.0, 2.0, 3.0), (0.5, 0.5, 0.5, 0.5))]
    cur = [((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)), ((1.0, 2.5, 3.0), (0.5, 0.5, 0.5, 0.5))]
    rows, bad = R.mesh_instance_motion(prev, cur)
    assert bad == 0 and rows["moving"].tolist() == [0, 1] and np.array_equal(rows["a"][1], np.eye(3, dtype=F))
    assert rows["from"][1].tolist() == [1.0, 2.5, 3.0] and rows["to"][1].tolist() == [1.0, 2.0, 3.0]
    L, C = R.lib(), R.C
    p = np.zeros((2, 7), F)
    p[:, 3] = 1.0
    out = np.full(2, 0x55, np.uint8).repeat(128).view(R.MOTION_ROW)
    before = out.tobytes()
    bad = C.c_uint32(77)
    for args in ((None, p.ctypes.data, 2, out.ctypes.data), (p.ctypes.data, None, 2, out.ctypes.data), (p.ctypes.data, p.ctypes.data, 2, None),
                 (p.ctypes.data, p.ctypes.data, 0, out.ctypes.data), (p.ctypes.data, p.ctypes.data, 65537, out.ctypes.data)):
        assert L.rtw_mesh_instance_motion(*args, C.byref(bad)) == E_INVALID
        assert out.tobytes() == before and bad.value == 77
    assert L.rtw_mesh_instance_motion(p.ctypes.data, p.ctypes.data, 2, out.ctypes.data, None) == 0        # n_invalid may be NULL
    assert np.array_equal(out, R.motion_rows(2))
    with pytest.raises(ValueError):
        R.mesh_instance_motion(prev, cur[:1])


# ---- 4. geometry -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_stays_within_the_measured_bounds():
    pos, nrm = measure_motion_bounds()
    print(f"[motion geometry] restatement against float64: positions {pos:.3g} px, normals {nrm:.3g}")
    assert pos <= MOTION_POSITION_MEASURED and nrm <= MOTION_NORMAL_MEASURED
    assert pos > MOTION_POSITION_MEASURED / 4 and nrm > MOTION_NORMAL_MEASURED / 4           # (the constants are not stale by much either)


@pytest.mark.parametrize("case", GEO_MOTION_CASES, ids=lambda c: "-".join(c))
def test_host_form_meets_float64_geometry(case):
    check_motion_geometry(R.temporal_accumulate, geo_motion_case(*case), case)


@pytest.mark.parametrize("case", [c for c in GEO_MOTION_CASES if c[1] in ("turn", "both")], ids=lambda c: "-".join(c))
def test_point_matrix_for_the_normals_loses_the_history_of_a_turned_placement(case):
    """The mistake the row's second matrix is there against: with nrm = I (or a's transpose taken for it) a placement turned by 60 degrees
    fails normal_cos = 0.9 everywhere -- cos 60 = 0.5 --, with the right matrix it passes everywhere."""
    c = geo_motion_case(*case)
    inside = motion_regions(c)[0]
    n, n_prev = c["normal"][0, 0].astype(np.float64), c["n_prev64"]
    assert abs(float(n @ n_prev) - 0.5) < 1e-6
    assert abs(float(turned_normal(c).astype(np.float64) @ n_prev) - 1.0) < 1e-6
    right = motion_probe(R.temporal_accumulate, c, normal_cos=0.9, prev_normal=c["prev_normal"])[1]
    assert np.all(right[inside] == 1)
    for name, nrm in (("identity", np.eye(3, dtype=F)), ("a itself", c["rows"]["a"][0])):
        rows = c["rows"].copy()
        rows["nrm"][0] = nrm
        wrong = motion_probe(R.temporal_accumulate, c, rows=rows, normal_cos=0.9, prev_normal=c["prev_normal"])[1]
        assert np.all(wrong == 0), (name, int((wrong != 0).sum()))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_two_placements_end_to_end_on_the_host():
    cam, prev_cam = e2e_cameras()
    prev_poses, cur_poses = e2e_poses()
    g0, g1 = e2e_guides_host(prev_cam, prev_poses), e2e_guides_host(cam, cur_poses)
    rows, bad = R.mesh_instance_motion(prev_poses, cur_poses)
    assert bad == 0 and rows["moving"].tolist() == [1, 0]
    e2e_check(R.temporal_accumulate, g0, g1, rows, "host")


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def motion_raw_call(fn, head=(), rows="rows", n_rows=4, first=2, idx="idx", prev_xy="xy", same_object=1):
    """One call of rtw_temporal_accumulate_motion (or the context's, after `head`) on a 5 x 3 frame with a history: rows / idx None -> NULL;
    prev_xy the name of the buffer out_prev_xy points to.  (status, outputs by name), the outputs filled with SENTINEL beforehand."""
    C = R.C
    h, w = 3, 5
    A = dyadic_camera(h, w)
    f0, f1 = frame(h, w, 0, A), frame(h, w, 1, turned(A, 0.4))
    out = dict(color=np.full((h, w, 3), SENTINEL), moments=np.full((h, w, 2), SENTINEL), len=np.full((h, w), SENTINEL),
               variance=np.full((h, w), SENTINEL), xy=np.full((h, w, 2), SENTINEL))
    keep = [np.ones((h, w, 2), F), np.ones((h, w), F), R.motion_rows(max(n_rows, 1))]
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    p = R.RtwTemporal(0.2, 0.2, 32, 0.05, 0.9, same_object, (C.c_float * 2)(*OFFSET))
    st = R.RtwFilterStats()
    rc = fn(*head, ptr(f1["cur"]), w, h, C.byref(f1["cam"]), ptr(f1["depth"]), ptr(f1["normal"]), ptr(f1["idx"]) if idx else None, C.byref(f0["cam"]),
            ptr(f0["cur"]), ptr(keep[0]), ptr(keep[1]), ptr(f0["depth"]), ptr(f0["normal"]), ptr(f0["idx"]) if same_object else None, C.byref(p),
            ptr(keep[2]) if rows else None, n_rows, first, ptr(out["color"]), ptr(out["moments"]), ptr(out["len"]), ptr(out["variance"]),
            None if prev_xy is None else ptr(out[prev_xy]), C.byref(st))
    return rc, out


MOTION_REFUSALS = [("rows without idx", dict(idx=None, same_object=0)), ("no row", dict(n_rows=0)),
                   ("first + n_rows beyond 2^31", dict(first=2 ** 31 - 3)), ("first beyond 2^31", dict(first=2 ** 32 - 1, n_rows=1))] + \
                  [(f"out_prev_xy is out_{k}", dict(prev_xy=k)) for k in ("color", "moments", "len", "variance")] + \
                  [(f"out_prev_xy is out_{k}, no rows", dict(prev_xy=k, rows=None)) for k in ("color", "variance")]
MOTION_ACCEPTED = [("as it is", {}), ("first + n_rows = 2^31", dict(first=2 ** 31 - 4)), ("no prev_xy", dict(prev_xy=None)),
                   ("no rows: n_rows and first are not read", dict(rows=None, n_rows=0, first=2 ** 32 - 1)),
                   ("rows, same_object off", dict(same_object=0))]


@pytest.mark.parametrize("name,change", MOTION_REFUSALS, ids=[n for n, _ in MOTION_REFUSALS])
def test_motion_refusals_write_nothing(name, change):
    rc, out = motion_raw_call(R.lib().rtw_temporal_accumulate_motion, **change)
    assert rc == E_INVALID
    assert all(np.all(v == SENTINEL) for v in out.values())


@pytest.mark.parametrize("name,change", MOTION_ACCEPTED, ids=[n for n, _ in MOTION_ACCEPTED])
def test_motion_calls_next_to_the_refusals_are_accepted(name, change):
    rc, out = motion_raw_call(R.lib().rtw_temporal_accumulate_motion, **change)
    assert rc == 0
    assert not np.any(out["color"] == SENTINEL) and (change.get("prev_xy", "xy") is None) == bool(np.all(out["xy"] == SENTINEL))


def test_todays_refusals_hold_with_rows():
    """Each refusal of rtw_temporal_accumulate through the new entry point, a table given: the list of temporal_common.refusal_calls."""
    from tests.temporal_common import raw_call, refusal_calls
    L, C = R.lib(), R.C
    rows = R.motion_rows(3)
    xy = np.full((3, 5, 2), SENTINEL)

    def fn(*a):                                                                # rtw_temporal_accumulate's arguments -> the new call's
        return L.rtw_temporal_accumulate_motion(*a[:15], C.c_void_p(rows.ctypes.data), 3, 0, *a[15:19], C.c_void_p(xy.ctypes.data), a[19])
    for name, change in refusal_calls():
        rc, outs, _ = raw_call(fn, **change)
        assert rc == E_INVALID, name
        assert all(np.all(o == SENTINEL) for o in outs) and np.all(xy == SENTINEL), name
    assert raw_call(fn)[0] == 0


def test_python_arguments():
    h, w = 3, 5
    A = dyadic_camera(h, w)
    f = frame(h, w, 0, A)
    with pytest.raises(ValueError):
        R.temporal_accumulate(f["cur"], A, depth=f["depth"], ids=f["idx"], motion=np.zeros((2, 31), F))
    with pytest.raises(ValueError):
        R.temporal_accumulate(f["cur"], A, depth=f["depth"], ids=f["idx"], motion=R.motion_rows(0))
    with pytest.raises(R.RtwError):
        R.temporal_accumulate(f["cur"], A, depth=f["depth"], motion=R.motion_rows(2))            # rows need ids
    as_floats = R.motion_rows(2).view(F).reshape(2, 32)
    hist, _, _ = R.temporal_accumulate(f["cur"], A, depth=f["depth"], ids=f["idx"], motion=as_floats, out_prev_xy=np.empty((h, w, 2), F))
    assert np.isnan(hist["prev_xy"]).all()
    assert "prev_xy" not in R.temporal_accumulate(f["cur"], A, depth=f["depth"], ids=f["idx"])[0]
