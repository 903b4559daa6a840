"""What the tests of temporal accumulation with moving objects share (tests/test_temporal_motion_cpu.py, tests/test_gpu_temporal_motion.py;
include/rtw.h "temporal accumulation with moving objects"): a numpy float32 restatement of the rule with a table of motion
rows, one of rtw_mesh_instance_motion, a float64 reference of where a point of a moved placement lay in the previous view that shares
nothing with either, and the case builders.  tests/temporal_common.py and tests/temporal_geometry_common.py are reused by import.

The bounds of the geometry are measured, not guessed, as in temporal_geometry_common: the numpy restatement run against the float64
reference over GEO_MOTION_CASES (on the CPU, by measure_motion_bounds below).
    positions:  the largest |restated - reference| of the gathered ramps and of prev_xy is 6.11e-4 px (the pose 1000 units out, shifted and
                turned; 7.1e-5 px among the Book-1 poses): MOTION_POSITION_MEASURED = 6.2e-4, the bound 8 x that = 4.96e-3 px, below
                1/64 px.
    normals:    the largest |1 - n' . (R64(qn_p) R64(qn_c)^T n rounded to float32)|, the dot product in float32 and in float64, is
                8.3e-8: MOTION_NORMAL_MEASURED = 8.5e-8, MOTION_NORMAL_TOL = 8 x that = 6.8e-7.
The factor 8 is temporal_geometry_common's, for roundings in which numpy and the library might come to differ."""
import functools

import numpy as np

import rtw_amd as R
from tests.temporal_common import (ALL_OFF, F, GEO_POSES, OFFSET, TEMPORAL_TEST_DEFAULTS, _cross, _dot, _v, dyadic_camera, frame, geo_cameras,
                                   geo_depth, look_camera, turned)
from tests.temporal_geometry_common import LEFT_OUT_MOST, PROBE_PARAMS, bad_frame, project, ramp_history, world_points

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
MOTION_POSITION_MEASURED = 6.2e-4
MOTION_POSITION_BOUND = 8 * MOTION_POSITION_MEASURED
MOTION_NORMAL_MEASURED = 8.5e-8
MOTION_NORMAL_TOL = 8 * MOTION_NORMAL_MEASURED
assert MOTION_POSITION_BOUND < 1.0 / 64.0
MOTION_SHAPES = [(1, 1), (7, 31), (9, 33), (35, 67)]          # (h, w): 31 x 7 and 33 x 9 straddle the 32 x 8 workgroup both ways


# ---- the rule with rows, in numpy ------------------------------------------------------------------------------------------------------------
def row_lookup(idx, rows, first):
    """(has_row [h][w] bool, k [h][w] clipped into the table): k = idx - first in 64 bits, 0 <= k < n_rows, rows[k].moving != 0."""
    idx = np.asarray(idx)
    if rows is None:
        return np.zeros(idx.shape, bool), np.zeros(idx.shape, np.int64)
    k = idx.astype(np.int64) - int(first)
    kc = np.clip(k, 0, len(rows) - 1)
    return (k >= 0) & (k < len(rows)) & (rows["moving"][kc] != 0), kc


def restate_motion(cur, cam, depth, normal, idx, prev, rows, first, alpha, alpha_moments, max_history, depth_tol, normal_cos, same_object,
                   offset=OFFSET):
    """include/rtw.h's rule with a table of rows, vectorised over the frame, every operation a float32 one in the written order.  Returns
    what temporal_common.restate returns, and has_row; fx, fy are what out_prev_xy receives."""
    cur = np.asarray(cur, F)
    h, w = cur.shape[:2]
    ox, oy = F(offset[0]), F(offset[1])
    ii, jj = np.meshgrid(np.arange(w), np.arange(h))
    depth = np.asarray(depth, F)
    with np.errstate(all="ignore"):
        r, g, b = cur[..., 0], cur[..., 1], cur[..., 2]
        L = (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b
        fin = np.isfinite(r) & np.isfinite(g) & np.isfinite(b)
        wsum = np.zeros((h, w), F)
        sums = [np.zeros((h, w), F) for _ in range(6)]
        fx = fy = s = np.full((h, w), np.nan, F)
        cand = np.zeros((h, w), bool)
        has_row = np.zeros((h, w), bool)
        if prev is not None:
            pc = prev["cam"]
            p00, du, dv = _v(pc.pixel00), _v(pc.delta_u), _v(pc.delta_v)
            static = all(bytes(getattr(cam, k)) == bytes(getattr(pc, k)) for k in ("origin", "pixel00", "delta_u", "delta_v"))
            has_row, kc = row_lookup(idx, rows, first)
            n = _cross(du, dv); a = _cross(dv, n); bb = _cross(n, du)
            pn, pa, pb, ua, vb = _dot(p00, n), _dot(p00, a), _dot(p00, bb), _dot(du, a), _dot(dv, bb)
            fi, fj = (ii.astype(F) + ox)[..., None], (jj.astype(F) + oy)[..., None]
            dirs = (_v(cam.pixel00) + _v(cam.delta_u) * fi) + _v(cam.delta_v) * fj
            P = _v(cam.origin) + dirs * depth[..., None]
            if rows is not None:
                A, fr, to = rows["a"][kc], rows["from"][kc], rows["to"][kc]
                e = P - fr
                Pm = np.stack([((A[..., c, 0] * e[..., 0] + A[..., c, 1] * e[..., 1]) + A[..., c, 2] * e[..., 2]) + to[..., c] for c in range(3)], -1)
                P = np.where(has_row[..., None], Pm, P)
            d = P - _v(pc.origin)
            s = _dot(d, n) / pn
            fx = ((_dot(d, a) / s - pa) / ua) - ox
            fy = ((_dot(d, bb) / s - pb) / vb) - oy
            if static:
                fx, fy, s = np.where(has_row, fx, ii.astype(F)), np.where(has_row, fy, jj.astype(F)), np.where(has_row, s, depth)
            nrm = None
            if normal_cos > 0:
                nrm = np.asarray(normal, F)
                if rows is not None:
                    N = rows["nrm"][kc]
                    nm = np.stack([(N[..., c, 0] * nrm[..., 0] + N[..., c, 1] * nrm[..., 1]) + N[..., c, 2] * nrm[..., 2] for c in range(3)], -1)
                    nrm = np.where(has_row[..., None], nm, nrm)
            cand = (s > 0) & (fx > -1) & (fx < F(w)) & (fy > -1) & (fy < F(h))
            x0f, y0f = np.where(cand, np.floor(fx), F(0)), np.where(cand, np.floor(fy), F(0))
            wx, wy = np.where(cand, fx, F(0)) - x0f, np.where(cand, fy, F(0)) - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            one = F(1)
            pcol, pmom, plen = np.asarray(prev["color"], F), np.asarray(prev["moments"], F), np.asarray(prev["len"], F)
            for qx, qy, wt in ((x0, y0, (one - wx) * (one - wy)), (x0 + 1, y0, wx * (one - wy)), (x0, y0 + 1, (one - wx) * wy),
                               (x0 + 1, y0 + 1, wx * wy)):
                ok = cand & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                ok &= plen[cy, cx] > 0
                if depth_tol > 0:
                    ok &= np.abs(np.asarray(prev["depth"], F)[cy, cx] - s) <= F(depth_tol) * s
                if normal_cos > 0:
                    ok &= _dot(nrm, np.asarray(prev["normal"], F)[cy, cx]) >= F(normal_cos)
                if same_object:
                    ok &= np.asarray(prev["idx"])[cy, cx] == np.asarray(idx)
                ok &= wt > 0
                wsum = np.where(ok, wsum + wt, wsum)
                vals = [pcol[cy, cx, 0], pcol[cy, cx, 1], pcol[cy, cx, 2], pmom[cy, cx, 0], pmom[cy, cx, 1], plen[cy, cx]]
                sums = [np.where(ok, t + wt * v, t) for t, v in zip(sums, vals)]
        hist = wsum > 0
        H = [t / wsum for t in sums]
        n1 = H[5] + F(1)
        n_ = np.where(n1 < F(max_history), n1, F(max_history))
        a_ = F(1) / n_
        am_ = np.where(a_ < F(alpha_moments), F(alpha_moments), a_)
        a_ = np.where(a_ < F(alpha), F(alpha), a_)
        blend = [H[c] + (cur[..., c] - H[c]) * a_ for c in range(3)] + [H[3] + (L - H[3]) * am_, H[4] + (L * L - H[4]) * am_, n_]
        fresh = [r, g, b, np.where(fin, L, F(0)), np.where(fin, L * L, F(0)), np.where(fin, F(1), F(0))]
        out = [np.where(hist, np.where(fin, blend[k], H[k]), fresh[k]).astype(F) for k in range(6)]
        var = out[4] - out[3] * out[3]
        var = np.where(var > 0, var, F(0)).astype(F)
    return dict(color=np.stack(out[:3], -1), moments=np.stack(out[3:5], -1), len=out[5], variance=var, fx=fx.astype(F), fy=fy.astype(F), s=s,
                cand=cand, has_row=has_row, prev_xy=np.stack([fx, fy], -1).astype(F))


# ---- rtw_mesh_instance_motion in numpy ---------------------------------------------------------------------------------------------------
def _hamilton(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def _rotate_n(qn, v):
    """quat_rotate_n (csrc/rtw_quat.h): (qn (0, v) conj(qn)).vec, float32, the written order; qn, v tuples of arrays."""
    hq = _hamilton(qn, (np.zeros_like(v[0]), v[0], v[1], v[2]))
    cw, cx, cy, cz = qn[0], -qn[1], -qn[2], -qn[3]
    return (hq[0] * cx + hq[1] * cw + hq[2] * cz - hq[3] * cy,
            hq[0] * cy - hq[1] * cz + hq[2] * cw + hq[3] * cx,
            hq[0] * cz + hq[1] * cy - hq[2] * cx + hq[3] * cw)


def _pose_rows(pose):
    """mesh_pose_rows: (ok [n], qn tuple of [n], pos [n][3])."""
    q = tuple(pose[:, 3 + k] for k in range(4))
    length = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    ok = np.isfinite(pose).all(1) & (length > 0) & np.isfinite(length)
    sc = F(1) / length
    return ok, tuple(c * sc for c in q), pose[:, :3]


def restate_mesh_motion(prev_poses, cur_poses):
    """(rows [n] of R.MOTION_ROW, n_invalid) by include/rtw.h's rule for rtw_mesh_instance_motion, float32 in the written order."""
    pp, cp = np.asarray(prev_poses, F).reshape(-1, 7), np.asarray(cur_poses, F).reshape(-1, 7)
    n = len(cp)
    rows = R.motion_rows(n)
    with np.errstate(all="ignore"):
        same = (pp.view(np.uint32) == cp.view(np.uint32)).all(1)
        ok_c, qc, pos_c = _pose_rows(cp)
        ok_p, qp, pos_p = _pose_rows(pp)
        conj = lambda q: (q[0], -q[1], -q[2], -q[3])
        a, nrm = np.zeros((n, 3, 3), F), np.zeros((n, 3, 3), F)
        for j in range(3):
            e = tuple(np.full(n, 1.0 if k == j else 0.0, F) for k in range(3))
            col = _rotate_n(conj(qp), _rotate_n(qc, e))
            ncol = _rotate_n(qp, _rotate_n(conj(qc), e))
            for c in range(3):
                a[:, c, j], nrm[:, c, j] = col[c], ncol[c]
    good = ~same & ok_c & ok_p
    rows["a"][good], rows["nrm"][good], rows["from"][good], rows["to"][good] = a[good], nrm[good], pos_c[good], pos_p[good]
    rows["a"][~same & ~(ok_c & ok_p)] = np.uint32(0x7fc00000).view(F)
    rows["moving"] = (~same).astype(np.uint32)
    return rows, int(((~ok_c) | (~same & ~ok_p)).sum())


# ---- synthetic cases with every id class ---------------------------------------------------------------------------------------------------
def quat_axis(degrees, axis):
    """(w, x, y, z) in float64 of a turn by `degrees` about `axis`."""
    ax = np.array(axis, np.float64)
    ax /= np.linalg.norm(ax)
    t = np.deg2rad(degrees) / 2.0
    return np.concatenate([[np.cos(t)], np.sin(t) * ax])


TABLES = {"first0": (0, 5), "first3": (3, 5), "one-row": (7, 1)}                  # name -> (first, n_rows)
TERMS = [dict(depth_tol=d, normal_cos=n, same_object=o) for d in (0.0, 0.05) for n in (0.0, 0.9) for o in (0, 1)]
terms_id = lambda t: "".join(k[0] if v else "-" for k, v in t.items())


def small_rows(n_rows, seed, still=()):
    """A table of small rigid motions about (0, 0, -3.5) -- turns of a few degrees, shifts of a pixel or two of the dyadic camera -- from
    rtw_mesh_instance_motion; the rows in `still` get equal poses (moving 0)."""
    rng = np.random.default_rng(900 + seed)
    prev, cur = np.zeros((n_rows, 7), F), np.zeros((n_rows, 7), F)
    for k in range(n_rows):
        prev[k, :3] = (0.0, 0.0, -3.5)
        prev[k, 3:] = quat_axis(rng.uniform(-20, 20), rng.normal(size=3))
        cur[k, :3] = prev[k, :3] + rng.uniform(-0.06, 0.06, 3).astype(F)
        cur[k, 3:] = quat_axis(rng.uniform(-3, 3), rng.normal(size=3)) if k % 2 else prev[k, 3:]
        if k in still:
            cur[k] = prev[k]
    rows, bad = R.mesh_instance_motion(prev, cur)
    assert bad == 0
    return rows


@functools.lru_cache(maxsize=None)
def class_case(h, w, table, moved_cam, nan_row=False):
    """Two frames of temporal_common.frame whose ids hold, in one frame, every class about the table (first, n_rows): -1, first - 1, first,
    first + n_rows - 1, first + n_rows, INT32_MIN, INT32_MAX, in bands of three columns, the same bands in both frames.  The last row of a
    table of more than one row stands still.  nan_row: row 0 holds a NaN in a[1][1].  Returns (frames, rows, first)."""
    first, n_rows = TABLES[table]
    A = dyadic_camera(h, w)
    f0, f1 = frame(h, w, 0, A), frame(h, w, 1, turned(A, 0.4, (0.01, 0.0, 0.02)) if moved_cam else A)
    ids = sorted({-1, first - 1, first, first + n_rows // 2, first + n_rows - 1, first + n_rows, I32_MIN, I32_MAX})
    jj, ii = np.mgrid[0:h, 0:w]
    idx = np.array(ids, np.int64)[(ii // 3 + jj // 4) % len(ids)].astype(np.int32)
    f0, f1 = dict(f0, idx=idx), dict(f1, idx=idx.copy())
    rows = small_rows(n_rows, 31 * h + w + first, still=(n_rows - 1,) if n_rows > 1 else ())
    if nan_row:
        rows = rows.copy()
        rows["a"][0, 1, 1] = np.nan
        rows["moving"][0] = 1
    return [f0, f1], rows, first


def run_motion(accumulate, frames, params, rows, first, wrap=None, prev_xy=True, out_color_is_cur=False):
    """The frames through `accumulate` with the table on every call: per frame a dict of color, moments, len, variance, prev_xy (numpy)."""
    wrap = wrap or (lambda a: a)
    params = dict(dict(offset=OFFSET), **params)
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
    hist, outs = None, []
    for fr in frames:
        cur = wrap(fr["cur"].copy())
        hist, var, st = accumulate(cur, fr["cam"], depth=wrap(fr["depth"]), normal=wrap(fr["normal"]), ids=wrap(fr["idx"]), history=hist,
                                   motion=rows, motion_first=first, out_prev_xy=True if prev_xy else None,
                                   out_color=cur if out_color_is_cur else None, **params)
        o = dict(color=host(hist["color"]).copy(), moments=host(hist["moments"]).copy(), len=host(hist["len"]).copy(), variance=host(var).copy())
        if prev_xy:
            o["prev_xy"] = host(hist["prev_xy"]).copy()
        outs.append(o)
    return outs


def run_motion_restated(frames, params, rows, first):
    prev, outs = None, []
    params = dict(dict(offset=OFFSET), **params)
    for fr in frames:
        o = restate_motion(fr["cur"], fr["cam"], fr["depth"], fr["normal"], fr["idx"], prev, rows, first, **params)
        prev = dict(color=o["color"], moments=o["moments"], len=o["len"], depth=fr["depth"], normal=fr["normal"], idx=fr["idx"], cam=fr["cam"])
        outs.append(o)
    return outs


@functools.lru_cache(maxsize=None)
def class_answer(h, w, table, moved_cam, terms_key, nan_row=False):
    """The host form's answer for a class_case under the terms TERMS[terms_key], computed once and shared (read-only)."""
    frames, rows, first = class_case(h, w, table, moved_cam, nan_row)
    return run_motion(R.temporal_accumulate, frames, dict(TEMPORAL_TEST_DEFAULTS, **TERMS[terms_key]), rows, first)


MOTION_KEYS = ("color", "moments", "len", "variance", "prev_xy")


# ---- geometry in float64 -----------------------------------------------------------------------------------------------------------------
def rot64(q):
    """The rotation matrix of the quaternion q (w, x, y, z; normalised here in float64), by the textbook formula."""
    w, x, y, z = np.array(q, np.float64) / np.linalg.norm(np.array(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def moved_reference(cam, prev_cam, depth, offset, prev_pose, cur_pose):
    """(fx, fy, s) in float64 of every pixel's point, taken as a point of a placement that went from prev_pose to cur_pose ([7] float32):
    P from the camera; x' = R64(qn_c)(P - pos_c); P' = R64(qn_p)^T x' + pos_p; then temporal_geometry_common.project."""
    pp, cp = np.asarray(prev_pose, F).astype(np.float64), np.asarray(cur_pose, F).astype(np.float64)
    P = world_points(cam, depth, offset)
    x = (P - cp[:3]) @ rot64(cp[3:]).T
    return project(prev_cam, x @ rot64(pp[3:]) + pp[:3], offset)


def normal_reference(prev_pose, cur_pose, n):
    """R64(qn_p) R64(qn_c)^T n: where the reported normal n of the placement pointed in the previous frame."""
    pp, cp = np.asarray(prev_pose, F).astype(np.float64), np.asarray(cur_pose, F).astype(np.float64)
    return rot64(pp[3:]) @ (rot64(cp[3:]).T @ np.asarray(n, np.float64))


TURN_AXIS = (1.0, 2.0, 3.0)                                                   # not a coordinate axis
SHIFT = (0.3, -0.2, 0.25)                                                     # about three pixels of the Book-1 view at 67 x 35
STATIC = "static"
# (camera pair of temporal_common.GEO_POSES or STATIC, kind of motion, offset)
GEO_MOTION_CASES = ([(c, "shift", "half") for c in GEO_POSES] + [("orbit", "turn", "half"), ("orbit", "both", "uneven"), ("far", "both", "half"),
                    (STATIC, "both", "half"), (STATIC, "turn", "zero")])
GEO_MOTION_OFFSETS = {"half": (0.5, 0.5), "zero": (0.0, 0.0), "uneven": (0.25, 0.875)}
GEO_MOTION_SHAPE = (35, 67)
OBJECT_ID = 12


@functools.lru_cache(maxsize=None)
def geo_motion_case(cam_name, kind, offset_name, h=GEO_MOTION_SHAPE[0], w=GEO_MOTION_SHAPE[1]):
    """One geometry case: the whole frame is one placement (id OBJECT_ID) that stood at the view's target and, between the frames, was
    shifted by SHIFT and / or turned by 60 degrees about TURN_AXIS.  dict(cam, prev_cam, depth, offset, rows, prev_pose, cur_pose, fx, fy,
    s, reach, idx, normal, prev_normal): rows from rtw_mesh_instance_motion, the reference from moved_reference; normal one unit vector
    perpendicular to the axis for every pixel, prev_normal its float64 image rounded to float32."""
    if cam_name == STATIC:
        cam, _, reach = geo_cameras(h, w, "orbit")
        prev_cam, target = cam, np.zeros(3)
    else:
        cam, prev_cam, reach = geo_cameras(h, w, cam_name)
        target = np.array(GEO_POSES[cam_name][0]["target"], np.float64)
    offset = GEO_MOTION_OFFSETS[offset_name]
    depth = geo_depth(h, w, reach, 1)
    q0 = quat_axis(25.0, (0.3, -1.0, 0.2))
    prev_pose = np.concatenate([target, q0]).astype(F)
    cur_pose = prev_pose.copy()
    if kind in ("shift", "both"):
        cur_pose[:3] = (target + np.array(SHIFT)).astype(F)
    if kind in ("turn", "both"):
        qt = quat_axis(60.0, TURN_AXIS)
        cur_pose[3:] = np.array(_hamilton(qt, q0), np.float64).astype(F) * F(1.7)                    # (not normalised: the rows normalise)
    rows, bad = R.mesh_instance_motion(prev_pose[None], cur_pose[None])
    assert bad == 0 and rows["moving"][0] == 1
    fx, fy, s = moved_reference(cam, prev_cam, depth, offset, prev_pose, cur_pose)
    ax = np.array(TURN_AXIS) / np.linalg.norm(TURN_AXIS)
    # a unit normal perpendicular to the axis the normals turn about (R(qn_p) R(qn_c)^T = R(qt)^T): n . n' = cos 60 degrees under a turn
    n = np.cross(ax, (0.0, 0.0, 1.0))
    n = (n / np.linalg.norm(n)).astype(F)
    n_prev = normal_reference(prev_pose, cur_pose, n.astype(np.float64))
    return dict(cam=cam, prev_cam=prev_cam, depth=depth, offset=offset, rows=rows, prev_pose=prev_pose, cur_pose=cur_pose, fx=fx, fy=fy, s=s,
                reach=reach, idx=np.full((h, w), OBJECT_ID, np.int32), normal=np.broadcast_to(n, (h, w, 3)).copy(),
                prev_normal=np.broadcast_to(n_prev.astype(F), (h, w, 3)).copy(), n_prev64=n_prev)


def motion_regions(c, bound=MOTION_POSITION_BOUND):
    """temporal_geometry_common.regions with this file's bound."""
    h, w = c["depth"].shape
    fx, fy, s = c["fx"], c["fy"], c["s"]
    sure = np.abs(s) > 1e-3 * c["reach"]
    inside = sure & (s > 0) & (fx >= -1 + bound) & (fx <= w - bound) & (fy >= -1 + bound) & (fy <= h - bound)
    outside = sure & ((s < 0) | (fx <= -1 - bound) | (fx >= w + bound) | (fy <= -1 - bound) | (fy >= h + bound))
    return inside, outside, ~(inside | outside)


def motion_probe(accumulate, c, rows=None, normal_cos=0.0, prev_normal=None):
    """The ramp probe of temporal_geometry_common with the case's row: (out_color, out_len, prev_xy)."""
    h, w = c["depth"].shape
    hist = dict(ramp_history(h, w, c["prev_cam"]), normal=prev_normal if normal_cos > 0 else None)
    out, _, _ = accumulate(bad_frame(h, w), c["cam"], depth=c["depth"], normal=c["normal"] if normal_cos > 0 else None, ids=c["idx"], history=hist,
                           motion=c["rows"] if rows is None else rows, motion_first=OBJECT_ID, out_prev_xy=True, offset=c["offset"],
                           **dict(PROBE_PARAMS, normal_cos=normal_cos))
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
    return host(out["color"]), host(out["len"]), host(out["prev_xy"])


def motion_probe_restated(c, normal_cos=0.0, prev_normal=None):
    h, w = c["depth"].shape
    hist = dict(ramp_history(h, w, c["prev_cam"]), normal=prev_normal)
    o = restate_motion(bad_frame(h, w), c["cam"], c["depth"], c["normal"], c["idx"], hist, c["rows"], OBJECT_ID, offset=c["offset"],
                       **dict(PROBE_PARAMS, normal_cos=normal_cos))
    return o["color"], o["len"], o["prev_xy"]


def motion_position_error(c, color, prev_xy):
    """The largest |gathered ramp - reference| and |prev_xy - reference| over the pixels that are candidates for certain."""
    h, w = c["depth"].shape
    inside = motion_regions(c)[0]
    ramp = max(np.abs(color[..., 0].astype(np.float64) - np.clip(c["fx"], 0, w - 1))[inside].max(),
               np.abs(color[..., 1].astype(np.float64) - np.clip(c["fy"], 0, h - 1))[inside].max())
    direct = max(np.abs(prev_xy[..., 0].astype(np.float64) - c["fx"])[inside].max(), np.abs(prev_xy[..., 1].astype(np.float64) - c["fy"])[inside].max())
    return float(ramp), float(direct)


def turned_normal(c, rows=None):
    """n' of the case by the rule's float32 line, from the rows."""
    N, n = (c["rows"] if rows is None else rows)["nrm"][0], c["normal"][0, 0]
    return np.array([(N[k, 0] * n[0] + N[k, 1] * n[1]) + N[k, 2] * n[2] for k in range(3)], F)


def check_motion_geometry(accumulate, c, what, bound=MOTION_POSITION_BOUND):
    """The assertions of one geometry case on `accumulate`: positions by the ramp and by prev_xy, candidates kept, the normal accepted at
    1 - MOTION_NORMAL_TOL against the reference normal and rejected against one 8 tolerances of cosine away."""
    color, length, xy = motion_probe(accumulate, c)
    inside, outside, left_out = motion_regions(c)
    assert inside.mean() > 0.02 and left_out.mean() <= LEFT_OUT_MOST, (what, inside.mean(), left_out.mean())
    ramp, direct = motion_position_error(c, color, xy)
    print(f"[motion geometry] {what}: largest position error {ramp:.3g} px by the ramp, {direct:.3g} px by prev_xy (bound {bound:.3g}), "
          f"inside {inside.mean():.3f}, left out {left_out.mean():.4f}")
    assert ramp <= bound and direct <= bound, (what, ramp, direct)
    assert np.all(length[inside] == 1) and np.all(length[outside] == 0), what
    cos = F(1.0 - MOTION_NORMAL_TOL)
    keep = motion_probe(accumulate, c, normal_cos=cos, prev_normal=c["prev_normal"])[1]
    assert np.all(keep[inside] == 1), (what, "the turned normal rejected against its reference", int((keep[inside] != 1).sum()))
    tilt = np.sqrt(2 * 8 * MOTION_NORMAL_TOL)                                      # cos(tilt) = 1 - 8 tolerances
    side = np.cross(c["n_prev64"], (0.3, 0.5, 0.8))
    away = np.cos(tilt) * c["n_prev64"] + np.sin(tilt) * side / np.linalg.norm(side)
    drop = motion_probe(accumulate, c, normal_cos=cos, prev_normal=np.broadcast_to(away.astype(F), c["normal"].shape).copy())[1]
    assert np.all(drop == 0), (what, "a normal 8 tolerances away accepted", int((drop != 0).sum()))


def measure_motion_bounds():
    """The measurement behind MOTION_POSITION_MEASURED and MOTION_NORMAL_MEASURED: the restatement against the float64 reference over
    GEO_MOTION_CASES.  Returns (positions, normals), the largest deviations."""
    pos = nrm = 0.0
    for case in GEO_MOTION_CASES:
        c = geo_motion_case(*case)
        color, _, xy = motion_probe_restated(c)
        pos = max(pos, *motion_position_error(c, color, xy))
        nrm = max(nrm, abs(1.0 - float(np.dot(turned_normal(c).astype(np.float64), c["prev_normal"][0, 0].astype(np.float64)))),
                  abs(1.0 - float(_dot(turned_normal(c), c["prev_normal"][0, 0]))))
    return pos, nrm


# ---- end to end: two placements of an icosphere ----------------------------------------------------------------------------------------------
E2E_W, E2E_H = 131, 67
E2E_MINT, E2E_MAXT = 0.001, 1000.0
E2E_PARAMS = dict(TEMPORAL_TEST_DEFAULTS, depth_tol=0.05, normal_cos=0.9, same_object=1)
E2E_CAMERA = dict(origin=(9.0, 3.0, 7.3), target=(0.0, 0.0, 0.0), vfov=24.0)
E2E_FIRST = 0                                                                # a scene of placements alone: placement k is object k


def e2e_mesh():
    v, f = R.mesh_icosphere(3, radius=1.0)
    return R.Triangle.from_mesh(v, f)


def e2e_poses():
    """(previous, current) poses [2][7]: placement 0 moves by about three pixels and turns by 60 degrees, placement 1 stands still.  The
    turn is about the line from the placement to the camera, the one turn of a convex object that brings none of its hidden side into
    view: about another axis the points that come round the silhouette were hidden behind the object itself a frame ago, and losing
    their history is right (with TURN_AXIS, 35 degrees off that line, 3 % of the interior pixels are such points)."""
    q0 = quat_axis(10.0, (0.0, 1.0, 0.0))
    prev = np.array([[-1.3, 0.0, 0.0, *q0], [1.4, 0.1, 0.3, 1.0, 0.0, 0.0, 0.0]], F)
    cur = prev.copy()
    cur[0, :3] += np.array([0.12, 0.08, -0.05], F)
    to_camera = np.array(E2E_CAMERA["origin"]) - prev[0, :3]
    cur[0, 3:] = np.array(_hamilton(quat_axis(60.0, rot64(q0) @ to_camera), q0), np.float64).astype(F)     # (points turn by R(q0)^T R(qt) R(q0))
    return prev, cur


def e2e_cameras():
    """(current, previous): 12 units from the origin, a vfov of 24 degrees over 67 rows (a pixel is 0.076 units there), one degree of
    orbit apart."""
    pose = E2E_CAMERA
    from tests.temporal_common import _orbit_y
    return look_camera(E2E_H, E2E_W, **pose), look_camera(E2E_H, E2E_W, **dict(pose, origin=_orbit_y(pose["origin"], 1.0)))


def e2e_guides_host(cam, poses):
    """depth, normal, idx of the view from the host form mesh_instance_hits over pixel_rays: idx = E2E_FIRST + placement, -1 on a miss,
    where depth is 1.6 E2E_MAXT as surface_map writes it."""
    rays = R.pixel_rays(cam, E2E_W, E2E_H, OFFSET)
    placements = [(p[:3], p[3:]) for p in poses]
    t, pl, _, nrm = R.mesh_instance_hits(e2e_mesh(), placements, rays.reshape(-1, 6), E2E_MINT, E2E_MAXT)[:4]
    hit = pl >= 0
    depth = np.where(hit, t, F(1.6 * E2E_MAXT)).astype(F).reshape(E2E_H, E2E_W)
    idx = np.where(hit, pl + E2E_FIRST, -1).astype(np.int32).reshape(E2E_H, E2E_W)
    return depth, np.ascontiguousarray(nrm.reshape(E2E_H, E2E_W, 3), F), idx


def e2e_check(accumulate, g0, g1, rows, what):
    """The conditions of the end-to-end case on the guides g0 (previous) and g1 (current), each (depth, normal, idx): with the rows the
    moved placement's interior pixels keep a history from where the reference says; without rows fewer than half of them do.  Returns
    the outputs of the call with rows (color, len, prev_xy)."""
    cam, prev_cam = e2e_cameras()
    prev_poses, cur_poses = e2e_poses()
    h, w = E2E_H, E2E_W
    hist = dict(ramp_history(h, w, prev_cam), depth=g0[0], normal=g0[1], idx=g0[2])
    cur = np.random.default_rng(5).random((h, w, 3)).astype(F)
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
    call = lambda motion: accumulate(cur.copy(), cam, depth=g1[0], normal=g1[1], ids=g1[2], history=hist, motion=motion, motion_first=E2E_FIRST,
                                     out_prev_xy=True, offset=OFFSET, **E2E_PARAMS)[0]
    with_rows, without = call(rows), call(None)
    obj = g1[2] == E2E_FIRST
    fx, fy, s = moved_reference(cam, prev_cam, g1[0], OFFSET, prev_poses[0], cur_poses[0])
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    interior = obj & (s > 0) & (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        interior &= g0[2][np.clip(y0 + dy, 0, h - 1), np.clip(x0 + dx, 0, w - 1)] == E2E_FIRST
    kept = host(with_rows["len"]) > 1
    kept_without = host(without["len"]) > 1
    xy = host(with_rows["prev_xy"])
    err = max(np.abs(xy[..., 0] - fx)[interior & kept].max(), np.abs(xy[..., 1] - fy)[interior & kept].max())
    print(f"[motion end to end] {what}: {int(obj.sum())} object pixels, {int(interior.sum())} interior, kept {kept[interior].mean():.4f} with rows, "
          f"{kept_without[interior].mean():.4f} without, largest position error {err:.3g} px")
    assert obj.sum() > 200 and interior.sum() >= 0.5 * obj.sum(), (what, int(obj.sum()), int(interior.sum()))
    assert kept[interior].mean() >= 0.98, (what, kept[interior].mean())
    assert err <= MOTION_POSITION_BOUND, (what, err)
    assert kept_without[interior].mean() < 0.5, (what, kept_without[interior].mean())
    still = g1[2] == E2E_FIRST + 1                                            # the placement that stands still is untouched by the table
    for k in ("color", "moments", "len"):
        assert np.array_equal(host(with_rows[k])[still], host(without[k])[still]), (what, k)
    return {k: host(with_rows[k]) for k in ("color", "moments", "len", "prev_xy")}
