"""What the tests of per-pixel motion share (tests/test_deform_motion_cpu.py, tests/test_gpu_deform_motion.py; include/rtw.h "temporal
accumulation with per-pixel motion"): numpy float32 restatements of rtw_tri_bary, rtw_deform_motion and the points rule of the
temporal pass, a float64 reference of where a point of a deformed (and placed, and moved) mesh lay in the previous view that shares nothing
with them, and the case builders.  tests/temporal_common.py, temporal_geometry_common.py and temporal_motion_common.py are reused by import.

The bounds of the geometry are measured, not guessed, as in temporal_motion_common: the numpy restatement run against the float64 reference
over DEFORM_GEO_CASES (on the CPU, by measure_deform_bounds below).
    positions:  the largest |restated prev_xy - reference| and |gathered ramp - reference| is 6.35e-4 px (the pose 1000 units out with the
                mesh unplaced, its vertices 1000 units out too; 3.1e-4 px placed and moved there, 4.5e-5 px among the Book-1 poses):
                DEFORM_POSITION_MEASURED = 6.4e-4, the bound 8 x that = 5.12e-3 px, below 1/64 px.
    normals:    the largest |1 - carried . reference| (the reference unit(u' x v') in float64 turned by R64(qn_p), the dot product in
                float64) is 1.743e-7 placed, 1.0e-7 unplaced: DEFORM_NORMAL_MEASURED = 1.8e-7, DEFORM_NORMAL_TOL = 8 x that = 1.44e-6.
    end to end: of the sheet's 3499 pixels the reference alone calls 3348 interior; with points all 3348 keep a history, without them 3166
                (0.9456) do -- most of those from another surface point, which is what the points are for.
The factor 8 is temporal_geometry_common's, for roundings in which numpy and the library might come to differ."""
import functools

import numpy as np

import rtw_amd as R
from tests.temporal_common import F, GEO_POSES, OFFSET, TEMPORAL_TEST_DEFAULTS, _cross, _dot, _orbit_y, _v, geo_cameras, look_camera
from tests.temporal_geometry_common import PROBE_PARAMS, bad_frame, project, ramp_history, world_points
from tests.temporal_motion_common import (GEO_MOTION_OFFSETS, _hamilton, _pose_rows, _rotate_n, motion_regions, quat_axis, restate_motion, rot64)

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
QNAN = np.uint32(0x7fc00000).view(F)
DEFORM_POSITION_MEASURED = 6.4e-4
DEFORM_POSITION_BOUND = 8 * DEFORM_POSITION_MEASURED
DEFORM_NORMAL_MEASURED = 1.8e-7
DEFORM_NORMAL_TOL = 8 * DEFORM_NORMAL_MEASURED
assert DEFORM_POSITION_BOUND < 1.0 / 64.0
POINT_SHAPES = [(1, 1), (7, 31), (9, 33), (35, 67)]           # (h, w): 31 x 7 and 33 x 9 straddle the 32 x 8 workgroup both ways
DEFORM_SIZES = [1, 255, 256, 257]                             # pixels about the workgroup of 256


def host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


# ---- the three rules in numpy ------------------------------------------------------------------------------------------------------------------
def _derive(o, u, v):
    """tri_derive (csrc/rtw_tri.h): (normal, w) of rows o, u, v [n][3], float32 in the written order."""
    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    nn = nx * nx + ny * ny + nz * nz
    length = np.sqrt(nn)
    return np.stack([nx / length, ny / length, nz / length], 1), np.stack([nx / nn, ny / nn, nz / nn], 1)


def restate_tri_bary(ouv, rays, t, tri):
    """include/rtw.h's rule of bary_out from the ouv rows: [n][2] float32."""
    a, r = np.asarray(ouv, F).reshape(-1, 9), np.asarray(rays, F).reshape(-1, 6)
    t, tri = np.asarray(t, F).reshape(-1), np.asarray(tri, np.int64).reshape(-1)
    has = (tri >= 0) & (tri < len(a))
    row = a[np.clip(tri, 0, len(a) - 1)]
    o, u, v = row[:, 0:3], row[:, 3:6], row[:, 6:9]
    with np.errstate(all="ignore"):
        _, w = _derive(o, u, v)
        q = (r[:, 0:3] + r[:, 3:6] * t[:, None]) - o
        cx, cy, cz = q[:, 1] * v[:, 2] - q[:, 2] * v[:, 1], q[:, 2] * v[:, 0] - q[:, 0] * v[:, 2], q[:, 0] * v[:, 1] - q[:, 1] * v[:, 0]
        ex, ey, ez = u[:, 1] * q[:, 2] - u[:, 2] * q[:, 1], u[:, 2] * q[:, 0] - u[:, 0] * q[:, 2], u[:, 0] * q[:, 1] - u[:, 1] * q[:, 0]
        alfa = w[:, 0] * cx + w[:, 1] * cy + w[:, 2] * cz
        beta = w[:, 0] * ex + w[:, 1] * ey + w[:, 2] * ez
    return np.where(has[:, None], np.stack([alfa, beta], 1), F(0)).astype(F)


def restate_local_rays(poses, idx, rays, first=0):
    """rtw_mesh_local_rays in numpy."""
    pp, r = np.asarray(poses, F).reshape(-1, 7), np.asarray(rays, F).reshape(-1, 6)
    k = np.asarray(idx, np.int64).reshape(-1) - int(first)
    kc = np.clip(k, 0, len(pp) - 1)
    with np.errstate(all="ignore"):
        ok, qn, pos = _pose_rows(pp[kc])
        o = _rotate_n(qn, tuple(r[:, c] - pos[:, c] for c in range(3)))
        d = _rotate_n(qn, tuple(r[:, 3 + c] for c in range(3)))
    use = ok & (k >= 0) & (k < len(pp))
    return np.where(use[:, None], np.stack(o + d, 1), r).astype(F)


def restate_deform(tri, bary, prev_ouv, idx=None, prev_poses=None, first=0):
    """include/rtw.h's rule of rtw_deform_motion: (prev_point, carried_normal), float32 in the written order, shaped like tri + (3,)."""
    shp = np.shape(tri)
    tri = np.asarray(tri, np.int64).reshape(-1)
    b = np.asarray(bary, F).reshape(-1, 2)
    a = np.asarray(prev_ouv, F).reshape(-1, 9)
    has = (tri >= 0) & (tri < len(a))
    row = a[np.clip(tri, 0, len(a) - 1)]
    o, u, v = row[:, 0:3], row[:, 3:6], row[:, 6:9]
    with np.errstate(all="ignore"):
        x = (o + b[:, 0:1] * u) + b[:, 1:2] * v
        n, _ = _derive(o, u, v)
        if prev_poses is not None:
            pp = np.asarray(prev_poses, F).reshape(-1, 7)
            k = np.asarray(idx, np.int64).reshape(-1) - int(first)
            ok, qn, pos = _pose_rows(pp[np.clip(k, 0, len(pp) - 1)])
            has &= (k >= 0) & (k < len(pp)) & ok
            conj = (qn[0], -qn[1], -qn[2], -qn[3])
            x = np.stack(_rotate_n(conj, (x[:, 0], x[:, 1], x[:, 2])), 1) + pos
            n = np.stack(_rotate_n(qn, (n[:, 0], n[:, 1], n[:, 2])), 1)
    point = np.where(has[:, None], x, QNAN).astype(F).reshape(shp + (3,))
    normal = np.where(has[:, None], n, QNAN).astype(F).reshape(shp + (3,))
    return point, normal


def restate_points(cur, cam, depth, normal, idx, prev, rows, first, prev_point, carried_normal, offset=OFFSET, **params):
    """include/rtw.h's rule with per-pixel points: a pixel whose prev_point x is not NaN projects that point, takes the four taps and tests
    carried_normal (None: normal); every other pixel is temporal_motion_common.restate_motion's.  The keys of restate_motion, and has_pt."""
    base = restate_motion(cur, cam, depth, normal, idx, prev, rows, first, offset=offset, **params)
    cur = np.asarray(cur, F)
    h, w = cur.shape[:2]
    if prev is None or prev_point is None:
        return dict(base, has_pt=np.zeros((h, w), bool))
    Pp = np.asarray(prev_point, F)
    has_pt = Pp[..., 0] == Pp[..., 0]
    ox, oy = F(offset[0]), F(offset[1])
    alpha, alpha_moments, max_history = params["alpha"], params["alpha_moments"], params["max_history"]
    depth_tol, normal_cos, same_object = params["depth_tol"], params["normal_cos"], params["same_object"]
    with np.errstate(all="ignore"):
        r, g, b = cur[..., 0], cur[..., 1], cur[..., 2]
        L = (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b
        fin = np.isfinite(r) & np.isfinite(g) & np.isfinite(b)
        pc = prev["cam"]
        p00, du, dv = _v(pc.pixel00), _v(pc.delta_u), _v(pc.delta_v)
        n = _cross(du, dv); a = _cross(dv, n); bb = _cross(n, du)
        pn, pa, pb, ua, vb = _dot(p00, n), _dot(p00, a), _dot(p00, bb), _dot(du, a), _dot(dv, bb)
        d = Pp - _v(pc.origin)
        s = _dot(d, n) / pn
        fx = ((_dot(d, a) / s - pa) / ua) - ox
        fy = ((_dot(d, bb) / s - pb) / vb) - oy
        nrm = np.asarray(carried_normal if carried_normal is not None else normal, F) if normal_cos > 0 else None
        cand = (s > 0) & (fx > -1) & (fx < F(w)) & (fy > -1) & (fy < F(h))
        x0f, y0f = np.where(cand, np.floor(fx), F(0)), np.where(cand, np.floor(fy), F(0))
        wx, wy = np.where(cand, fx, F(0)) - x0f, np.where(cand, fy, F(0)) - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        one = F(1)
        wsum = np.zeros((h, w), F)
        sums = [np.zeros((h, w), F) for _ in range(6)]
        pcol, pmom, plen = np.asarray(prev["color"], F), np.asarray(prev["moments"], F), np.asarray(prev["len"], F)
        for qx, qy, wt in ((x0, y0, (one - wx) * (one - wy)), (x0 + 1, y0, wx * (one - wy)), (x0, y0 + 1, (one - wx) * wy), (x0 + 1, y0 + 1, wx * wy)):
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
    mine = dict(color=np.stack(out[:3], -1), moments=np.stack(out[3:5], -1), len=out[5], variance=var, prev_xy=np.stack([fx, fy], -1).astype(F))
    pick = lambda k: np.where(has_pt.reshape(has_pt.shape + (1,) * (mine[k].ndim - 2)), mine[k], base[k]).astype(F)
    return dict(base, has_pt=has_pt, **{k: pick(k) for k in mine})


POINT_KEYS = ("color", "moments", "len", "variance", "prev_xy")


# ---- a mesh all of whose vertices move: a sheet facing +x under a travelling wave -------------------------------------------------------------
def sheet(n_side, phase, half_y=2.6, half_z=3.6, amplitude=0.3):
    """(vertices [(n+1)^2][3] float32, faces [2 n^2][3]) of a grid in the plane x = 0, y in +-half_y, z in +-half_z, bent by a wave that
    travels with `phase`: x = amplitude sin(1.3 z + 0.9 y + phase), and y and z sway with it, so that every vertex moves along every
    axis.  Seen from +x (the Book-1 view) it fills most of a 67 x 35 frame."""
    g = np.linspace(-1.0, 1.0, n_side + 1)
    yy, zz = np.meshgrid(g * half_y, g * half_z, indexing="ij")
    x = amplitude * np.sin(1.3 * zz + 0.9 * yy + phase)
    y = yy + 0.10 * np.sin(phase + zz)
    z = zz + 0.08 * np.cos(phase + 1.7 * yy)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(F)
    k = np.arange(n_side * n_side)
    a = k // n_side * (n_side + 1) + k % n_side
    f = np.concatenate([np.stack([a, a + 1, a + n_side + 1], 1), np.stack([a + 1, a + n_side + 2, a + n_side + 1], 1)])
    return v, f


def triangles_of(v, f):
    return R.Triangle.from_mesh(v, f)


# ---- geometry in float64 ------------------------------------------------------------------------------------------------------------------
def deformed_reference(cam, prev_cam, depth, offset, tri, cur_ouv, prev_ouv, cur_pose=None, prev_pose=None):
    """(fx, fy, s, n_prev) in float64 for the pixels with tri >= 0 (NaN elsewhere): P from the camera; into the mesh's frame by the float64
    current pose, x = R64(qn_c)(P - pos_c); the barycentrics solved in float64 from x - o = alfa u + beta v (least squares: the point lies
    off the plane by the depth's rounding); P' = o' + alfa u' + beta v' on the previous triangle, out by the float64 previous pose,
    R64(qn_p)^T P' + pos_p; then temporal_geometry_common.project.  n_prev: unit(u' x v') turned by R64(qn_p)."""
    h, w = np.shape(depth)
    on = np.asarray(tri).reshape(h, w) >= 0
    tc = np.clip(np.asarray(tri, np.int64).reshape(h, w), 0, None)
    co, pv = np.asarray(cur_ouv, F).astype(np.float64), np.asarray(prev_ouv, F).astype(np.float64)
    P = world_points(cam, depth, offset)
    if cur_pose is not None:
        cp, pp = np.asarray(cur_pose, F).astype(np.float64), np.asarray(prev_pose, F).astype(np.float64)
        P = (P - cp[:3]) @ rot64(cp[3:]).T
    o, u, v = co[tc][..., 0:3], co[tc][..., 3:6], co[tc][..., 6:9]
    q = P - o
    uu, uv, vv, qu, qv = (u * u).sum(-1), (u * v).sum(-1), (v * v).sum(-1), (q * u).sum(-1), (q * v).sum(-1)
    det = uu * vv - uv * uv
    alfa, beta = (qu * vv - qv * uv) / det, (qv * uu - qu * uv) / det
    o2, u2, v2 = pv[tc][..., 0:3], pv[tc][..., 3:6], pv[tc][..., 6:9]
    Pp = o2 + alfa[..., None] * u2 + beta[..., None] * v2
    n2 = np.cross(u2, v2)
    n2 /= np.linalg.norm(n2, axis=-1, keepdims=True)
    if cur_pose is not None:
        Pp = Pp @ rot64(pp[3:]) + pp[:3]
        n2 = n2 @ rot64(pp[3:]).T
    fx, fy, s = project(prev_cam, Pp, offset)
    nan = lambda a: np.where(on, a, np.nan)
    return nan(fx), nan(fy), nan(s), np.where(on[..., None], n2, np.nan)


PLACINGS = ("unplaced", "placed", "placed-and-moved")
# (camera pair of temporal_common.GEO_POSES, placing, offset)
DEFORM_GEO_CASES = ([(c, "placed-and-moved", "half") for c in GEO_POSES] + [("orbit", "unplaced", "half"), ("orbit", "placed", "uneven"),
                    ("far", "unplaced", "half"), ("far", "placed", "zero"), ("roll+zoom", "unplaced", "uneven")])
DEFORM_GEO_SHAPE = (35, 67)
MESH_ID = 0                                                                   # a scene of the mesh alone
MINT, MAXT = 0.001, 100000.0
PHASES = (0.0, 0.7)                                                           # previous, current


def case_poses(placing, target):
    """(previous, current) pose [7] float32 of the sheet standing at `target`, or (None, None)."""
    if placing == "unplaced":
        return None, None
    q0 = quat_axis(20.0, (0.2, 1.0, -0.3))
    prev = np.concatenate([np.asarray(target, np.float64), q0]).astype(F)
    cur = prev.copy()
    if placing == "placed-and-moved":
        cur[:3] = (np.asarray(target, np.float64) + np.array([0.1, 0.15, -0.2])).astype(F)
        cur[3:] = np.array(_hamilton(quat_axis(12.0, (1.0, 2.0, 3.0)), q0), np.float64).astype(F) * F(1.3)       # (not normalised)
    return prev, cur


def host_guides(cam, h, w, offset, v, f, pose):
    """depth, idx, tri, bary, normal of the view from the host forms: mesh_instance_hits (a pose) or triangle_hits (none) over pixel_rays,
    tri_bary over the rays as the mesh meets them, and the normal as deform_motion reports it for the same mesh."""
    rays = R.pixel_rays(cam, w, h, offset)
    T = triangles_of(v, f)
    ouv = R.mesh_ouv(v, f)
    if pose is None:
        t, tri = R.triangle_hits(T, rays, MINT, MAXT)[:2]
        local = rays
    else:
        t, _, tri, _ = R.mesh_instance_hits(T, [(pose[:3], pose[3:])], rays, MINT, MAXT)
        local = R.mesh_local_rays(pose[None], np.where(tri >= 0, MESH_ID, -1), rays, MESH_ID)
    hit = tri >= 0
    depth = np.where(hit, t, F(1.6 * MAXT)).astype(F).reshape(h, w)
    idx = np.where(hit, MESH_ID, -1).astype(np.int32).reshape(h, w)
    tri = tri.astype(np.int32).reshape(h, w)
    bary = R.tri_bary(ouv, local, t, tri).reshape(h, w, 2)
    normal = R.deform_motion(tri, bary, ouv, idx if pose is not None else None, None if pose is None else pose[None], MESH_ID)[1]
    normal = np.where(hit.reshape(h, w, 1), normal, F(0)).astype(F)
    return dict(depth=depth, idx=idx, tri=tri, bary=bary, normal=normal, ouv=ouv)


@functools.lru_cache(maxsize=None)
def deform_geo_case(cam_name, placing, offset_name, h=DEFORM_GEO_SHAPE[0], w=DEFORM_GEO_SHAPE[1], n_side=8):
    """One geometry case: the sheet at the view's target, waving from PHASES[0] to PHASES[1] (and placed, and moved).  dict(cam, prev_cam,
    offset, reach, g: the current frame's host guides, prev_ouv, prev_pose, cur_pose, fx, fy, s, n_prev: the float64 reference, depth)."""
    cam, prev_cam, reach = geo_cameras(h, w, cam_name)
    target = np.array(GEO_POSES[cam_name][0]["target"], np.float64)
    offset = GEO_MOTION_OFFSETS[offset_name]
    prev_pose, cur_pose = case_poses(placing, target)
    (v0, f), (v1, _) = sheet(n_side, PHASES[0]), sheet(n_side, PHASES[1])
    if placing == "unplaced":
        v0, v1 = (v0.astype(np.float64) + target).astype(F), (v1.astype(np.float64) + target).astype(F)
    g = host_guides(cam, h, w, offset, v1, f, cur_pose)
    prev_ouv = R.mesh_ouv(v0, f)
    fx, fy, s, n_prev = deformed_reference(cam, prev_cam, g["depth"], offset, g["tri"], g["ouv"], prev_ouv, cur_pose, prev_pose)
    return dict(cam=cam, prev_cam=prev_cam, offset=offset, reach=reach, g=g, prev_ouv=prev_ouv, prev_pose=prev_pose, cur_pose=cur_pose, fx=fx, fy=fy,
                s=s, n_prev=n_prev, depth=g["depth"])


def case_points(c, deform=R.deform_motion):
    """(prev_point, carried_normal) of a geometry case through `deform`."""
    g = c["g"]
    placed = c["prev_pose"] is not None
    return deform(g["tri"], g["bary"], c["prev_ouv"], g["idx"] if placed else None, c["prev_pose"][None] if placed else None, MESH_ID)


def points_probe(accumulate, c, point):
    """The ramp probe of temporal_geometry_common with per-pixel points: (out_color, out_len, prev_xy)."""
    h, w = c["depth"].shape
    out, _, _ = accumulate(bad_frame(h, w), c["cam"], depth=c["depth"], history=ramp_history(h, w, c["prev_cam"]), prev_point=point,
                           out_prev_xy=True, offset=c["offset"], **PROBE_PARAMS)
    return host(out["color"]), host(out["len"]), host(out["prev_xy"])


def points_probe_restated(c, point):
    h, w = c["depth"].shape
    o = restate_points(bad_frame(h, w), c["cam"], c["depth"], None, None, ramp_history(h, w, c["prev_cam"]), None, 0, point, None,
                       offset=c["offset"], **PROBE_PARAMS)
    return o["color"], o["len"], o["prev_xy"]


def position_error(c, color, prev_xy):
    """The largest |gathered ramp - reference| and |prev_xy - reference| over the mesh's pixels that are candidates for certain."""
    h, w = c["depth"].shape
    inside = motion_regions(c, DEFORM_POSITION_BOUND)[0]
    assert inside.sum() >= 100, int(inside.sum())                             # ('past' keeps 143 of 2345 in the previous view; the others over 1000)
    ramp = max(np.abs(color[..., 0].astype(np.float64) - np.clip(c["fx"], 0, w - 1))[inside].max(),
               np.abs(color[..., 1].astype(np.float64) - np.clip(c["fy"], 0, h - 1))[inside].max())
    direct = max(np.abs(prev_xy[..., 0].astype(np.float64) - c["fx"])[inside].max(), np.abs(prev_xy[..., 1].astype(np.float64) - c["fy"])[inside].max())
    return float(ramp), float(direct)


def normal_error(c, carried):
    """The largest |1 - carried . reference| over the mesh's pixels, the dot product in float64."""
    on = c["g"]["tri"] >= 0
    return float(np.abs(1.0 - (np.asarray(carried, np.float64) * c["n_prev"]).sum(-1))[on].max())


def measure_deform_bounds():
    """The measurement behind DEFORM_POSITION_MEASURED and DEFORM_NORMAL_MEASURED: the restatements against the float64 reference over
    DEFORM_GEO_CASES.  Returns (positions, normals), the largest deviations, and prints each case's."""
    pos = nrm = 0.0
    for case in DEFORM_GEO_CASES:
        c = deform_geo_case(*case)
        g, placed = c["g"], c["prev_pose"] is not None
        point, carried = restate_deform(g["tri"], g["bary"], c["prev_ouv"], g["idx"] if placed else None, c["prev_pose"][None] if placed else None, MESH_ID)
        color, _, xy = points_probe_restated(c, point)
        e, n = max(position_error(c, color, xy)), normal_error(c, carried)
        print(f"[deform bounds] {case}: positions {e:.3g} px, normals {n:.3g}")
        pos, nrm = max(pos, e), max(nrm, n)
    return pos, nrm


# ---- synthetic frames with every class of pixel ------------------------------------------------------------------------------------------------
def synthetic_points(h, w, seed, which):
    """prev_point, carried_normal [h][w][3] for temporal_common.frame's frames (a dyadic camera at the origin looking down -z, depths 2 to
    6): points a few pixels from where the static rule lands, unit normals; `which`: 'all', 'alternating' (NaN in x on every other pixel,
    y and z kept), 'none' (all NaN), 'edges' (infinities, a NaN in y or z alone, points behind the camera, the camera's own origin)."""
    rng = np.random.default_rng(7000 + 31 * h + w + seed)
    jj, ii = np.mgrid[0:h, 0:w]
    z = -(3.0 + 2.0 * rng.random((h, w)))
    a = 2.0 ** -6
    x = ((ii - w / 2 + rng.uniform(-3, 3, (h, w))) * a) * -z
    y = (-(jj - h / 2 + rng.uniform(-3, 3, (h, w))) * a) * -z
    point = np.stack([x, y, z], -1).astype(F)
    n = rng.normal(size=(h, w, 3))
    normal = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    if which == "alternating":
        point[(ii + jj) % 2 == 1, 0] = np.nan
    elif which == "none":
        point[...] = QNAN
        normal[...] = QNAN
    elif which == "edges":
        flat = point.reshape(-1, 3)
        specials = [(np.inf, 0, -3), (-np.inf, 0, -3), (0, np.inf, -3), (0, 0, np.inf), (0, 0, -np.inf), (0, np.nan, -3), (0, 0, np.nan), (0, 0, 3),
                    (0, 0, 0), (1e30, 1e30, -1e-30), (np.nan, 0, -3)]
        for k, sp in enumerate(specials):
            flat[k::len(specials) + 2][:] = np.array(sp, F)
    return point, normal


def tri_classes(n_tris):
    """Every class of tri about [0, n_tris)."""
    return sorted({-1, 0, n_tris // 2, n_tris - 1, n_tris, n_tris + 1, I32_MIN, I32_MAX, -2})


def idx_classes(first, n_mesh):
    """Every class of idx about the pose table."""
    return sorted({-1, first - 1, first, first + n_mesh // 2, first + n_mesh - 1, first + n_mesh, I32_MIN, I32_MAX})


@functools.lru_cache(maxsize=None)
def deform_case(n, placed, seed=0, n_tris=37, n_mesh=5, first=3):
    """n pixels holding every class of tri (and of idx, placed) in turn: dict(tri, bary, prev_ouv, idx, prev_poses, first); one pose is refused
    (a zero quaternion) and one triangle is degenerate (u x v = 0)."""
    rng = np.random.default_rng(8100 + 31 * n + seed)
    tc, ic = tri_classes(n_tris), idx_classes(first, n_mesh)
    k = np.arange(n)
    tri = np.where(k % 3 == 0, np.array(tc, np.int64)[(k // 3) % len(tc)], rng.integers(0, n_tris, n)).astype(np.int32)
    idx = np.where(k % 5 == 1, np.array(ic, np.int64)[(k // 5) % len(ic)], rng.integers(first, first + n_mesh, n)).astype(np.int32)
    bary = rng.uniform(-0.1, 1.1, (n, 2)).astype(F)
    ouv = rng.uniform(-2, 2, (n_tris, 9)).astype(F)
    ouv[n_tris // 2, 6:9] = ouv[n_tris // 2, 3:6] * F(2.0)
    poses = np.zeros((n_mesh, 7), F)
    poses[:, :3] = rng.uniform(-5, 5, (n_mesh, 3))
    poses[:, 3:] = rng.normal(size=(n_mesh, 4))
    poses[n_mesh - 1, 3:] = 0.0
    return dict(tri=tri, bary=bary, prev_ouv=ouv, idx=idx if placed else None, prev_poses=poses if placed else None, first=first if placed else 0)


# ---- end to end: a placed sheet that waves and moves under an orbiting camera ------------------------------------------------------------------
E2E_W, E2E_H = 131, 67
E2E_PARAMS = dict(TEMPORAL_TEST_DEFAULTS, depth_tol=0.05, normal_cos=0.9, same_object=1)
E2E_CAMERA = dict(origin=(13.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), vfov=20.0)
E2E_SIDE = 6                                                                  # 72 triangles: coarse, each about 20 pixels wide
E2E_HALF = (1.7, 2.6)                                                         # the sheet keeps clear of the frame's edge


def e2e_cameras():
    """(current, previous): the Book-1 view, one degree of orbit apart."""
    pose = E2E_CAMERA
    return look_camera(E2E_H, E2E_W, **pose), look_camera(E2E_H, E2E_W, **dict(pose, origin=_orbit_y(pose["origin"], 1.0)))


def e2e_meshes():
    """((previous vertices, current vertices), faces)."""
    (v0, f), (v1, _) = (sheet(E2E_SIDE, p, *E2E_HALF, amplitude=0.25) for p in PHASES)
    return (v0, v1), f


def e2e_poses():
    """(previous, current) [1][7]: the placement shifts by about four pixels and turns by three degrees."""
    prev, cur = case_poses("placed", (0.0, 0.0, 0.0))
    cur = cur.copy()
    cur[:3] += np.array([0.0, 0.12, 0.3], F)
    cur[3:] = np.array(_hamilton(quat_axis(3.0, (1.0, 0.2, 0.1)), prev[3:].astype(np.float64)), np.float64).astype(F)
    return prev[None], cur[None]


def e2e_host_guides():
    """(g0, g1): host_guides of the previous and the current frame."""
    cam, prev_cam = e2e_cameras()
    (v0, v1), f = e2e_meshes()
    pp, cp = e2e_poses()
    return host_guides(prev_cam, E2E_H, E2E_W, OFFSET, v0, f, pp[0]), host_guides(cam, E2E_H, E2E_W, OFFSET, v1, f, cp[0])


def e2e_check(accumulate, g0, g1, point, carried, what):
    """The conditions of the end-to-end case on the guides g0 (previous) and g1 (current): with the points EVERY interior pixel keeps a
    history; without them strictly fewer do.  Interior: the four taps of the float64 reference lie in the frame, carry the mesh's id and
    pass the reference's own depth test.  Returns the outputs of the call with points and the counts."""
    cam, prev_cam = e2e_cameras()
    pp, cp = e2e_poses()
    h, w = E2E_H, E2E_W
    hist = dict(ramp_history(h, w, prev_cam), depth=g0["depth"], normal=g0["normal"], idx=g0["idx"])
    cur = np.random.default_rng(5).random((h, w, 3)).astype(F)
    call = lambda **k: accumulate(cur.copy(), cam, depth=g1["depth"], normal=g1["normal"], ids=g1["idx"], history=hist, out_prev_xy=True, offset=OFFSET,
                                  **k, **E2E_PARAMS)[0]
    with_points, without = call(prev_point=point, carried_normal=carried), call()
    obj = g1["idx"] == MESH_ID
    fx, fy, s, _ = deformed_reference(cam, prev_cam, g1["depth"], OFFSET, g1["tri"], g1["ouv"], g0["ouv"], cp[0], pp[0])
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(np.nan_to_num(fx, nan=-9.0)).astype(np.int64), np.floor(np.nan_to_num(fy, nan=-9.0)).astype(np.int64)
        interior = obj & (s > 0) & (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            qy, qx = np.clip(y0 + dy, 0, h - 1), np.clip(x0 + dx, 0, w - 1)
            interior &= (g0["idx"][qy, qx] == MESH_ID) & (np.abs(g0["depth"][qy, qx].astype(np.float64) - s) <= E2E_PARAMS["depth_tol"] * s)
    kept, kept_without = host(with_points["len"]) > 1, host(without["len"]) > 1
    xy = host(with_points["prev_xy"])
    err = max(np.abs(xy[..., 0] - fx)[interior].max(), np.abs(xy[..., 1] - fy)[interior].max())
    counts = dict(mesh=int(obj.sum()), interior=int(interior.sum()), kept=int(kept[interior].sum()), kept_without=int(kept_without[interior].sum()))
    print(f"[deform end to end] {what}: {counts['mesh']} mesh pixels, {counts['interior']} interior, {counts['kept']} keep a history with points, "
          f"{counts['kept_without']} ({counts['kept_without'] / counts['interior']:.4f}) without, largest position error {err:.3g} px")
    assert counts["mesh"] > 2000 and counts["interior"] >= 0.25 * counts["mesh"], (what, counts)
    assert counts["kept"] == counts["interior"], (what, counts)
    assert counts["kept_without"] < counts["interior"], (what, counts)
    assert err <= DEFORM_POSITION_BOUND, (what, err)
    return {k: host(with_points[k]) for k in ("color", "moments", "len", "prev_xy")}, counts
