"""The reprojection of the temporal accumulation held to geometry (tests/test_temporal_cpu.py, tests/test_gpu_temporal.py): a float64
reference that shares nothing with the rule's derivation, and a probe that reads fx, fy and the acceptance of s out of the public call.

The reference.  For pixel (i, j) of the current camera at depth t, from the cameras' float32 fields, all in float64:
    P = origin + (pixel00 + du (i + ox) + dv (j + oy)) t;   solve [p00' du' dv'] (s, sX, sY)^T = P - origin' for the previous camera;
    fx = sX / s - ox;   fy = sY / s - oy
-- a 3 x 3 linear solve (numpy.linalg.solve), no cross product, no n, a, b.

The probe.  The call does not return fx and fy, so it is handed a history made by hand: prev_color[q] = (qx, qy, 1), prev_len = 1, every
term off, and a `cur` with a NaN in channel 0 of every pixel.  By the rule a pixel with a history and a bad sample writes the history back
unchanged (out_color = H, out_len = H.len = 1) and one without writes out_len 0: out_color[..., 0] and [..., 1] are the bilinear gather
of two linear ramps -- fx and fy wherever all four taps exist, and clip(fx, 0, w - 1), clip(fy, 0, h - 1) where the taps outside the frame
drop out and the rest are renormalised -- and out_len tells whether the pixel was a candidate.

The cameras are temporal_common.GEO_POSES (an orbit step at the Book-1 pose, a vertical move, a roll, a change of vfov, both with an orbit
step, a dolly, a dolly past a fifth of the points -- which end up behind the previous camera --, non-square pixels, and the orbit step 1000
units from the world's origin), the offsets GEO_OFFSETS, the frames 33 x 17 and
67 x 35, the depths 0.6 .. 1.4 times the distance of the view's target.

The bounds are measured, not guessed: the numpy restatement (temporal_common.restate, float32) run through the same probe against the
reference over every case above.
    positions:  the largest |restated - reference| of the two gathered ramps is 4.44e-4 px (the far pose at 67 x 35; 2.9e-5 px among
                the Book-1 poses).
                POSITION_MEASURED = 4.5e-4, POSITION_BOUND = 8 x that = 3.6e-3 px, below the 1/64 px the bound must stay under: the
                smallest slip the probe is there for (ox and oy swapped under the offset (0.25, 0.875)) moves a tap by 0.375 px.
    s:          on a plane fronto-parallel to the previous camera at s = D the largest |restated s - D| / D is 2.76e-6 (the far pose; 2.9e-7 among the others).
                S_MEASURED = 2.8e-6, S_TOL = 8 x that = 2.24e-5: the depth_tol under which every candidate keeps its history against
                prev_depth = D and none does against prev_depth = D (1 + 8 S_TOL).
The factor 8 is for roundings in which numpy and the library might come to differ (they do not today: test_host_equals_restatement holds them
bit for bit).  tests/test_temporal_cpu.py asserts that the restatement stays within the MEASURED values, so a change of the cases that
moves them shows there.  Pixels whose reference position lies within POSITION_BOUND of a border of the candidate box (-1, w) x (-1, h), or
whose s is within 1e-3 of 0 relative to the depth, are decided by rounding and left out; their share is asserted to be at most 2 %."""
import functools

import numpy as np

from tests.temporal_common import ALL_OFF, F, GEO_OFFSETS, GEO_POSES, TEMPORAL_TEST_DEFAULTS, geo_cameras, geo_depth, restate

GEO_SHAPES = [(17, 33), (35, 67)]                                            # (h, w)
POSITION_MEASURED = 4.5e-4
POSITION_BOUND = 8 * POSITION_MEASURED
S_MEASURED = 2.8e-6
S_TOL = 8 * S_MEASURED
LEFT_OUT_MOST = 0.02
assert POSITION_BOUND < 1.0 / 64.0
PROBE_PARAMS = dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF)
GEO_CASES = [(c, o) for c in GEO_POSES for o in GEO_OFFSETS]


def _f64(cam):
    return [np.array(list(getattr(cam, k)), np.float64) for k in ("origin", "pixel00", "delta_u", "delta_v")]


def world_points(cam, depth, offset):
    """P [h][w][3] in float64: the points of `cam`'s pixel rays at `depth`."""
    o, p00, du, dv = _f64(cam)
    h, w = np.shape(depth)
    jj, ii = np.mgrid[0:h, 0:w]
    d = p00 + du * (ii + float(offset[0]))[..., None] + dv * (jj + float(offset[1]))[..., None]
    return o + d * np.asarray(depth, np.float64)[..., None]


def project(prev_cam, P, offset):
    """(fx, fy, s) in float64 of the world points P [..][3] in `prev_cam` (module docstring)."""
    o, p00, du, dv = _f64(prev_cam)
    sol = np.linalg.solve(np.stack([p00, du, dv], 1), (P - o).reshape(-1, 3).T).T.reshape(P.shape)
    with np.errstate(all="ignore"):
        return sol[..., 1] / sol[..., 0] - float(offset[0]), sol[..., 2] / sol[..., 0] - float(offset[1]), sol[..., 0]


def reference(cam, prev_cam, depth, offset):
    return project(prev_cam, world_points(cam, depth, offset), offset)


def plane_depth(cam, prev_cam, D, offset, h, w):
    """The float64 t at which `cam`'s pixel rays meet the plane s = D of prev_cam (the points origin' + D (p00' + X du' + Y dv')), from
    origin + dir t = origin' + D p00' + X D du' + Y D dv' solved for (t, X, Y)."""
    o, p00, du, dv = _f64(cam)
    po, pp00, pdu, pdv = _f64(prev_cam)
    jj, ii = np.mgrid[0:h, 0:w]
    dirs = p00 + du * (ii + float(offset[0]))[..., None] + dv * (jj + float(offset[1]))[..., None]
    M = np.empty((h, w, 3, 3))
    M[..., 0], M[..., 1], M[..., 2] = dirs, -D * pdu, -D * pdv
    return np.linalg.solve(M, np.broadcast_to(po + D * pp00 - o, (h, w, 3))[..., None])[..., 0, 0]


def ramp_history(h, w, prev_cam, depth=None):
    """The hand-made history: colour (qx, qy, 1), length 1, no moments."""
    jj, ii = np.mgrid[0:h, 0:w]
    return dict(color=np.stack([ii, jj, np.ones_like(ii)], -1).astype(F), moments=np.zeros((h, w, 2), F), len=np.ones((h, w), F),
                depth=depth, normal=None, idx=None, cam=prev_cam)


def bad_frame(h, w):
    """A frame with a NaN in channel 0 of every pixel."""
    cur = np.random.default_rng(7 + 31 * h + w).random((h, w, 3)).astype(F)
    cur[..., 0] = np.nan
    return cur


@functools.lru_cache(maxsize=None)
def probe_case(h, w, cam_name, offset_name):
    """The inputs of one probe and its reference: dict(cam, prev_cam, depth, offset, fx, fy, s, reach)."""
    cam, prev_cam, reach = geo_cameras(h, w, cam_name)
    offset = GEO_OFFSETS[offset_name]
    depth = geo_depth(h, w, reach, 1)
    fx, fy, s = reference(cam, prev_cam, depth, offset)
    return dict(cam=cam, prev_cam=prev_cam, depth=depth, offset=offset, fx=fx, fy=fy, s=s, reach=reach)


def probe(accumulate, c, prev_depth=None, depth_tol=0.0, prev_cam=None):
    """(out_color, out_len) of the probe of case `c` through `accumulate` (R.temporal_accumulate or a Renderer's)."""
    h, w = c["depth"].shape
    hist = ramp_history(h, w, prev_cam or c["prev_cam"], prev_depth)
    out, _, _ = accumulate(bad_frame(h, w), c["cam"], depth=c["depth"], history=hist, offset=c["offset"],
                           **dict(PROBE_PARAMS, depth_tol=depth_tol))
    return np.asarray(out["color"]), np.asarray(out["len"])


def probe_restated(c, prev_depth=None, depth_tol=0.0):
    """The same through the numpy restatement; also its s."""
    h, w = c["depth"].shape
    o = restate(bad_frame(h, w), c["cam"], c["depth"], None, None, ramp_history(h, w, c["prev_cam"], prev_depth),
                offset=c["offset"], **dict(PROBE_PARAMS, depth_tol=depth_tol))
    return o["color"], o["len"], o["s"]


def regions(c, bound=POSITION_BOUND):
    """(inside, outside, left_out) of a case's pixels by the reference: a candidate for certain; none for certain; decided by rounding."""
    h, w = c["depth"].shape
    fx, fy, s = c["fx"], c["fy"], c["s"]
    sure = np.abs(s) > 1e-3 * c["reach"]
    inside = sure & (s > 0) & (fx >= -1 + bound) & (fx <= w - bound) & (fy >= -1 + bound) & (fy <= h - bound)
    outside = sure & ((s < 0) | (fx <= -1 - bound) | (fx >= w + bound) | (fy <= -1 - bound) | (fy >= h + bound))
    return inside, outside, ~(inside | outside)


def position_error(c, color):
    """The largest |gathered ramp - reference| over the pixels that are candidates for certain, and the largest |third channel - 1|."""
    h, w = c["depth"].shape
    inside = regions(c)[0]
    ex = np.abs(color[..., 0].astype(np.float64) - np.clip(c["fx"], 0, w - 1))[inside]
    ey = np.abs(color[..., 1].astype(np.float64) - np.clip(c["fy"], 0, h - 1))[inside]
    e1 = np.abs(color[..., 2].astype(np.float64) - 1.0)[inside]
    return float(max(ex.max(), ey.max())), float(e1.max())


def check_probe(accumulate, c, what):
    """The assertions of the probe on one case."""
    color, length = probe(accumulate, c)
    inside, outside, left_out = regions(c)
    assert inside.mean() > 0.02 and left_out.mean() <= LEFT_OUT_MOST, (what, inside.mean(), left_out.mean())
    err, err1 = position_error(c, color)
    print(f"[geometry] {what}: largest position error {err:.3g} px (bound {POSITION_BOUND:.3g}), inside {inside.mean():.3f}, "
          f"outside {outside.mean():.3f}, left out {left_out.mean():.4f}")
    assert err <= POSITION_BOUND, (what, err)
    assert err1 <= 4 * 2.0 ** -23, (what, err1)                               # the weights sum to 1 to a few ulp
    assert np.all(length[inside] == 1), (what, "a candidate without its history")
    assert np.all(length[outside] == 0), (what, "a history from outside the previous view")


@functools.lru_cache(maxsize=None)
def plane_case(h, w, cam_name, offset_name):
    """probe_case on a plane fronto-parallel to the previous camera at s = D (D the distance of the target as a float32): the current depth
    is the float64 ray-plane intersection rounded to float32, and the reference is that of the rounded depth."""
    c = dict(probe_case(h, w, cam_name, offset_name))
    D = float(F(c["reach"]))
    c["depth"] = plane_depth(c["cam"], c["prev_cam"], D, c["offset"], h, w).astype(F)
    c["fx"], c["fy"], c["s"] = reference(c["cam"], c["prev_cam"], c["depth"], c["offset"])
    c["D"] = D
    return c


def check_plane(accumulate, c, what):
    h, w = c["depth"].shape
    inside, _, left_out = regions(c)
    assert inside.mean() > 0.02 and left_out.mean() <= LEFT_OUT_MOST, (what, inside.mean(), left_out.mean())
    assert np.abs(c["s"] / c["D"] - 1.0).max() < 1e-6                          # (the float32 depth's rounding, seen in float64)
    keep = probe(accumulate, c, prev_depth=np.full((h, w), c["D"], F), depth_tol=S_TOL)[1]
    drop = probe(accumulate, c, prev_depth=np.full((h, w), c["D"] * (1 + 8 * S_TOL), F), depth_tol=S_TOL)[1]
    assert np.all(keep[inside] == 1), (what, "a tap at s = D rejected", int((keep[inside] != 1).sum()))
    assert np.all(drop == 0), (what, "a tap 8 tolerances away accepted", int((drop != 0).sum()))


def check_static_is_continuous(accumulate, h, w, cam_name, what):
    """The static shortcut (cam and prev_cam equal byte for byte: fx = i, fy = j, s = depth) against the general path one ulp away: the
    same inputs with prev_cam.origin[0] moved to the next float32."""
    import rtw_amd as R
    c = dict(probe_case(h, w, cam_name, "uneven"))
    same = R.RtwCamera.from_buffer_copy(c["cam"])
    moved = R.RtwCamera.from_buffer_copy(c["cam"])
    moved.origin[0] = float(np.nextafter(F(moved.origin[0]), F(np.inf)))
    assert bytes(same) == bytes(c["cam"]) and bytes(moved) != bytes(c["cam"])
    color0, len0 = probe(accumulate, c, prev_cam=same)
    color1, len1 = probe(accumulate, c, prev_cam=moved)
    jj, ii = np.mgrid[0:h, 0:w]
    assert np.array_equal(color0[..., 0], ii.astype(F)) and np.array_equal(color0[..., 1], jj.astype(F)) and np.all(len0 == 1), what
    fx, fy, s = reference(c["cam"], moved, c["depth"], c["offset"])           # (no pixel of it is within the bound of a border)
    assert np.abs(fx - ii).max() < POSITION_BOUND and np.abs(fy - jj).max() < POSITION_BOUND and s.min() > 0
    err = float(np.abs(color1[..., :2].astype(np.float64) - color0[..., :2]).max())
    print(f"[geometry] {what}: the general path one ulp from the static camera differs by {err:.3g} px")
    assert err <= POSITION_BOUND, (what, err)
    assert np.abs(color1[..., 2] - 1.0).max() <= 4 * 2.0 ** -23 and np.array_equal(len1, len0), what


# ---- a rendered view: do the surface buffers and the rule mean the same depth? ---------------------------------------------------------------
# A few spheres on a ground sphere seen from above by two Viewport cameras two degrees apart on an orbit, 64 x 36.  The reference
# knows the scene analytically: it projects each current pixel's point (from the float32 depth it is given) into the previous view as above
# and intersects the previous camera's rays through the four integer taps with the spheres in float64.
RENDERED_W, RENDERED_H = 64, 36
RENDERED_SPHERES = [((0.0, -1000.0, 0.0), 1000.0), ((0.0, 1.0, 0.0), 1.0), ((-1.5, 0.6, 2.0), 0.6), ((2.5, 0.5, -1.5), 0.5), ((1.0, 0.4, 3.0), 0.4)]
RENDERED_MINT, RENDERED_MAXT = 0.001, 1000.0
RENDERED_TOL = 0.05
RENDERED_UNDECIDED_MOST = 0.25


def rendered_cameras():
    """(current, previous): Viewport cameras at (13, 6, 3) and two degrees further along the orbit about the y axis, looking at (0, 0.5, 0)
    with a vfov of 10 degrees: the ground is seen at 19 .. 29 degrees, where its depth changes by 1.4 % a row at most -- inside half the
    tolerance -- and two degrees of orbit are up to 1.5 pixels at the ground's far and near ends."""
    import rtw_amd as R
    cams = []
    for degrees in (0.0, 2.0):
        t = np.deg2rad(degrees)
        o = np.array([np.cos(t) * 13.0 + np.sin(t) * 3.0, 6.0, -np.sin(t) * 13.0 + np.cos(t) * 3.0])
        d = np.array([0.0, 0.5, 0.0]) - o
        vp = R.Viewport.new_from_res(RENDERED_W, RENDERED_H, 1, 1, 1.0, vfov=10.0, origin=tuple(o), direction=tuple(d / np.linalg.norm(d)))
        assert vp.height == RENDERED_H
        cams.append(vp.camera())
    return cams[0], cams[1]


def sphere_hits(origin, dirs):
    """The nearest hit of the rays origin + dirs t, t in (MINT, MAXT), with RENDERED_SPHERES in float64: (t, idx, grazing) -- t is 1.6 MAXT
    and idx -1 on a miss, as surface_map writes them; grazing marks a ray so close to a silhouette that float32 may decide otherwise."""
    a = (dirs * dirs).sum(-1)
    best_t = np.full(dirs.shape[:-1], np.inf)
    best_i = np.full(dirs.shape[:-1], -1, np.int64)
    grazing = np.zeros(dirs.shape[:-1], bool)
    for k, (centre, r) in enumerate(RENDERED_SPHERES):
        oc = np.asarray(origin, np.float64) - np.array(centre)
        b = (dirs * oc).sum(-1)
        disc = b * b - a * ((oc * oc).sum() - r * r)
        grazing |= np.abs(disc) <= 1e-3 * a * r * r
        with np.errstate(invalid="ignore"):
            root = np.sqrt(disc)
            for t in ((-b - root) / a, (-b + root) / a):                     # (the nearer root first)
                ok = (disc > 0) & (t > RENDERED_MINT) & (t < RENDERED_MAXT) & (t < best_t)
                best_t, best_i = np.where(ok, t, best_t), np.where(ok, k, best_i)
    return np.where(best_i < 0, 1.6 * RENDERED_MAXT, best_t), best_i, grazing


def pixel_dirs(cam, ii, jj, offset):
    _, p00, du, dv = _f64(cam)
    return p00 + du * (np.asarray(ii, np.float64) + offset[0])[..., None] + dv * (np.asarray(jj, np.float64) + offset[1])[..., None]


def analytic_guides(cam, offset):
    """(depth float32, idx int32) of the view by the analytic intersection: what surface_map is expected to write, but for grazing rays."""
    jj, ii = np.mgrid[0:RENDERED_H, 0:RENDERED_W]
    t, idx, _ = sphere_hits(_f64(cam)[0], pixel_dirs(cam, ii, jj, offset))
    return t.astype(F), idx.astype(np.int32)


def rendered_sets(cam, prev_cam, depth, idx, offset):
    """(must_keep, must_reset) for the current view's guides `depth` and `idx` (module comment): must_keep -- the point lies in front of the
    previous camera, its four taps are inside the frame, none of their rays grazes a sphere, all four hit the pixel's object, at depths
    within half of RENDERED_TOL of s; must_reset -- the point lies behind the previous camera or projects more than a pixel (and 1/64 px
    for rounding) outside the previous frame's pixel centres 0 .. w - 1, 0 .. h - 1."""
    h, w = RENDERED_H, RENDERED_W
    fx, fy, s = reference(cam, prev_cam, depth, offset)
    x0, y0 = np.floor(fx), np.floor(fy)
    keep = (s > 0) & (x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)
    po = _f64(prev_cam)[0]
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        t, hit, grazing = sphere_hits(po, pixel_dirs(prev_cam, x0 + dx, y0 + dy, offset))
        with np.errstate(invalid="ignore"):
            keep &= ~grazing & (hit == idx) & (np.abs(t - s) <= 0.5 * RENDERED_TOL * s)
    m = 1.0 / 64.0
    reset = (s <= 0) | (fx < -1 - m) | (fx > w + m) | (fy < -1 - m) | (fy > h + m)
    return keep, reset & ~keep
