"""What the temporal-accumulation tests share (tests/test_temporal_cpu.py, tests/test_gpu_temporal.py): an independent numpy restatement of
the rule of include/rtw.h ("temporal accumulation") in float32, which also hands out fx, fy and s for inspection, and the case builders:
synthetic frames, guides and cameras, no renderer.  The restatement is the rule typed again; what holds both to geometry is
tests/temporal_geometry_common.py.

A case is a list of frames accumulated one after the other, each a dict of cur, cam, depth, normal, idx (and optionally `poke`, a
function that edits a copy of the history before this frame reads it), plus the parameters of every call.  "The same" is, as for the
a-trous filter, the same bits or NaN on both sides."""
import functools

import numpy as np

import rtw_amd as R

F = np.float32
SHAPES = [(1, 1), (3, 5), (17, 33), (35, 67)]                  # (h, w): one pixel; a few; 33 x 17 and 67 x 35 cross the 32 x 8 workgroup both ways
OFFSET = (0.5, 0.5)
ALL_ON = dict(depth_tol=0.05, normal_cos=0.9, same_object=1)
ALL_OFF = dict(depth_tol=0.0, normal_cos=0.0, same_object=0)
OUT_KEYS = ("color", "moments", "len", "variance")
TEMPORAL_TEST_DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, max_history=32)          # (the tests' own: the library's defaults may be retuned)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def mismatch(a, b):
    a, b = np.asarray(a), np.asarray(b)
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    at = np.argwhere(bad)
    return f"{int(bad.sum())} of {bad.size} differ, first at {at[0].tolist()}: {a[tuple(at[0])]!r} != {b[tuple(at[0])]!r}" if len(at) else "equal"


# ---- cameras -----------------------------------------------------------------------------------------------------------------------------
def camera(origin, p00, du, dv):
    c = R.RtwCamera()
    for name, v in (("origin", origin), ("pixel00", p00), ("delta_u", du), ("delta_v", dv)):
        setattr(c, name, (R.C.c_float * 3)(*[float(F(x)) for x in v]))
    return c


def dyadic_camera(h, w, origin=(0.0, 0.0, 0.0)):
    """Looks down -z from `origin`; every field a dyadic rational: du = (2^-6, 0, 0), dv = (0, -2^-6, 0), p00 = (-w/2 2^-6, h/2 2^-6, -1)."""
    a = 2.0 ** -6
    return camera(origin, (-w / 2 * a, h / 2 * a, -1.0), (a, 0.0, 0.0), (0.0, -a, 0.0))


def turned(cam, degrees, origin=None):
    """`cam` turned about the y axis (float32 fields, whatever they round to), optionally from another origin."""
    t = np.deg2rad(degrees)
    rot = np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])
    f = lambda v: rot @ np.array(list(v), np.float64)
    return camera(list(cam.origin) if origin is None else origin, f(cam.pixel00), f(cam.delta_u), f(cam.delta_v))


def orbit(cam, degrees):
    """A copy of `cam` carried rigidly about the world's y axis: a step along an orbit of the scene's centre."""
    t = np.deg2rad(degrees)
    rot = np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])
    c = R.RtwCamera.from_buffer_copy(cam)
    if degrees:
        for name in ("origin", "u", "v", "pixel00", "delta_u", "delta_v"):
            setattr(c, name, (R.C.c_float * 3)(*[float(F(x)) for x in rot @ np.array(list(getattr(cam, name)), np.float64)]))
    return c


def look_camera(h, w, origin, target, vfov, roll=0.0, pixel_aspect=1.0):
    """A camera as rtw_viewport_new lays one out (du, dv and the view direction mutually orthogonal, pixel00 the centre of pixel 0, 0), built
    in float64 from its pose and rounded to float32 at the end: at `origin` looking at `target`, `vfov` degrees over the h rows, rolled by
    `roll` radians about the view direction.  pixel_aspect: |du| / |dv| (1: square pixels; rtw_viewport_new gives others for a direction
    that is not a unit vector)."""
    origin, target = np.array(origin, np.float64), np.array(target, np.float64)
    fwd = (target - origin) / np.linalg.norm(target - origin)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c, s = np.cos(roll), np.sin(roll)
    right, down = c * right + s * down, c * down - s * right
    vh = 2.0 * np.tan(np.deg2rad(vfov) / 2.0)
    dv = down * (vh / h)
    du = right * (vh / h) * pixel_aspect
    p00 = fwd - du * (w / 2.0) - dv * (h / 2.0) + (du + dv) * 0.5
    return camera(origin, p00, du, dv)


# The camera pairs of the geometry cases (tests/temporal_geometry_common.py): name -> (current pose, previous pose), a pose the keyword
# arguments of look_camera.  BOOK1 is the Book-1 view: from (13, 2, 3) at the origin, 20 degrees.  Every pair keeps most of the frame in
# view for points 0.6 .. 1.4 times the target's distance away.  A skewed grid (du . dv != 0) is not among them: include/rtw.h gives the rule
# "for cameras of rtw_viewport_new only", whose du, dv and view direction are orthogonal (|du| != |dv| they do reach).
def _orbit_y(p, degrees):
    t = np.deg2rad(degrees)
    return (np.cos(t) * p[0] + np.sin(t) * p[2], p[1], -np.sin(t) * p[0] + np.cos(t) * p[2])


BOOK1 = dict(origin=(13.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), vfov=20.0)
FAR = (600.0, 500.0, 620.0)                                                     # about 1000 units from the world's origin
GEO_POSES = {
    "orbit": (BOOK1, dict(BOOK1, origin=_orbit_y(BOOK1["origin"], 2.0))),
    "vertical": (BOOK1, dict(BOOK1, origin=(13.0, 2.4, 3.0), target=(0.0, 0.4, 0.0))),
    "roll": (dict(BOOK1, roll=0.2), BOOK1),
    "zoom": (dict(BOOK1, vfov=25.0), BOOK1),
    "roll+zoom": (dict(BOOK1, roll=0.2, vfov=25.0), dict(BOOK1, origin=_orbit_y(BOOK1["origin"], 1.0))),
    "dolly": (dict(BOOK1, origin=(11.05, 1.7, 2.55)), BOOK1),
    "past": (BOOK1, dict(BOOK1, origin=(3.25, 0.5, 0.75))),                    # the previous camera has passed the nearest fifth of the points
    "nonsquare": (dict(BOOK1, pixel_aspect=1.25), dict(BOOK1, origin=_orbit_y(BOOK1["origin"], -1.5), pixel_aspect=0.8)),
    "far": (dict(BOOK1, origin=tuple(a + b for a, b in zip(FAR, BOOK1["origin"])), target=FAR),
            dict(BOOK1, origin=tuple(a + b for a, b in zip(FAR, _orbit_y(BOOK1["origin"], 2.0))), target=FAR)),
}
GEO_OFFSETS = {"half": (0.5, 0.5), "zero": (0.0, 0.0), "uneven": (0.25, 0.875)}
GEO_NAMES = [f"geo-{c}-{o}" for c in GEO_POSES for o in GEO_OFFSETS]


def geo_cameras(h, w, name):
    """(current camera, previous camera, the distance of the current camera's target) of GEO_POSES[name] for an h x w frame."""
    cur, prev = GEO_POSES[name]
    return look_camera(h, w, **cur), look_camera(h, w, **prev), float(np.linalg.norm(np.subtract(cur["target"], cur["origin"])))


def geo_depth(h, w, reach, seed=0):
    """Depths 0.6 .. 1.4 times `reach`, random per pixel."""
    return (reach * (0.6 + 0.8 * np.random.default_rng(4000 + 1000 * seed + 31 * h + w).random((h, w)))).astype(F)


# ---- the rule in numpy -------------------------------------------------------------------------------------------------------------------
def _v(x):
    return np.array(list(x), F)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.array([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]], F)


def restate(cur, cam, depth, normal, idx, prev, alpha, alpha_moments, max_history, depth_tol, normal_cos, same_object, offset=OFFSET):
    """include/rtw.h's rule, vectorised over the frame, every operation a float32 one in the written order.  prev: None or a dict of color,
    moments, len, depth, normal, idx, cam.  Returns a dict of color, moments, len, variance, and of fx, fy, s, cand (NaN / False without a
    previous frame)."""
    cur = np.asarray(cur, F)
    h, w = cur.shape[:2]
    ox, oy = F(offset[0]), F(offset[1])
    ii, jj = np.meshgrid(np.arange(w), np.arange(h))
    with np.errstate(all="ignore"):
        r, g, b = cur[..., 0], cur[..., 1], cur[..., 2]
        L = (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b
        fin = np.isfinite(r) & np.isfinite(g) & np.isfinite(b)
        wsum = np.zeros((h, w), F)
        sums = [np.zeros((h, w), F) for _ in range(6)]                      # c0 c1 c2 m1 m2 len
        fx = fy = s = np.full((h, w), np.nan, F)
        cand = np.zeros((h, w), bool)
        if prev is not None:
            pc = prev["cam"]
            p00, du, dv = _v(pc.pixel00), _v(pc.delta_u), _v(pc.delta_v)
            static = all(bytes(getattr(cam, k)) == bytes(getattr(pc, k)) for k in ("origin", "pixel00", "delta_u", "delta_v"))
            if static:
                fx, fy, s = ii.astype(F), jj.astype(F), np.asarray(depth, F)
            else:
                n = _cross(du, dv); a = _cross(dv, n); bb = _cross(n, du)
                pn, pa, pb, ua, vb = _dot(p00, n), _dot(p00, a), _dot(p00, bb), _dot(du, a), _dot(dv, bb)
                fi, fj = (ii.astype(F) + ox)[..., None], (jj.astype(F) + oy)[..., None]
                dirs = (_v(cam.pixel00) + _v(cam.delta_u) * fi) + _v(cam.delta_v) * fj
                P = _v(cam.origin) + dirs * np.asarray(depth, F)[..., None]
                d = P - _v(pc.origin)
                s = _dot(d, n) / pn
                fx = ((_dot(d, a) / s - pa) / ua) - ox
                fy = ((_dot(d, bb) / s - pb) / vb) - oy
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
                    ok &= _dot(np.asarray(normal, F), np.asarray(prev["normal"], F)[cy, cx]) >= F(normal_cos)
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
    return dict(color=np.stack(out[:3], -1), moments=np.stack(out[3:5], -1), len=out[5], variance=var, fx=fx, fy=fy, s=s, cand=cand)


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def frame(h, w, seed, cam, flat=False):
    """One synthetic frame for `cam`: colours in 0 .. 2; flat: the guides of a fronto-parallel plane at depth 4 (one normal, ids in bands);
    else a depth that varies smoothly with a few steps, four normals and ids by region."""
    rng = np.random.default_rng(1000 * seed + 31 * h + w)
    cur = (rng.random((h, w, 3)) * 2.0).astype(F)
    jj, ii = np.mgrid[0:h, 0:w]
    if flat:
        depth = np.full((h, w), 4.0, F)
        normal = np.broadcast_to(np.array([0.0, 0.0, 1.0], F), (h, w, 3)).copy()
        idx = (ii // 4).astype(np.int32)
    else:
        depth = (3.0 + 0.5 * np.sin(ii * 0.21) + 0.3 * np.cos(jj * 0.37) + 0.6 * ((ii + 2 * jj) % 11 == 0)).astype(F)
        table = np.array([[0, 0, 1], [0, 0.6, 0.8], [0.28, 0, 0.96], [1, 0, 0]], F)
        normal = table[((ii // 4 + jj // 5) % 4)].copy()
        idx = ((ii // 6) * 7 + jj // 4 - 1).astype(np.int32)
    return dict(cur=cur, cam=cam, depth=depth, normal=normal, idx=idx)


def _poke_holes(hist):
    """Holes in the history: a length of 0 and of NaN in a scatter of pixels (and NaN colours under them, which must not be read)."""
    hist = dict(hist, len=np.array(hist["len"], F), color=np.array(hist["color"], F))
    flat = hist["len"].reshape(-1)
    flat[::3] = 0.0
    flat[1::7] = np.nan
    hist["color"].reshape(-1, 3)[::3] = np.nan
    return hist


def bad_pixel_places(n, second):
    """The flat indices of the three non-finite pixels of the "bad-cur" frames: pixel 0 in both (never a history), and two more that move
    between the first and the second frame (so the second frame's meet a history)."""
    return [0, (n // 2 + 1) % n, (n - 2) % n] if second else [0, n // 2, n - 1]


def _bad_pixels(fr, second=False):
    c = fr["cur"].reshape(-1, 3)
    for at, (ch, v) in zip(bad_pixel_places(len(c), second), ((0, np.nan), (1, np.inf), (2, -np.inf))):
        c[at, ch] = v
    return fr


@functools.lru_cache(maxsize=None)
def cases(h, w):
    """{name: (frames, params)} for an h x w frame."""
    A = dyadic_camera(h, w)
    T = turned(A, 2.5)
    out = {}
    out["first"] = ([frame(h, w, 0, A)], dict(TEMPORAL_TEST_DEFAULTS, **ALL_ON))
    out["static3"] = ([frame(h, w, k, A, flat=True) for k in range(3)], dict(alpha=0.0, alpha_moments=0.0, max_history=32, **ALL_ON))
    for k in (1, 3, -2):
        out[f"shift{k}"] = ([frame(h, w, 0, dyadic_camera(h, w, (k * 2.0 ** -4, 0.0, 0.0)), flat=True), frame(h, w, 1, A, flat=True)],
                            dict(TEMPORAL_TEST_DEFAULTS, **ALL_ON))
    out["turned"] = ([frame(h, w, 0, A), frame(h, w, 1, T), frame(h, w, 2, turned(A, 4.0))], dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF))
    out["dolly"] = ([frame(h, w, 0, A), frame(h, w, 1, dyadic_camera(h, w, (0.0, 0.0, -0.3)))], dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF))
    out["behind"] = ([frame(h, w, 0, turned(A, 180.0)), frame(h, w, 1, A)], dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF))
    for name, terms in (("depth", dict(ALL_OFF, depth_tol=0.05)), ("normal", dict(ALL_OFF, normal_cos=0.9)), ("idx", dict(ALL_OFF, same_object=1)),
                        ("all", ALL_ON)):
        out[f"terms-{name}"] = ([frame(h, w, 0, A), frame(h, w, 1, turned(A, 0.4, (0.01, 0.0, 0.02)))], dict(TEMPORAL_TEST_DEFAULTS, **terms))
    out["holes-static"] = ([frame(h, w, 0, A), dict(frame(h, w, 1, A), poke=_poke_holes)], dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF))
    out["holes-turned"] = ([frame(h, w, 0, A), dict(frame(h, w, 1, T), poke=_poke_holes)], dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF))
    out["bad-cur"] = ([_bad_pixels(frame(h, w, 0, A)), _bad_pixels(frame(h, w, 1, A), second=True), frame(h, w, 2, turned(A, 1.0))],
                      dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF))
    out["saturate"] = ([frame(h, w, k, A, flat=True) for k in range(4)], dict(alpha=0.0, alpha_moments=0.0, max_history=2, **ALL_ON))
    out["floor"] = ([frame(h, w, k, A, flat=True) for k in range(4)], dict(alpha=0.5, alpha_moments=0.25, max_history=32, **ALL_ON))
    # the cameras and offsets of the geometry probe (tests/temporal_geometry_common.py) with ordinary finite frames: the previous frame, then
    # the current one; the depth test alone is on under the uneven offset (the depths are random: it accepts some taps and rejects others)
    for c in GEO_POSES:
        cur_cam, prev_cam, reach = geo_cameras(h, w, c)
        for o, offset in GEO_OFFSETS.items():
            f0, f1 = (dict(frame(h, w, k, cam), depth=geo_depth(h, w, reach, k)) for k, cam in enumerate((prev_cam, cur_cam)))
            terms = dict(ALL_OFF, depth_tol=0.25) if o == "uneven" else ALL_OFF
            out[f"geo-{c}-{o}"] = ([f0, f1], dict(TEMPORAL_TEST_DEFAULTS, offset=offset, **terms))
    return out


CASE_NAMES = ["first", "static3", "shift1", "shift3", "shift-2", "turned", "dolly", "behind", "terms-depth", "terms-normal", "terms-idx",
              "terms-all", "holes-static", "holes-turned", "bad-cur", "saturate", "floor"] + GEO_NAMES


def run(accumulate, frames, params, wrap=None):
    """The frames through `accumulate` (R.temporal_accumulate or a Renderer's), the history handed on: a list of dict(color, moments, len,
    variance) as numpy arrays, one per frame.  wrap: how an input array is handed over (e.g. onto the device)."""
    wrap = wrap or (lambda a: a)
    params = dict(dict(offset=OFFSET), **params)                                 # (a case may bring its own offset)
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
    hist, outs = None, []
    for fr in frames:
        if "poke" in fr:
            hist = {k: (wrap(v) if isinstance(v, np.ndarray) else v) for k, v in fr["poke"]({k: (host(v) if k != "cam" else v) for k, v in hist.items()}).items()}
        hist, var, st = accumulate(wrap(fr["cur"].copy()), fr["cam"], depth=wrap(fr["depth"]), normal=wrap(fr["normal"]), ids=wrap(fr["idx"]),
                                   history=hist, **params)
        assert st.taps == 4 * fr["depth"].size
        outs.append(dict(color=host(hist["color"]).copy(), moments=host(hist["moments"]).copy(), len=host(hist["len"]).copy(), variance=host(var).copy()))
    return outs


def run_restated(frames, params):
    """The same through restate(); each entry also carries fx, fy, s, cand."""
    prev, outs = None, []
    params = dict(dict(offset=OFFSET), **params)
    for fr in frames:
        if "poke" in fr:
            prev = fr["poke"](prev)
        o = restate(fr["cur"], fr["cam"], fr["depth"], fr["normal"], fr["idx"], prev, **params)
        prev = dict(color=o["color"], moments=o["moments"], len=o["len"], depth=fr["depth"], normal=fr["normal"], idx=fr["idx"], cam=fr["cam"])
        outs.append(o)
    return outs


@functools.lru_cache(maxsize=None)
def host_answer(h, w, name):
    """The host form's answer for a case, computed once and shared (read-only)."""
    frames, params = cases(h, w)[name]
    return run(R.temporal_accumulate, frames, params)


def assert_same_runs(got, want, what):
    assert len(got) == len(want)
    for k, (g, x) in enumerate(zip(got, want)):
        for key in OUT_KEYS:
            assert same_bits(g[key], x[key]), (what, f"frame {k}", key, mismatch(g[key], x[key]))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def refusal_calls(h=3, w=5):
    """[(name, kwargs of raw_call)]: every refusal of include/rtw.h, each one change to a call that is accepted."""
    nan, inf = float("nan"), float("inf")
    bad_cam = camera((0, 0, 0), (0, 0, -1), (1, 0, 0), (2, 0, 0))                      # du parallel to dv: n = 0, pn = 0
    nan_cam = camera((0, 0, 0), (0, 0, -1), (nan, 0, 0), (0, -1, 0))
    calls = [(f"null {k}", {k: None}) for k in ("cur", "cam", "depth", "params", "out_color", "out_moments", "out_len")]
    calls += [("w zero", dict(w=0)), ("h zero", dict(h=0)), ("w beyond 65535", dict(w=65536)), ("h beyond 65535", dict(h=65536))]
    calls += [(f"prev set without {k}", {k: None}) for k in ("prev_cam", "prev_color", "prev_moments", "prev_len")]
    none = dict(prev_cam=None, prev_color=None, prev_moments=None, prev_len=None, prev_depth=None, prev_normal=None, prev_idx=None)
    calls += [(f"only {k} of the prev set", dict(none, **{k: "keep"}))
              for k in ("prev_cam", "prev_color", "prev_len", "prev_depth", "prev_normal", "prev_idx")]
    calls += [(f"term on, {k} null", {k: None}) for k in ("normal", "idx", "prev_depth", "prev_normal", "prev_idx")]
    for k in ("alpha", "alpha_moments"):
        calls += [(f"{k} {v}", {k: v}) for v in (-0.01, 1.01, nan, inf)]
    calls += [("max_history 0", dict(max_history=0)), ("max_history 65536", dict(max_history=65536))]
    calls += [(f"depth_tol {v}", dict(depth_tol=v)) for v in (-0.1, nan, inf)]
    calls += [(f"normal_cos {v}", dict(normal_cos=v)) for v in (-0.1, 1.01, nan, inf)]
    calls += [("same_object 2", dict(same_object=2)), ("offset nan", dict(offset=(nan, 0.5))), ("offset inf", dict(offset=(0.5, inf)))]
    calls += [("prev_cam with pn 0", dict(prev_cam=bad_cam)), ("prev_cam not finite", dict(prev_cam=nan_cam))]
    calls += [(f"{o} is {p}", {o: p}) for o, p in (("out_color", "prev_color"), ("out_moments", "prev_moments"), ("out_len", "prev_len"))]
    return calls


SENTINEL = F(-77.0)


def raw_call(fn, head=(), h=3, w=5, **change):
    """One call of the C function `fn` (after the arguments `head`) with the arguments of an accepted two-frame call, `change` applied: a
    buffer name -> None (NULL), "keep" (as it is), or the name of another buffer (aliased); w, h, a parameter or a camera -> its value.
    Returns (status, the four output arrays), the outputs filled with SENTINEL beforehand."""
    C = R.C
    A = dyadic_camera(h, w)
    f0, f1 = frame(h, w, 0, A), frame(h, w, 1, turned(A, 0.4))
    buf = dict(cur=f1["cur"], depth=f1["depth"], normal=f1["normal"], idx=f1["idx"],
               prev_color=f0["cur"], prev_moments=np.ones((h, w, 2), F), prev_len=np.ones((h, w), F), prev_depth=f0["depth"],
               prev_normal=f0["normal"], prev_idx=f0["idx"],
               out_color=np.full((h, w, 3), SENTINEL), out_moments=np.full((h, w, 2), SENTINEL), out_len=np.full((h, w), SENTINEL),
               out_variance=np.full((h, w), SENTINEL))
    cams = dict(cam=f1["cam"], prev_cam=f0["cam"])
    prm = dict(TEMPORAL_TEST_DEFAULTS, offset=OFFSET, **ALL_ON)
    ptr = {k: C.c_void_p(v.ctypes.data) for k, v in buf.items()}
    ptr.update({k: C.byref(v) for k, v in cams.items()})
    size = dict(w=w, h=h)
    params_null = False
    for k, v in change.items():
        if k == "params":
            params_null = True
        elif k in size:
            size[k] = v
        elif k in prm:
            prm[k] = v
        elif k in cams and v is not None and v != "keep":
            ptr[k] = C.byref(v); cams[k] = v
        elif v is None:
            ptr[k] = None
        elif v != "keep":
            ptr[k] = ptr[v]
    p = R.RtwTemporal(prm["alpha"], prm["alpha_moments"], prm["max_history"], prm["depth_tol"], prm["normal_cos"], prm["same_object"],
                      (C.c_float * 2)(*prm["offset"]))
    st = R.RtwFilterStats()
    rc = fn(*head, ptr["cur"], size["w"], size["h"], ptr["cam"], ptr["depth"], ptr["normal"], ptr["idx"], ptr["prev_cam"], ptr["prev_color"],
            ptr["prev_moments"], ptr["prev_len"], ptr["prev_depth"], ptr["prev_normal"], ptr["prev_idx"], None if params_null else C.byref(p),
            ptr["out_color"], ptr["out_moments"], ptr["out_len"], ptr["out_variance"], C.byref(st))
    return rc, [buf[k] for k in ("out_color", "out_moments", "out_len", "out_variance")], buf


# ---- the C call, buffer by buffer ----------------------------------------------------------------------------------------------------------
BUFFERS = ("cur", "depth", "normal", "idx", "prev_color", "prev_moments", "prev_len", "prev_depth", "prev_normal", "prev_idx",
           "out_color", "out_moments", "out_len", "out_variance")                   # the 14 buffers of a call, in the order of its arguments
OUT_BUFFERS = dict(out_color="color", out_moments="moments", out_len="len", out_variance="variance")


def second_frame_buffers(h, w, name):
    """The buffers of the second call of a two-frame case as numpy arrays -- the ten inputs (the history is the host form's answer to the
    first frame), the four outputs filled with SENTINEL --, the two cameras, the parameters, and the host form's answer."""
    frames, params = cases(h, w)[name]
    (f0, f1), (first, want) = frames, host_answer(h, w, name)
    assert "poke" not in f1
    buf = dict(cur=f1["cur"].copy(), depth=f1["depth"], normal=f1["normal"], idx=f1["idx"], prev_color=first["color"], prev_moments=first["moments"],
               prev_len=first["len"], prev_depth=f0["depth"], prev_normal=f0["normal"], prev_idx=f0["idx"],
               out_color=np.full((h, w, 3), SENTINEL), out_moments=np.full((h, w, 2), SENTINEL), out_len=np.full((h, w), SENTINEL),
               out_variance=np.full((h, w), SENTINEL))
    return buf, f1["cam"], f0["cam"], params, want


def c_call(fn, head, h, w, cam, prev_cam, address, params):
    """One call of the C function `fn` (after the arguments `head`): address maps each of BUFFERS to an address in host or device memory (or
    None).  Returns the status."""
    C = R.C
    q = dict(dict(offset=OFFSET), **params)
    p = R.RtwTemporal(q["alpha"], q["alpha_moments"], q["max_history"], q["depth_tol"], q["normal_cos"], q["same_object"], (C.c_float * 2)(*q["offset"]))
    a = [None if address.get(k) is None else C.c_void_p(int(address[k])) for k in BUFFERS]
    st = R.RtwFilterStats()
    return fn(*head, a[0], w, h, C.byref(cam), a[1], a[2], a[3], C.byref(prev_cam), *a[4:10], C.byref(p), *a[10:14], C.byref(st))
