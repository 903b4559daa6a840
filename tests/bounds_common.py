"""What the tests of the neighbourhood colour bounds and of the bounded accumulation share (tests/test_bounds_cpu.py,
tests/test_gpu_bounds.py): numpy restatements of the two rules of include/rtw.h ("neighbourhood colour bounds", "bounded temporal
accumulation"), the case matrix, the edge-value frames and the refusals.

restate_bounds is the rule typed again pixel by pixel with np.float32 scalars: every operation rounds once, np.sqrt of a float32 is
correctly rounded, the taps run dy outer, dx inner.  restate_bounded adds the clamp to the restatements the temporal tests already have
(tests/temporal_common.py's restate, tests/deform_motion_common.py's restate_points for rows and points): those are imported and give the
history's colour (through a frame that does not enter), the moments and the length; only the clamp and the blend of the clamped colour are
written here.  "The same" is the same bits, or NaN on both sides (tests/atrous_common.py)."""
import ctypes as C
import functools

import numpy as np

import rtw_amd as R
from tests.atrous_common import mismatch, same_bits  # noqa: F401  (re-exported)
from tests.deform_motion_common import restate_points, synthetic_points
from tests.temporal_common import ALL_OFF, ALL_ON, OFFSET, TEMPORAL_TEST_DEFAULTS, dyadic_camera, frame, restate, turned
from tests.temporal_motion_common import small_rows

F = np.float32
INF = F(np.inf)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SHAPES = [(1, 1), (7, 1), (1, 7), (2, 2), (4, 5), (9, 3)]   # (h, w): 1x1, 1x7, 7x1, 2x2, 5x4, and 3x9, narrower than the window of radius 3
RADII = [1, 2, 3]
KS = [0.0, 0.5, 1.0, 3.0, 1e38]
FLAGS = [(s, e) for s in (False, True) for e in (False, True)]     # (same_object, exclude_centre)
TILE_SHAPES = [(32, 16), (31, 15), (33, 17), (65, 33)]            # (h, w): 16x32, 15x31, 17x33, 33x65 about the 32 x 16 workgroup
MANY_TILES = (70, 50)                                               # 50x70: 2 x 5 workgroups, ragged both ways


# ---- the rule of the bounds in numpy -------------------------------------------------------------------------------------------------------
def restate_bounds(frame, ids=None, radius=1, k=1.0, same_object=False, exclude_centre=False):
    """(lo, hi, clamped), include/rtw.h's rule pixel by pixel, every operation a float32 one in the written order."""
    frame = np.asarray(frame, F)
    h, w, _ = frame.shape
    lo, hi, clamped = (np.empty((h, w, 3), F) for _ in range(3))
    kf = F(k)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                taps = []
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        qx, qy = x + dx, y + dy
                        if qx < 0 or qx >= w or qy < 0 or qy >= h:
                            continue
                        if exclude_centre and dx == 0 and dy == 0:
                            continue
                        if same_object and ids[qy, qx] != ids[y, x]:
                            continue
                        if not np.isfinite(frame[qy, qx]).all():
                            continue
                        taps.append(frame[qy, qx])
                if not taps:
                    lo[y, x], hi[y, x] = -INF, INF
                else:
                    nf = F(len(taps))
                    for c in range(3):
                        s = F(0.0)
                        for t in taps:
                            s = s + t[c]
                        mu = s / nf
                        qq = F(0.0)
                        for t in taps:
                            d = t[c] - mu
                            qq = qq + d * d
                        e = kf * np.sqrt(qq / nf)
                        lo[y, x, c], hi[y, x, c] = mu - e, mu + e
                for c in range(3):
                    v = frame[y, x, c]
                    clamped[y, x, c] = v if not np.isfinite(v) else (lo[y, x, c] if v < lo[y, x, c] else (hi[y, x, c] if v > hi[y, x, c] else v))
    return lo, hi, clamped


# ---- frames --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(h, w, seed=0):
    """(frame, ids): colours in 0 .. 2 with a firefly, ids in blocks of a few pixels with -1 among them.  Read-only."""
    rng = np.random.default_rng(8100 + 1000 * seed + 31 * h + w)
    fr = (rng.random((h, w, 3)) * 2.0).astype(F)
    fr.reshape(-1, 3)[(h * w) // 2] = (40.0, 0.5, 1e4)
    jj, ii = np.mgrid[0:h, 0:w]
    ids = ((ii // 3) * 5 + jj // 2 - 1).astype(np.int32)
    for a in (fr, ids):
        a.setflags(write=False)
    return fr, ids


def edge_pixels():
    """The values the rule names: NaN, both infinities, a value whose sums overflow, denormals and -0."""
    tiny = np.float32(1e-45)
    return [(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (3e38, 3e38, -3e38), (tiny, -tiny, F(-0.0)), (F(-0.0), F(-0.0), F(-0.0))]


@functools.lru_cache(maxsize=None)
def edge_frame(h, w, places, which):
    """inputs(h, w)'s frame, small values 0.1 .. 0.3 under it, with edge_pixels()[which] at each (y, x) of `places` that lies inside.
    ids as inputs' but for -1, INT32_MIN and INT32_MAX at the first three places.  Read-only."""
    fr, ids = (np.array(a) for a in inputs(h, w))
    fr = (F(0.1) + fr * F(0.1)).astype(F)
    px = np.array(edge_pixels()[which], F)
    special = (-1, I32_MIN, I32_MAX)
    for n, (y, x) in enumerate(places):
        if 0 <= y < h and 0 <= x < w:
            fr[y, x] = px
            if n < 3:
                ids[y, x] = special[n]
    for a in (fr, ids):
        a.setflags(write=False)
    return fr, ids


def tile_places(h, w):
    """A tile's first and last row and column, its halo on every side (the neighbouring tiles' edge pixels), and the frame's corners."""
    ys = [0, 1, 14, 15, 16, 17, 18, h - 2, h - 1]
    xs = [0, 1, 30, 31, 32, 33, 34, w - 2, w - 1]
    return tuple(sorted({(y, x) for y in ys for x in xs if 0 <= y < h and 0 <= x < w and (y + x) % 3 != 1}))


def small_places(h, w):
    """The centre alone; one neighbour of the centre; every neighbour of the centre (the three cases of the rule's edge values)."""
    cy, cx = h // 2, w // 2
    ring = tuple((cy + dy, cx + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx))
    return [((cy, cx),), ((cy, cx + 1) if w > 1 else (cy + 1, cx),), ring]


@functools.lru_cache(maxsize=None)
def host_bounds(h, w, radius, k, same_object, exclude_centre, edge=None):
    """The host form's (lo, hi, clamped, taps) for inputs(h, w) -- or for edge_frame(h, w, *edge) --, computed once (read-only)."""
    fr, ids = inputs(h, w) if edge is None else edge_frame(h, w, *edge)
    lo, hi, cl, st = R.colour_bounds(fr, ids=ids, radius=radius, k=k, same_object=same_object, exclude_centre=exclude_centre, out_clamped=True)
    for a in (lo, hi, cl):
        a.setflags(write=False)
    return lo, hi, cl, int(st.taps)


def taps_inside(h, w, radius):
    return sum(max(0, w - abs(d)) for d in range(-radius, radius + 1)) * sum(max(0, h - abs(d)) for d in range(-radius, radius + 1))


def check_bounds(call, h, w, radius, k, same_object, exclude_centre, edge=None, wrap=None):
    """`call` (a Renderer's colour_bounds) against the host form on one case; returns its stats."""
    wrap = wrap or (lambda a: a)
    fr, ids = inputs(h, w) if edge is None else edge_frame(h, w, *edge)
    lo, hi, cl, st = call(wrap(fr), ids=wrap(ids), radius=radius, k=k, same_object=same_object, exclude_centre=exclude_centre, out_clamped=True)
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else a
    want = host_bounds(h, w, radius, k, same_object, exclude_centre, edge)
    for name, g, x in zip(("lo", "hi", "clamped"), (lo, hi, cl), want):
        assert same_bits(host(g), x), ((h, w), radius, k, same_object, exclude_centre, edge, name, mismatch(host(g), x))
    assert st.taps == want[3]
    return st


# ---- the refusals of the bounds ------------------------------------------------------------------------------------------------------------
def check_bounds_refusals(call, head):
    """Every refusal include/rtw.h lists: RTW_E_INVALID (-1) and the outputs untouched; then a call that is accepted, so that the arguments
    the refused ones share are known to be good."""
    h, w = 4, 5
    fr, ids = (np.array(a) for a in inputs(h, w))
    before = fr.copy()
    lo, hi, cl = (np.full((h, w, 3), 7.0, F) for _ in range(3))
    P = lambda a: C.c_void_p(a.ctypes.data)
    nan, inf = float("nan"), float("inf")

    def prm(radius=2, k=1.0, same=1, excl=0):
        return C.byref(R.RtwColourBounds(radius, k, same, excl))

    def refused(*args):
        assert call(*head, *args, None) == -1, args
        assert (lo == 7.0).all() and (hi == 7.0).all() and (cl == 7.0).all() and same_bits(fr, before)

    fp, ip, lp, hp, cp = P(fr), P(ids), P(lo), P(hi), P(cl)
    refused(None, w, h, ip, prm(), lp, hp, cp)
    refused(fp, w, h, ip, None, lp, hp, cp)
    refused(fp, w, h, ip, prm(), None, hp, cp)
    refused(fp, w, h, ip, prm(), lp, None, cp)
    refused(fp, 0, h, ip, prm(), lp, hp, cp)
    refused(fp, w, 0, ip, prm(), lp, hp, cp)
    refused(fp, 0x7FFFFC01, 1, ip, prm(), lp, hp, cp)
    refused(fp, 1, 0x7FFFFC01, ip, prm(), lp, hp, cp)
    refused(fp, 65536, 65536, ip, prm(), lp, hp, cp)
    for radius in (0, R.BOUNDS_MAX_RADIUS + 1):
        refused(fp, w, h, ip, prm(radius=radius), lp, hp, cp)
    for k in (-0.5, nan, inf, -inf):
        refused(fp, w, h, ip, prm(k=k), lp, hp, cp)
    refused(fp, w, h, ip, prm(same=2), lp, hp, cp)
    refused(fp, w, h, ip, prm(excl=2), lp, hp, cp)
    refused(fp, w, h, None, prm(same=1), lp, hp, cp)
    refused(fp, w, h, ip, prm(), lp, lp, cp)                    # two outputs the same buffer
    refused(fp, w, h, ip, prm(), lp, hp, lp)
    refused(fp, w, h, ip, prm(), lp, hp, hp)
    refused(fp, w, h, ip, prm(), fp, hp, cp)                    # an output that is `in`
    refused(fp, w, h, ip, prm(), lp, fp, cp)
    refused(fp, w, h, ip, prm(), lp, hp, fp)
    assert call(*head, fp, w, h, None, prm(same=0), lp, hp, None, None) == 0          # no idx without same_object, no out_clamped
    want = R.colour_bounds(fr, radius=2, k=1.0)
    assert same_bits(lo, want[0]) and same_bits(hi, want[1]) and (cl == 7.0).all()


# ---- the bounded accumulation --------------------------------------------------------------------------------------------------------------
def _clip(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(F)


def restate_bounded(cur, cam, depth, normal, idx, prev, lo, hi, rows=None, first=0, prev_point=None, carried_normal=None, offset=OFFSET, **params):
    """include/rtw.h's rule: dict of color, moments, len, variance, clipped.  The imported restatement is run twice: on `cur` (the moments,
    the length and the variance, which the bounds do not touch) and on a frame of NaN, which does not enter and so returns the history's
    colour h where a pixel has one and a length of 0 where it has none.  The clamp and the blend of the clamped colour are this file's."""
    cur = np.asarray(cur, F)
    general = rows is not None or prev_point is not None
    run = (lambda c: restate_points(c, cam, depth, normal, idx, prev, rows, first, prev_point, carried_normal, offset=offset, **params)) if general \
        else (lambda c: restate(c, cam, depth, normal, idx, prev, offset=offset, **params))
    base = run(cur)
    out = {k: base[k] for k in ("color", "moments", "len", "variance")}
    out["clipped"] = np.zeros(cur.shape[:2], F)
    if prev is None:
        return out
    probe = run(np.full_like(cur, np.nan))
    hist = probe["len"] > 0
    with np.errstate(all="ignore"):
        H = probe["color"]
        Hc = H if lo is None else _clip(H, np.asarray(lo, F), np.asarray(hi, F))
        d = np.abs(H - Hc)
        out["clipped"] = np.where(hist, (d[..., 0] + d[..., 1]) + d[..., 2], F(0)).astype(F)
        fin = np.isfinite(cur).all(-1)
        a_ = F(1) / base["len"]                                                   # (len is n_ where the frame entered)
        a_ = np.where(a_ < F(params["alpha"]), F(params["alpha"]), a_)[..., None]
        blend = Hc + (cur - Hc) * a_
        out["color"] = np.where(hist[..., None], np.where(fin[..., None], blend, Hc), cur).astype(F)
    return out


BOUNDED_KEYS = ("color", "moments", "len", "variance", "clipped")
BOUNDED_CASES = ["static", "moved", "row", "point", "first", "bad-cur"]


@functools.lru_cache(maxsize=None)
def bounded_case(name, h=9, w=33):
    """(frames, params, extra): two frames (one for "first") and the keyword arguments the second call takes beside the bounds."""
    A = dyadic_camera(h, w)
    T = turned(A, 0.4, (0.01, 0.0, 0.02))
    params = dict(TEMPORAL_TEST_DEFAULTS, **ALL_ON)
    extra = {}
    if name == "first":
        return [frame(h, w, 0, A)], params, extra
    flat = name in ("static", "bad-cur")
    f0, f1 = frame(h, w, 0, A, flat=flat), frame(h, w, 1, A if name in ("static", "bad-cur", "row", "point") else T, flat=flat)
    if name == "bad-cur":
        c = f1["cur"].reshape(-1, 3)
        c[3, 0], c[h * w // 2, 1], c[-2, 2] = np.nan, np.inf, -np.inf
    if name == "row":
        jj, ii = np.mgrid[0:h, 0:w]
        idx = (ii // 4 % 3).astype(np.int32)
        f0, f1 = dict(f0, idx=idx), dict(f1, idx=idx.copy())
        extra = dict(motion=small_rows(2, 31 * h + w), motion_first=1)
        params = dict(TEMPORAL_TEST_DEFAULTS, **dict(ALL_OFF, same_object=1))
    if name == "point":
        point, carried = synthetic_points(h, w, 0, "alternating")
        extra = dict(prev_point=point, carried_normal=carried)
        params = dict(TEMPORAL_TEST_DEFAULTS, **ALL_OFF)
    return [f0, f1], params, extra


def case_bounds(fr, kind):
    """(hist_lo, hist_hi) for the frame `fr` of a case: 'box' the bounds of its cur (radius 1, k 0.5: narrow enough to clip most pixels),
    'open' (-inf, +inf), 'nan', 'cur' (lo = hi = cur), None: no bounds."""
    cur = fr["cur"]
    if kind is None:
        return None, None
    if kind == "box":
        return R.colour_bounds(cur, radius=1, k=0.5)[:2]
    if kind == "open":
        return np.full_like(cur, -np.inf), np.full_like(cur, np.inf)
    if kind == "nan":
        return np.full_like(cur, np.nan), np.full_like(cur, np.nan)
    assert kind == "cur"
    return cur.copy(), cur.copy()


def run_bounded(accumulate, name, kind, wrap=None, clipped=True):
    """The case's frames through `accumulate`, the last with the bounds `kind`: dict of BOUNDED_KEYS as numpy arrays (without 'clipped' when
    it was not asked for)."""
    wrap = wrap or (lambda a: a)
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
    frames, params, extra = bounded_case(name)
    hist = None
    for n, fr in enumerate(frames):
        kw = dict(depth=wrap(fr["depth"]), normal=wrap(fr["normal"]), ids=wrap(fr["idx"]), history=hist, offset=OFFSET, **params)
        if n == len(frames) - 1:
            lo, hi = case_bounds(fr, kind)
            kw.update(extra, hist_lo=None if lo is None else wrap(lo), hist_hi=None if hi is None else wrap(hi), out_clipped=True if clipped else None)
        hist, var, _ = accumulate(wrap(fr["cur"].copy()), fr["cam"], **kw)
    out = dict(color=host(hist["color"]), moments=host(hist["moments"]), len=host(hist["len"]), variance=host(var))
    if "clipped" in hist:
        out["clipped"] = host(hist["clipped"])
    return out


def run_bounded_restated(name, kind):
    frames, params, extra = bounded_case(name)
    prev = None
    for n, fr in enumerate(frames):
        last = n == len(frames) - 1
        lo, hi = case_bounds(fr, kind) if last else (None, None)
        kw = dict(rows=extra.get("motion"), first=extra.get("motion_first", 0), prev_point=extra.get("prev_point"),
                  carried_normal=extra.get("carried_normal")) if last else {}
        o = restate_bounded(fr["cur"], fr["cam"], fr["depth"], fr["normal"], fr["idx"], prev, lo, hi, **kw, **params)
        prev = dict(color=o["color"], moments=o["moments"], len=o["len"], depth=fr["depth"], normal=fr["normal"], idx=fr["idx"], cam=fr["cam"])
    return o


@functools.lru_cache(maxsize=None)
def host_bounded(name, kind):
    """The host form's answer, computed once (read-only)."""
    return run_bounded(R.temporal_accumulate, name, kind)


def assert_same_outputs(got, want, what):
    for key in want:
        assert key in got, (what, key)
        assert same_bits(got[key], want[key]), (what, key, mismatch(got[key], want[key]))


def lighting_step(accumulate, colour_bounds, h=6, w=9, radius=1, k=1.0, wrap=None):
    """Eight flat frames of 0.25, then one of 0.75, static camera, flat guides, alpha 0: (the ninth colour without bounds, with the bounds of
    the ninth frame, out_clipped) as numpy arrays."""
    wrap = wrap or (lambda a: a)
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
    A = dyadic_camera(h, w)
    g = frame(h, w, 0, A, flat=True)
    guides = dict(depth=wrap(g["depth"]), normal=wrap(g["normal"]), ids=wrap(g["idx"]))
    params = dict(alpha=0.0, alpha_moments=0.0, max_history=32, offset=OFFSET, **ALL_ON)
    hist = None
    for _ in range(8):
        hist, _, _ = accumulate(wrap(np.full((h, w, 3), 0.25, F)), A, history=hist, **guides, **params)
    ninth = wrap(np.full((h, w, 3), 0.75, F))
    plain, _, _ = accumulate(ninth, A, history=hist, **guides, **params)
    lo, hi, _, _ = colour_bounds(ninth, radius=radius, k=k)
    bounded, _, _ = accumulate(ninth, A, history=hist, hist_lo=lo, hist_hi=hi, out_clipped=True, **guides, **params)
    return host(plain["color"]), host(bounded["color"]), host(bounded["clipped"])


# ---- the C entry points with the three new pointers NULL ----------------------------------------------------------------------------------
def raw_null_bounds_vs_points(bounded, points, head, name):
    """The last frame of the case `name` through the C entry point `bounded` with hist_lo, hist_hi and out_clipped NULL, and through the
    `_points` entry point on the same inputs (both after the arguments `head`): two lists of the five outputs color, moments, len,
    variance, prev_xy, filled with a sentinel beforehand.  Nothing of Python's dispatch lies between."""
    frames, params, extra = bounded_case(name)
    fr = frames[-1]
    h, w = fr["depth"].shape
    hist = None
    for f in frames[:-1]:
        hist = R.temporal_accumulate(f["cur"], f["cam"], depth=f["depth"], normal=f["normal"], ids=f["idx"], history=hist, offset=OFFSET, **params)[0]
    P = lambda a: None if a is None else C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    prm = R.RtwTemporal(params["alpha"], params["alpha_moments"], params["max_history"], params["depth_tol"], params["normal_cos"],
                        params["same_object"], (C.c_float * 2)(*OFFSET))
    rows = extra.get("motion")
    keep = [np.ascontiguousarray(a) for a in (fr["cur"], fr["depth"], fr["normal"], fr["idx"], extra.get("prev_point"), extra.get("carried_normal"))
            if a is not None]                                                            # (contiguous already: P takes their addresses)
    hk = hist or {}
    fixed = [P(fr["cur"]), w, h, C.byref(fr["cam"]), P(fr["depth"]), P(fr["normal"]), P(fr["idx"]), C.byref(hk["cam"]) if hist else None,
             P(hk.get("color")), P(hk.get("moments")), P(hk.get("len")), P(hk.get("depth")), P(hk.get("normal")), P(hk.get("idx")), C.byref(prm),
             P(rows), 0 if rows is None else len(rows), extra.get("motion_first", 0), P(extra.get("prev_point")), P(extra.get("carried_normal"))]
    new = lambda: [np.full(shape, F(-77.0)) for shape in ((h, w, 3), (h, w, 2), (h, w), (h, w), (h, w, 2))]
    got, want = new(), new()
    assert bounded(*head, *fixed, None, None, *(P(a) for a in got), None, None) == 0
    assert points(*head, *fixed, *(P(a) for a in want), None) == 0
    del keep
    return got, want


# ---- the refusals of the bounded accumulation ----------------------------------------------------------------------------------------------
def check_bounded_refusals(call, head):
    """Every refusal the bounded call adds (include/rtw.h), each with the outputs untouched, and an accepted call with the same arguments."""
    frames, params, _ = bounded_case("moved")
    f0, f1 = frames
    h, w = f1["depth"].shape
    first = R.temporal_accumulate(f0["cur"], f0["cam"], depth=f0["depth"], normal=f0["normal"], ids=f0["idx"], offset=OFFSET, **params)[0]
    lo, hi = case_bounds(f1, "box")
    S = F(-77.0)
    outs = dict(out_color=np.full((h, w, 3), S), out_moments=np.full((h, w, 2), S), out_len=np.full((h, w), S), out_variance=np.full((h, w), S),
                out_prev_xy=np.full((h, w, 2), S), out_clipped=np.full((h, w), S))
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    prm = R.RtwTemporal(params["alpha"], params["alpha_moments"], params["max_history"], params["depth_tol"], params["normal_cos"],
                        params["same_object"], (C.c_float * 2)(*OFFSET))

    def go(**change):
        a = dict(hist_lo=lo, hist_hi=hi, **outs)
        a.update({k: (a[v] if isinstance(v, str) else v) for k, v in change.items()})
        return call(*head, P(f1["cur"]), w, h, C.byref(f1["cam"]), P(f1["depth"]), P(f1["normal"]), P(f1["idx"]), C.byref(first["cam"]),
                    P(first["color"]), P(first["moments"]), P(first["len"]), P(f0["depth"]), P(f0["normal"]), P(f0["idx"]), C.byref(prm),
                    None, 0, 0, None, None, P(a["hist_lo"]), P(a["hist_hi"]), P(a["out_color"]), P(a["out_moments"]), P(a["out_len"]),
                    P(a["out_variance"]), P(a["out_prev_xy"]), P(a["out_clipped"]), None)

    refusals = [dict(hist_lo=None), dict(hist_hi=None)]
    refusals += [{b: o} for b in ("hist_lo", "hist_hi", "out_clipped") for o in ("out_color", "out_moments", "out_len", "out_variance", "out_prev_xy")]
    refusals += [dict(out_clipped="hist_lo"), dict(out_clipped="hist_hi")]
    keep = (lo.copy(), hi.copy())
    for change in refusals:
        assert go(**change) == -1, change
        assert all((a == S).all() for a in outs.values()), change
        assert same_bits(lo, keep[0]) and same_bits(hi, keep[1]), change
    assert go() == 0
    want = host_bounded("moved", "box")
    for k in BOUNDED_KEYS:
        assert same_bits(outs["out_" + k], want[k]), (k, mismatch(outs["out_" + k], want[k]))
