"""What the tests of the variance estimate and the variance-steered a-trous filter share (tests/test_svgf_cpu.py,
tests/test_gpu_svgf.py): the case matrix, its inputs, and numpy restatements of the two rules of include/rtw.h ("variance estimate",
"variance-steered a-trous filter"), written from that text and independent of the library but for exp_plain.

The inputs are tests/atrous_common.py's frames and guides with all their specials (NaN and infinite pixels, a NaN depth, misses).  The
history -- moments and length -- comes from the host form of the temporal accumulation run over five noisy copies of that frame
under a camera that stands still three times and then turns twice, by about a seventh of the frame and by a third of a pixel, so that the
lengths are 2 in the strip the first turn uncovered, fractions between that edge and the rest, and 5; a few entries are then overwritten with
the values this sequence does not reach: a length of 0 (a hole), of 1, of NaN, of 1/2 and of 65535 (saturated), and an infinite second
moment.  The filter runs on the a-trous tests' frame itself (the accumulated colour has shed its NaN and infinite pixels); its variance
is the host estimate of that history with a 0, a +inf, a NaN and a negative entry written in.

The restatements are vectorised per tap, in tap order, as tests/atrous_common.py's; "bit for bit" is its same_bits."""
import functools

import numpy as np

import rtw_amd as R
from tests.atrous_common import (DEEP_LEVELS, DEEP_SHAPES, DEEP_TERM_SETS, FLOOR, SHAPES, TERM_SETS, deep_frame, inputs, mismatch,  # noqa: F401
                                 same_bits, taps_inside)                       # (re-exported to the two test files)
from tests.temporal_common import ALL_OFF, dyadic_camera, turned

F = np.float32
LEVELS = [1, 3, 8]
RADII = [1, 3]
MIN_HISTORIES = [1, 4]
SIGMA_LUM, EPSILON = 1.5, 1e-6
TILE_W, TILE_H = 32, 16                                    # the kernels' workgroup (csrc/rtw_atrous_dev.h ABX, ABY)
TILE_SHAPES = [(h, w) for h in (TILE_H - 1, TILE_H, TILE_H + 1) for w in (TILE_W - 1, TILE_W, TILE_W + 1)]
MANY_TILES = (4 * TILE_H + 3, 2 * TILE_W + 7)              # 71 x 67: 3 x 5 ragged workgroups
# name -> (sigma_color, sigma_depth, sigma_normal, same_object, albedo, emitted, sigma_luminance): the a-trous term sets with the luminance
# term off (the identity with rtw_atrous_filter), and the luminance term alone, beside the colour term, and beside everything
SVGF_TERM_SETS = {name: t + (0.0,) for name, t in TERM_SETS.items()}
SVGF_TERM_SETS.update({
    "var": (0.0, 0.0, 0.0, False, False, False, SIGMA_LUM),
    "var+color": (TERM_SETS["color"][0], 0.0, 0.0, False, False, False, SIGMA_LUM),
    "var+albedo": (0.0, 0.0, 0.0, False, True, False, SIGMA_LUM),
    "var+guides+albedo+emitted": (0.0,) + TERM_SETS["all+albedo+emitted"][1:] + (SIGMA_LUM,),
    "var+all+albedo+emitted": TERM_SETS["all+albedo+emitted"] + (SIGMA_LUM,),
})
# Levels 7 and 8 with taps inside the frame (tests/atrous_common.py, DEEP_SHAPES): its term sets with the luminance term off, and the
# luminance term -- whose width does not shrink with the level -- alone, beside an albedo, and beside the guides
SVGF_DEEP_TERM_SETS = {name: t + (0.0,) for name, t in DEEP_TERM_SETS.items()}
SVGF_DEEP_TERM_SETS.update({
    "var": SVGF_TERM_SETS["var"],
    "var+albedo": SVGF_TERM_SETS["var+albedo"],
    "var+guides+albedo+emitted": DEEP_TERM_SETS["guides+albedo+emitted"] + (SIGMA_LUM,),
})
# name -> (sigma_depth, sigma_normal, same_object) of the variance estimate
VARIANCE_TERM_SETS = {
    "none": (0.0, 0.0, False),
    "depth": (TERM_SETS["depth"][1], 0.0, False),
    "normal": (0.0, TERM_SETS["normal"][2], False),
    "idx": (0.0, 0.0, True),
    "all": TERM_SETS["all"][1:4],
}


@functools.lru_cache(maxsize=None)
def history(h, w):
    """(moments [h][w][2], length [h][w]) as the module docstring describes them.  Read-only arrays."""
    g = inputs(h, w)
    rng = np.random.default_rng(77 + 131 * h + w)
    cam0 = dyadic_camera(h, w)
    hist = None
    turn = 0.895 * max(1.3, 0.15 * w)                              # a pixel is 0.895 degrees at the centre
    for degrees in (0.0, 0.0, 0.0, turn, turn + 0.3):
        with np.errstate(all="ignore"):
            cur = (g["frame"] * (F(1.0) + F(0.3) * rng.standard_normal((h, w, 3)).astype(F))).astype(F)
        hist, _, _ = R.temporal_accumulate(cur, turned(cam0, degrees), g["depth"], history=hist, alpha=0.0, alpha_moments=0.0, max_history=8,
                                           **ALL_OFF)
    moments, length = hist["moments"].copy(), hist["len"].copy()
    if h * w >= 15:
        spots = rng.choice(h * w, 6, replace=False)
        length.reshape(-1)[spots[4]] = 0.0
        length.reshape(-1)[spots[5]] = 1.0
        length.reshape(-1)[spots[0]] = np.nan
        length.reshape(-1)[spots[1]] = 0.5
        length.reshape(-1)[spots[2]] = 65535.0
        moments.reshape(-1, 2)[spots[3], 1] = np.inf
        length.reshape(-1)[spots[3]] = 6.0                          # (taken down the first branch whatever min_history: V = +inf)
    else:
        length.reshape(-1)[0] = 0.5
    for a in (moments, length):
        a.setflags(write=False)
    return moments, length


def variance_kwargs(h, w, terms, min_history, radius):
    """The keyword arguments of variance_estimate / Renderer.variance_estimate for one case (moments and length are history(h, w)'s)."""
    sd, sn, same = VARIANCE_TERM_SETS[terms]
    g = inputs(h, w)
    return dict(depth=g["depth"] if sd > 0 else None, normal=g["normal"] if sn > 0 else None, ids=g["ids"] if same else None,
                min_history=min_history, radius=radius, sigma_depth=sd, sigma_normal=sn, same_object=same)


@functools.lru_cache(maxsize=None)
def host_variance(h, w, terms, min_history, radius):
    """The host form's estimate of one case, computed once (read-only)."""
    moments, length = history(h, w)
    out = R.variance_estimate(moments, length, **variance_kwargs(h, w, terms, min_history, radius))[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def filter_inputs(h, w):
    """(frame, variance) of the filter's cases: the a-trous tests' frame, and the estimate with every guide on, min_history 4 and radius 3
    with its specials written in.  Read-only arrays."""
    color = inputs(h, w)["frame"]
    variance = host_variance(h, w, "all", 4, 3).copy()
    if h * w >= 15:
        spots = np.random.default_rng(99 + 131 * h + w).choice(h * w, 4, replace=False)
        variance.reshape(-1)[spots] = (0.0, np.inf, np.nan, -0.25)
    variance.setflags(write=False)
    return color, variance


def filter_kwargs(h, w, terms, levels, prefilter):
    """The keyword arguments of svgf_filter / Renderer.svgf_filter for one case (frame and variance are filter_inputs(h, w)'s)."""
    sc, sd, sn, same, alb, emi, sl = SVGF_DEEP_TERM_SETS[terms] if (h, w) in DEEP_SHAPES else SVGF_TERM_SETS[terms]
    g = inputs(h, w)
    return dict(depth=g["depth"] if sd > 0 else None, normal=g["normal"] if sn > 0 else None, ids=g["ids"] if same else None,
                albedo=g["albedo"] if alb else None, emitted=g["emitted"] if emi else None, levels=levels, sigma_color=sc,
                sigma_depth=sd, sigma_normal=sn, same_object=same, albedo_floor=FLOOR, sigma_luminance=sl, epsilon=EPSILON,
                prefilter=bool(prefilter))


def atrous_kwargs(kw):
    """filter_kwargs' result as atrous_filter takes it."""
    return {k: v for k, v in kw.items() if k not in ("sigma_luminance", "epsilon", "prefilter")}


@functools.lru_cache(maxsize=None)
def host_filter(h, w, terms, levels, prefilter):
    """The host form's (out, out_variance) of one case, computed once (read-only)."""
    frame, variance = filter_inputs(h, w)
    out, var, _ = R.svgf_filter(frame, variance, **filter_kwargs(h, w, terms, levels, prefilter))
    out.setflags(write=False)
    var.setflags(write=False)
    return out, var


@functools.lru_cache(maxsize=None)
def deep_variance(h, w):
    """filter_inputs(h, w)'s variance with its non-finite entries set to 0.25, for the reason deep_frame gives: out_variance sums every
    counted tap's variance, and seven levels spread an infinite one over the strip.  (The 0 and the negative entry stay.)  Read-only."""
    variance = filter_inputs(h, w)[1].copy()
    variance[~np.isfinite(variance)] = 0.25
    variance.setflags(write=False)
    return variance


@functools.lru_cache(maxsize=None)
def deep_filter(h, w, terms, levels, prefilter):
    """The host form's (out, out_variance, taps) of one of the cases at DEEP_SHAPES on deep_frame and deep_variance, computed once
    (read-only)."""
    out, var, st = R.svgf_filter(deep_frame(h, w), deep_variance(h, w), **filter_kwargs(h, w, terms, levels, prefilter))
    out.setflags(write=False)
    var.setflags(write=False)
    return out, var, int(st.taps)


# ---- the rules in numpy ------------------------------------------------------------------------------------------------------------------
def _exp_plain(x):
    return R.exp_plain(np.ascontiguousarray(x, F).reshape(-1)).reshape(x.shape)


def _lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _windows(h, w, reach, step):
    """For each tap (dx, dy) of a (2 reach + 1)^2 window stepping by `step`, dy outer: (dx, dy, P, Q), the slices of the centres whose tap
    lies inside the frame and of those taps; taps outside the frame for every centre are left out."""
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            y0, y1, x0, x1 = max(0, -dy * step), min(h, h - dy * step), max(0, -dx * step), min(w, w - dx * step)
            if y0 < y1 and x0 < x1:
                yield (dx, dy, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy * step, y1 + dy * step), slice(x0 + dx * step, x1 + dx * step)))


def ref_variance(moments, length, depth=None, normal=None, ids=None, min_history=4, radius=3, sigma_depth=0.0, sigma_normal=0.0,
                 same_object=False):
    """include/rtw.h "variance estimate" in numpy, float32 throughout.  A guide that is None has its term off."""
    moments, n = np.asarray(moments, F), np.asarray(length, F)
    h, w = n.shape
    m1, m2 = moments[..., 0], moments[..., 1]
    sd = sigma_depth if depth is not None else 0.0
    sn = sigma_normal if normal is not None else 0.0
    same = same_object and ids is not None
    with np.errstate(all="ignore"):
        vt = m2 - m1 * m1
        vt = np.where(vt > 0, vt, F(0.0))
        inv_depth = F(0.5) / (F(sd) * F(sd)) if sd > 0 else F(0.0)
        inv_normal = F(0.5) / (F(sn) * F(sn)) if sn > 0 else F(0.0)
        s1, s2, ws = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        for _dx, _dy, P, Q in _windows(h, w, radius, 1):
            acc = np.zeros(n[P].shape, F)
            if sd > 0:
                dz = depth[Q] - depth[P]
                acc = acc + inv_depth * (dz * dz)
            if sn > 0:
                acc = acc + inv_normal * _sq3(normal[Q] - normal[P])
            g = np.where(acc >= 0, _exp_plain(-acc), F(0.0)).astype(F)
            if same:
                g = np.where(ids[Q] != ids[P], F(0.0), g)
            take = (n[Q] > 0) & (g > 0)
            s1[P] = np.where(take, s1[P] + g * m1[Q], s1[P])
            s2[P] = np.where(take, s2[P] + g * m2[Q], s2[P])
            ws[P] = np.where(take, ws[P] + g, ws[P])
        M1, M2 = s1 / ws, s2 / ws
        vs = M2 - M1 * M1
        vs = np.where(vs > 0, vs, F(0.0)) * (F(min_history) / np.where(n >= 1, n, F(1.0)))
        return np.where(n >= F(min_history), vt, np.where(ws > 0, vs, F(0.0))).astype(F)


def ref_svgf(frame, variance, depth=None, normal=None, ids=None, albedo=None, emitted=None, levels=3, sigma_color=0.0, sigma_depth=0.0,
             sigma_normal=0.0, same_object=False, albedo_floor=0.0, sigma_luminance=0.0, epsilon=1e-6, prefilter=True):
    """include/rtw.h "variance-steered a-trous filter" in numpy, float32 throughout: (out, out_variance)."""
    frame, variance = np.asarray(frame, F), np.asarray(variance, F)
    h, w, _ = frame.shape
    K, G = [F(0.375), F(0.25), F(0.0625)], [F(0.5), F(0.25)]
    sd = sigma_depth if depth is not None else 0.0
    sn = sigma_normal if normal is not None else 0.0
    same = same_object and ids is not None
    with np.errstate(all="ignore"):
        a = np.where(albedo >= F(albedo_floor), albedo, F(1.0)).astype(F) if albedo is not None else np.ones_like(frame)
        e = np.asarray(emitted, F) if emitted is not None else np.zeros_like(frame)
        c = (frame - e) / a
        la = _lum(a)
        la2 = la * la
        v = np.where(variance > 0, variance / la2, F(0.0)).astype(F)
        inv_depth = F(0.5) / (F(sd) * F(sd)) if sd > 0 else F(0.0)
        inv_normal = F(0.5) / (F(sn) * F(sn)) if sn > 0 else F(0.0)
        sl2 = (F(2.0) * F(sigma_luminance)) * F(sigma_luminance)
        for i in range(levels):
            s, scale = 1 << i, F(2.0 ** -i)
            sc_i = F(sigma_color) * scale
            inv_color = F(0.5) / (sc_i * sc_i) if sigma_color > 0 else F(0.0)
            if sigma_luminance > 0:
                vbar = v
                if prefilter:
                    num, gs = np.zeros((h, w), F), np.zeros((h, w), F)
                    for dx, dy, P, Q in _windows(h, w, 1, 1):
                        gw = G[abs(dx)] * G[abs(dy)]
                        num[P] = num[P] + gw * v[Q]
                        gs[P] = gs[P] + gw
                    vbar = num / gs
                den = sl2 * vbar + F(epsilon)
                lum = _lum(c)
            total, wsum, vsum = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dx, dy, P, Q in _windows(h, w, 2, s):
                hw = K[abs(dx)] * K[abs(dy)]
                acc = np.zeros(wsum[P].shape, F)
                if sigma_color > 0:
                    acc = acc + inv_color * _sq3(c[Q] - c[P])
                if sd > 0:
                    dz = (depth[Q] - depth[P]) * scale
                    acc = acc + inv_depth * (dz * dz)
                if sn > 0:
                    acc = acc + inv_normal * _sq3(normal[Q] - normal[P])
                if sigma_luminance > 0:
                    dl = lum[Q] - lum[P]
                    acc = acc + (dl * dl) / den[P]
                g = np.where(acc >= 0, _exp_plain(-acc), F(0.0)).astype(F)
                if same:
                    g = np.where(ids[Q] != ids[P], F(0.0), g)
                wt = hw * g
                take = wt > 0
                total[P] = np.where(take[..., None], total[P] + c[Q] * wt[..., None], total[P])
                wsum[P] = np.where(take, wsum[P] + wt, wsum[P])
                vsum[P] = np.where(take, vsum[P] + (wt * wt) * v[Q], vsum[P])
            c = np.where((wsum > 0)[..., None], total / wsum[..., None], c).astype(F)
            v = np.where(wsum > 0, vsum / (wsum * wsum), v).astype(F)
        return (c * a + e).astype(F), (v * la2).astype(F)


# ---- the refusals, through the host forms (head = ()) or a context's entry points (head = (handle,)) -----------------------------------------
def check_refusals(variance_call, filter_call, head):
    """Every refusal include/rtw.h lists for the two passes: RTW_E_INVALID (-1) and the outputs untouched; then a call that is accepted,
    so that the arguments the refused ones share are known to be good."""
    import ctypes as C
    h, w = 9, 17
    g = inputs(h, w)
    moments, length = (a.copy() for a in history(h, w))
    frame, variance = (a.copy() for a in filter_inputs(h, w))
    out_v, out_c = np.full((h, w), 7.0, F), np.full((h, w, 3), 7.0, F)
    P = lambda a: C.c_void_p(a.ctypes.data)
    dp, np_, xp, ap, ep = (P(g[k]) for k in ("depth", "normal", "ids", "albedo", "emitted"))
    nan, inf = float("nan"), float("inf")

    def untouched():
        assert (out_v == 7.0).all() and (out_c == 7.0).all()

    # rtw_variance_estimate(moments, len, w, h, depth, normal, idx, params, out, stats)
    def vprm(mh=4, r=3, sd=0.5, sn=0.5, same=1):
        return C.byref(R.RtwVarianceEstimate(mh, r, sd, sn, same))

    def v_refused(*args):
        assert variance_call(*head, *args) == -1, args
        untouched()

    mp, lp, ovp = P(moments), P(length), P(out_v)
    v_refused(None, lp, w, h, dp, np_, xp, vprm(), ovp, None)
    v_refused(mp, None, w, h, dp, np_, xp, vprm(), ovp, None)
    v_refused(mp, lp, w, h, dp, np_, xp, vprm(), None, None)
    v_refused(mp, lp, w, h, dp, np_, xp, None, ovp, None)
    v_refused(mp, lp, 0, h, dp, np_, xp, vprm(), ovp, None)
    v_refused(mp, lp, w, 0, dp, np_, xp, vprm(), ovp, None)
    v_refused(mp, lp, 65536, 65536, dp, np_, xp, vprm(), ovp, None)
    v_refused(mp, lp, 0x7FFFFC01, 1, dp, np_, xp, vprm(), ovp, None)
    for mh in (0, 65536):
        v_refused(mp, lp, w, h, dp, np_, xp, vprm(mh=mh), ovp, None)
    for r in (0, R.VARIANCE_MAX_RADIUS + 1):
        v_refused(mp, lp, w, h, dp, np_, xp, vprm(r=r), ovp, None)
    for v in (-1.0, nan, inf, 1e-30):
        v_refused(mp, lp, w, h, dp, np_, xp, vprm(sd=v), ovp, None)
        v_refused(mp, lp, w, h, dp, np_, xp, vprm(sn=v), ovp, None)
    v_refused(mp, lp, w, h, None, np_, xp, vprm(), ovp, None)
    v_refused(mp, lp, w, h, dp, None, xp, vprm(), ovp, None)
    v_refused(mp, lp, w, h, dp, np_, None, vprm(), ovp, None)
    v_refused(mp, lp, w, h, dp, np_, xp, vprm(same=2), ovp, None)
    before = (moments.copy(), length.copy())
    assert variance_call(*head, mp, lp, w, h, dp, np_, xp, vprm(), mp, None) == -1              # out aliasing moments or len
    assert variance_call(*head, mp, lp, w, h, dp, np_, xp, vprm(), lp, None) == -1
    assert same_bits(moments, before[0]) and same_bits(length, before[1])
    assert variance_call(*head, mp, lp, w, h, None, None, None, vprm(sd=0.0, sn=0.0, same=0), ovp, None) == 0     # off terms: NULL guides
    assert same_bits(out_v, R.variance_estimate(moments, length, min_history=4, radius=3)[0])
    out_v[:] = 7.0

    # rtw_svgf_filter(in, variance, w, h, depth, normal, idx, albedo, emitted, params, vparams, out, out_variance, stats)
    def aprm(levels=3, sc=0.5, sd=0.5, sn=0.5, same=1, floor=FLOOR):
        return C.byref(R.RtwAtrous(levels, sc, sd, sn, same, floor))

    def sprm(sl=SIGMA_LUM, eps=EPSILON, pre=1):
        return C.byref(R.RtwSvgf(sl, eps, pre))

    def f_refused(*args):
        assert filter_call(*head, *args) == -1, args
        untouched()

    ip, vp, ocp = P(frame), P(variance), P(out_c)
    f_refused(None, vp, w, h, dp, np_, xp, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, None, w, h, dp, np_, xp, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, None, sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(), None, ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(), sprm(), None, ovp, None)
    f_refused(ip, vp, 0, h, dp, np_, xp, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, 0, dp, np_, xp, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, vp, 65536, 65536, dp, np_, xp, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(levels=0), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(levels=R.ATROUS_MAX_LEVELS + 1), sprm(), ocp, ovp, None)
    for v in (-1.0, nan, inf, 1e-30):
        f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(sc=v), sprm(), ocp, ovp, None)
        f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(sd=v), sprm(), ocp, ovp, None)
        f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(sn=v), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, None, np_, xp, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, None, xp, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, None, ap, ep, aprm(), sprm(), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(same=2), sprm(), ocp, ovp, None)
    for v in (0.0, -0.5, nan, inf):
        f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(floor=v), sprm(), ocp, ovp, None)
    for v in (-1.0, -1e-30, nan, inf, 1e20):                                                     # (2 * 1e20^2 overflows)
        f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(), sprm(sl=v), ocp, ovp, None)
    for v in (0.0, -1e-6, nan, inf):
        f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(), sprm(eps=v), ocp, ovp, None)
    f_refused(ip, vp, w, h, dp, np_, xp, ap, ep, aprm(), sprm(pre=2), ocp, ovp, None)
    before = (frame.copy(), variance.copy())
    for alias in (vp, ip):                                                                       # out_variance aliasing variance, in ...
        assert filter_call(*head, ip, vp, w, h, dp, np_, xp, ap, ep, aprm(), sprm(), ocp, alias, None) == -1
    assert filter_call(*head, ip, vp, w, h, dp, np_, xp, ap, ep, aprm(), sprm(), ocp, ocp, None) == -1      # ... or out
    untouched()
    assert same_bits(frame, before[0]) and same_bits(variance, before[1])
    # accepted: off terms with NULL guides, no albedo, no out_variance, no stats
    assert filter_call(*head, ip, vp, w, h, None, None, None, None, None, aprm(sd=0.0, sn=0.0, same=0, floor=0.0), sprm(), ocp, None, None) == 0
    assert same_bits(out_c, R.svgf_filter(frame, variance, levels=3, sigma_color=0.5, sigma_luminance=SIGMA_LUM, epsilon=EPSILON, prefilter=True)[0])
    untouched_v = (out_v == 7.0).all()
    assert untouched_v
