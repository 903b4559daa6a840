"""Float64 references of the a-trous filter, the variance estimate, the variance-steered a-trous filter and the blending half of the
temporal accumulation, each with an error bound derived from the roundings of the float32 rule (tests/test_filter_f64_cpu.py,
tests/test_gpu_filter_f64.py).  numpy only: nothing here imports the library, so the references, their bounds, the condition on the
inputs and the table of wrong rules can all be examined before a single library call.  Written from the text of include/rtw.h.

Every reference returns (value, bound): the value in float64 from the float32 inputs taken as exact, and beside it, per pixel (per
channel for a colour), a bound on |what the float32 rule gives - value|.

The rounding model.  u = 2^-24 is the unit roundoff of float32; the build does not fuse, so every written operation rounds once and a
computed x op y is (x op y)(1 + d), |d| <= u.  Where an operand already carries an error e the rounding is charged on |value| + e, and the
error of a square is (2|x| + e) e, so these parts are bounds and not first-order estimates.  exp_plain is 0.95 ulp off at the most
(tests/test_guided_cpu.py), and an ulp is at most 2u of the value.  A parameter formed on the float32 side (inv_x = 0.5f / (s * s), sl2)
carries the roundings of its operations.

The weight of a tap.  Its exponent a is a sum of non-negative terms, and a term's error comes from the operands it is formed from: a
difference d of two float32 inputs is off by u|d| (plus the inputs' own errors, which are 0 when the level reads float32 buffers), its
square by (2|d| + e) e + u d^2, the sum (x + y) + z of three squares by the three errors and two roundings, and the product with inv_x
by inv_x's two roundings and its own.  The luminance term (dl*dl) / den is no sum of non-negative parts: lum = (k0 r + k1 g) + k2 b is
off by 3u times the size of its three products (|k0 r| + |k1 g| + |k2 b|: three products, two sums, each partial sum no larger than
that size), dl = lum[q] - lum[p] by both of these and u|dl| -- an error that does not shrink with |dl| -- and the quotient is bounded
as ((dl^2 + e) / (den - e_den))(1 + u) - dl^2 / den.  With e_a the error of a, the computed weight is w (1 + dw_q),
    1 + dw_q = exp(e_a) (1 + 2 * 0.95 u) (1 + u)             (the exponent, exp_plain, the product with the kernel weight, which is exact)
and dw_q = 1 where the float64 weight is below 2^-120: the float32 side may have flushed it and dropped the tap.

A weighted mean out = sum(w c) / sum(w) over n counted taps.  With the computed weights w_q (1 + d_q), |d_q| <= dw_q, and exact
arithmetic, out' - out = sum(w_q d_q (c_q - out)) / sum(w_q (1 + d_q)): the mean of the weights' errors cancels, what is left is
    sum(w_q dw_q |c_q - out|) / sum(w)                                                                        to first order in dw.
The float32 sums add: every product c_q w_q rounds once and then passes through at most n - 1 additions, n u sum(w|c|) / sum(w) on the
numerator at the very worst; the denominator's n - 1 additions of positive terms shift out by (n - 1) u |out| <= (n - 1) u sum(w|c|) /
sum(w); the division rounds once.  That is (2n) u sum(w|c|) / sum(w) in the worst case and about half of it when the weight is
spread over the taps, and the bound used is
    2 * ( sum(w_q dw_q |c_q - out|) / sum(w)  +  (n + 3) u sum(w_q |c_q|) / sum(w) )
whose factor 2 (SAFETY) covers the worst case of the sums ((2n + 6) u >= 2n u) and the second-order terms of the first part
(1 / (1 - max dw), and dw is below 1e-3 wherever a tap carries weight).  Where the taps c_q carry errors e_q of their own (the
demodulated colour of a whole call) sum(w_q e_q) / sum(w) is added inside the bracket; and n 2^-126 / sum(w) for the products that
may underflow.  The variance channel vs / (wsum*wsum) has no such cancellation: its bound is the plain sum of
    the terms' errors ((1 + dw)^2 (1 + u)^2 - 1 each, or 1 where (wt*wt) V may have underflowed),  n - 1 additions,
    the relative error of wsum, sum(w dw) / sum(w) + (n - 1) u, twice and once more for wsum*wsum,  and the division,
times the same factor 2.  The variance V = M2 - M1*M1 of two moments with errors e1, e2 is off by e2 + (2|M1| + e1) e1 + u M1^2 + u|V|:
for a pixel of luminance L this is an absolute floor of about L^2 u however small the variance is, and it is inherent in float32
moments ("accuracy").

One level at a time.  Without albedo and emission the remodulation is the identity, so out(levels = i) and out_variance(levels = i) are
exactly level i's inputs: a test checks out(levels = i + 1) against level i of the reference applied to the float32 out(levels = i), and
no bound compounds.  Albedo, emission and the floor are tested at levels = 1 (ref_atrous_call64, ref_svgf_call64), where demodulate,
level 0 and remodulate are one bounded step.

The wrong rules (MUTANTS) are variants of these references, selected by `mutant`; tests/test_filter_f64_cpu.py shows that each lies
outside the bound somewhere in the matrix."""
import functools

import numpy as np

D, F = np.float64, np.float32
U = 2.0 ** -24                       # the unit roundoff of float32
EXP_ULP = 0.95                       # exp_plain's largest error in ulp (tests/test_guided_cpu.py)
SAFETY = 2.0                         # the factor on every bound (module docstring)
FLUSH = 2.0 ** -120                  # a weight below this may have been flushed on the float32 side
TINY = 2.0 ** -126                   # the smallest normal float32: what a product that underflows can lose
CONDITION_LINE = 2.0 ** -12          # a bound above this share of the largest value in the pixel's window is no statement ...
CONDITION_CAP = 0.05                 # ... and at most this share of a case's pixels may have one

SHAPES = [(1, 1), (3, 5), (17, 33), (33, 17)]               # (h, w); the larger two keep taps inside the frame at step 16
GPU_SHAPES = [(17, 33), (33, 17), (16, 32)]                 # 2 x 2 ragged workgroups both ways, and exactly one 32 x 16 tile
N_LEVELS = 5
SIGMA_COLOR, SIGMA_DEPTH, SIGMA_NORMAL, FLOOR = 0.75, 0.5, 0.6, 0.05
SIGMA_LUM, EPSILON = 1.5, 1e-5
RADII = [1, 3]
MIN_HISTORIES = [1, 4]
N_FRAMES = 6
TEMPORAL_CASES = [(0.0, 0.35, 4), (0.0, 0.35, 64), (0.2, 0.0, 4), (0.2, 0.0, 64)]          # (alpha, alpha_moments, max_history)

# Which term sets run at which level: every set at all five.  The colour sigma halves per level, but so does the noise the levels before
# have left; the depth term widens by 2^-i; the normal, object and luminance terms keep their width, and the objects lie in bands along
# the frame's longer side, so that a tap 16 pixels away can be on the centre's object.  With the colour term alone the taps beside the
# centre carry 85, 85, 79, 71 and 39 % of the weight sum at the median pixel of levels 0 .. 4.  tests/test_filter_f64_cpu.py asserts per
# set and level that they carry more than u of it at more than 5 % of the pixels of the two larger frames (offcentre_share; measured:
# at 73 % of the pixels or more): below u of the sum a tap cannot move a float32 result, and the level would check one product and one
# division.
_T = lambda sc=0.0, sd=0.0, sn=0.0, same=False, sl=0.0, svgf=False: dict(
    sigma_color=sc, sigma_depth=sd, sigma_normal=sn, same_object=same, sigma_luminance=sl, svgf=svgf or sl > 0)
LEVEL_TERMS = {
    "color": _T(sc=SIGMA_COLOR),
    "depth": _T(sd=SIGMA_DEPTH),
    "normal": _T(sn=SIGMA_NORMAL),
    "idx": _T(same=True),
    "guides": _T(sd=SIGMA_DEPTH, sn=SIGMA_NORMAL, same=True),
    "all": _T(sc=SIGMA_COLOR, sd=SIGMA_DEPTH, sn=SIGMA_NORMAL, same=True),
    "var": _T(sl=SIGMA_LUM),
    "var+idx": _T(sl=SIGMA_LUM, same=True),
    "var+guides": _T(sl=SIGMA_LUM, sd=SIGMA_DEPTH, sn=SIGMA_NORMAL, same=True),
    "var+color": _T(sl=SIGMA_LUM, sc=SIGMA_COLOR),
    "guides,variance-channel": _T(sd=SIGMA_DEPTH, sn=SIGMA_NORMAL, same=True, svgf=True),   # the variance under the plain weights
}
# levels = 1 with albedo (and emission): name -> (term set, emitted)
CALL_TERMS = {
    "all+albedo": ("all", False),
    "all+albedo+emitted": ("all", True),
    "idx+albedo+emitted": ("idx", True),
    "var+albedo": ("var", False),
    "var+color+albedo+emitted": ("var+color", True),
    "var+guides+albedo+emitted": ("var+guides", True),
}
# name -> (sigma_depth, sigma_normal, same_object) of the variance estimate
VARIANCE_TERMS = {
    "none": (0.0, 0.0, False),
    "depth": (SIGMA_DEPTH, 0.0, False),
    "normal": (0.0, SIGMA_NORMAL, False),
    "idx": (0.0, 0.0, True),
    "all": (SIGMA_DEPTH, SIGMA_NORMAL, True),
}
LUM_709 = tuple(float(F(k)) for k in (0.2126, 0.7152, 0.0722))          # the rule's 0.2126f, 0.7152f, 0.0722f
LUM_601 = tuple(float(F(k)) for k in (0.299, 0.587, 0.114))

# The wrong rules: name -> (the pass whose reference takes it as `mutant`, what is wrong)
MUTANTS = {
    "outer-weight-1/8": ("level", "the tap kernel's outer weight is 1/8 instead of 1/16"),
    "depth-unscaled": ("level", "the depth difference is not scaled by 2^-i"),
    "sigma-color-not-halved": ("level", "sigma_color is not halved per level"),
    "step-linear": ("level", "the step is i + 1 instead of 2^i"),
    "border-clamped": ("level", "taps outside the frame are clamped to the border instead of skipped"),
    "albedo-floor-divides": ("call", "an albedo below the floor divides by the floor instead of by 1"),
    "emission-after-division": ("call", "emission is subtracted after the division"),
    "gate-ignored-on-miss": ("level", "the same-object gate is ignored where the id is -1"),
    "no-boost": ("estimate", "the estimate has no min_history / n boost"),
    "holes-enter": ("estimate", "holes (length 0) enter the window"),
    "spatial-at-min-history": ("estimate", "the spatial branch is taken at n == min_history"),
    "per-tap-variances": ("estimate", "the estimate averages per-tap variances instead of taking the variance of the averaged moments"),
    "variance-sum-wt": ("level", "the filter's variance sum uses wt instead of wt*wt"),
    "variance-by-wsum": ("level", "the variance is divided by wsum instead of wsum*wsum"),
    "prefilter-not-renormalised": ("level", "the prefilter is not renormalised at the frame's border"),
    "den-sqrt": ("level", "the luminance denominator is sigma_luminance * sqrt(vbar) + epsilon"),
    "rec601": ("level", "Rec. 601 luminance coefficients are used"),
    "variance-remodulated-by-la": ("call", "the variance is remodulated by la instead of la*la"),
    "prefilter-reads-call-input": ("level", "the prefilter reads the call's input variance at every level instead of the level's own"),
    "moments-use-alpha": ("temporal", "the moments are blended with alpha instead of alpha_moments"),
    "m2-from-blended-colour": ("temporal", "the second moment is formed from the blended colour's luminance"),
}


# ---- comparing -----------------------------------------------------------------------------------------------------------------------------
def share(got, value, bound):
    """The largest |got - value| / bound over the pixels: 0 where both are 0, inf where an error meets a bound of 0."""
    err = np.abs(np.asarray(got, D) - value)
    with np.errstate(all="ignore"):
        s = np.where(err == 0, 0.0, err / bound)
    return float(s.max())


def holds(got, value, bound):
    """The assertion of the CPU and the GPU tests alike: every entry of `got` within its own bound of the float64 value."""
    got = np.asarray(got)
    return got.shape == value.shape and bool(np.isfinite(got).all()) and share(got, value, bound) <= 1.0


def where_worst(got, value, bound):
    err = np.abs(np.asarray(got, D) - value)
    with np.errstate(all="ignore"):
        s = np.where(err == 0, 0.0, err / bound)
    at = np.unravel_index(int(np.argmax(s)), s.shape)
    return f"worst at {tuple(int(k) for k in at)}: got {np.asarray(got)[at]!r}, float64 {value[at]!r}, bound {bound[at]:.3e}, share {s[at]:.3f}"


# ---- values with errors ----------------------------------------------------------------------------------------------------------------------
def _sub(x, ex, y, ey):
    d = x - y
    e = ex + ey
    return d, e + U * (np.abs(d) + e)


def _sq(x, ex):
    s = x * x
    e = (2.0 * np.abs(x) + ex) * ex
    return s, e + U * (s + e)


def _sq3(d, ed):
    """(d.x*d.x + d.y*d.y) + d.z*d.z"""
    s, e = _sq(d, ed)
    t, e = s.sum(-1), e.sum(-1)
    return t, e + 2.0 * U * (t + e)


def _lum(c, ec, coef=LUM_709):
    """(k0 r + k1 g) + k2 b: three products, two sums whose partial sums are no larger than the size of the three products."""
    p = [coef[k] * c[..., k] for k in range(3)]
    ep = [coef[k] * ec[..., k] + U * (np.abs(p[k]) + coef[k] * ec[..., k]) for k in range(3)]
    size = sum(np.abs(q) for q in p) + sum(ep)
    return (p[0] + p[1]) + p[2], sum(ep) + 2.0 * U * size


def _inv(sigma):
    """inv_x = 0.5f / (sigma * sigma) and its relative error: one product, one division."""
    s = float(F(sigma))
    return 0.5 / (s * s), (1.0 + U) ** 2 - 1.0


def _scaled(x, ex, k, rel_k):
    """k * x for a positive parameter k with relative error rel_k, x >= 0."""
    t = k * x
    e = k * ex + rel_k * k * (x + ex)
    return t, e + U * (t + e)


def _taps(h, w, reach, step, clamp=False):
    """For each tap of a (2 reach + 1)^2 window stepping by `step`, dy outer, dx inner: (dx, dy, qy, qx, inside) over the whole frame,
    qy, qx clamped into it, `inside` the centres whose tap lies inside; with clamp every tap counts where it was clamped to."""
    yy, xx = np.mgrid[0:h, 0:w]
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            qy, qx = yy + dy * step, xx + dx * step
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            if clamp:
                inside = np.ones_like(inside)
            elif not inside.any():
                continue
            yield dx, dy, np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1), inside


def _weight(a, ea, hw):
    """w = hw * exp_plain(-a) and its relative error (module docstring)."""
    wt = hw * np.exp(-a)
    with np.errstate(over="ignore"):                                            # (a dead tap's exp(e_a) may overflow: its dw is 1)
        dw = np.exp(ea) * (1.0 + 2.0 * EXP_ULP * U) * (1.0 + U) - 1.0
    return wt, np.where(wt < FLUSH, 1.0, dw)


def _mean_bound(wt, dw, x, ex, out, wsum, n):
    """The bracket of the weighted mean's bound (module docstring), before SAFETY.  wt, dw [taps][h][w]; x, ex [taps][h][w](+ channels)."""
    if x.ndim > wt.ndim:
        wt, dw, wsum, n = wt[..., None], dw[..., None], wsum[..., None], n[..., None]
    return ((wt * dw * np.abs(x - out)).sum(0) + (wt * ex).sum(0) + (n + 3.0) * U * (wt * np.abs(x)).sum(0) + n * TINY) / wsum


def _guide_terms(a, ea, g, p, qy, qx, scale, first):
    """Adds the depth and the normal term to the exponent (a, ea); `first`: nothing has been added to a yet (0 + t is exact)."""
    if p["sigma_depth"] > 0:
        d, ed = _sub(g["depth"][qy, qx], 0.0, g["depth"], 0.0)
        d, ed = d * scale, ed * scale                                           # (a power of two: exact)
        t, et = _scaled(*_sq(d, ed), *_inv(p["sigma_depth"]))
        a, ea, first = a + t, ea + et + (0.0 if first else U * (a + t + ea + et)), False
    if p["sigma_normal"] > 0:
        d, ed = _sub(g["normal"][qy, qx], 0.0, g["normal"], 0.0)
        t, et = _scaled(*_sq3(d, ed), *_inv(p["sigma_normal"]))
        a, ea, first = a + t, ea + et + (0.0 if first else U * (a + t + ea + et)), False
    return a, ea, first


def _level(c, ec, v, ev, g, i, p, mutant=None, v_call=None, probe=None):
    """One level of the (variance-steered) a-trous rule on colour c +- ec [h][w][3] and, with v not None, variance v +- ev [h][w]:
    (colour, its bound before SAFETY, variance or None, its bound before SAFETY or None)."""
    h, w, _ = c.shape
    K = [0.375, 0.25, 0.125 if mutant == "outer-weight-1/8" else 0.0625]
    step = i + 1 if mutant == "step-linear" else 1 << i
    scale = 1.0 if mutant == "depth-unscaled" else 2.0 ** -i
    sl = float(F(p["sigma_luminance"])) if v is not None else 0.0
    coef = LUM_601 if mutant == "rec601" else LUM_709
    if p["sigma_color"] > 0:
        inv_color, rel_color = _inv(float(F(p["sigma_color"])) * (1.0 if mutant == "sigma-color-not-halved" else 2.0 ** -i))
    if sl > 0:
        vin, evin = (np.asarray(v_call, D), np.zeros_like(ev)) if mutant == "prefilter-reads-call-input" and p["prefilter"] else (v, ev)
        if p["prefilter"]:
            G = [0.5, 0.25]
            num, enum, gs, n3 = (np.zeros((h, w)) for _ in range(4))
            for dx, dy, qy, qx, inside in _taps(h, w, 1, 1):
                gw = G[abs(dx)] * G[abs(dy)]
                num, enum, gs, n3 = num + inside * gw * vin[qy, qx], enum + inside * gw * evin[qy, qx], gs + inside * gw, n3 + inside
            if mutant == "prefilter-not-renormalised":
                gs = np.ones_like(gs)
            vbar = num / gs
            evbar = enum / gs + n3 * U * (vbar + enum / gs)                     # n3 - 1 additions and the division; the products are exact
        else:
            vbar, evbar = vin, evin
        sl2, rel_sl2 = 2.0 * sl * sl, (1.0 + U) ** 2 - 1.0
        eps = float(F(p["epsilon"]))
        if mutant == "den-sqrt":
            den, eden = sl * np.sqrt(vbar) + eps, 0.0
        else:
            prod, eprod = _scaled(vbar, evbar, sl2, rel_sl2)
            den = prod + eps
            eden = eprod + U * (den + eprod)
        lum, el = _lum(c, ec, coef)
    W, DW, CQ, EQ, VQ, EVQ = [], [], [], [], [], []
    for dx, dy, qy, qx, inside in _taps(h, w, 2, step, clamp=mutant == "border-clamped"):
        a, ea, first = np.zeros((h, w)), np.zeros((h, w)), True
        if p["sigma_color"] > 0:
            d, ed = _sub(c[qy, qx], ec[qy, qx], c, ec)
            a, ea = _scaled(*_sq3(d, ed), inv_color, rel_color)
            first = False
        a, ea, first = _guide_terms(a, ea, g, p, qy, qx, scale, first)
        if sl > 0:
            dl, edl = _sub(lum[qy, qx], el[qy, qx], lum, el)
            s, es = _sq(dl, edl)
            t = s / den
            et = (s + es) / (den - eden) * (1.0 + U) - t
            a, ea = a + t, ea + et + (0.0 if first else U * (a + t + ea + et))
        wt, dw = _weight(a, ea, K[abs(dx)] * K[abs(dy)])
        if p["same_object"]:
            other = g["ids"][qy, qx] != g["ids"]
            if mutant == "gate-ignored-on-miss":
                other &= (g["ids"][qy, qx] != -1) & (g["ids"] != -1)
            wt = np.where(other, 0.0, wt)
        W.append(np.where(inside, wt, 0.0))
        DW.append(dw)
        CQ.append(c[qy, qx])
        EQ.append(ec[qy, qx])
        if v is not None:
            VQ.append(v[qy, qx])
            EVQ.append(ev[qy, qx])
    W, DW, CQ, EQ = np.array(W), np.array(DW), np.array(CQ), np.array(EQ)
    wsum, n = W.sum(0), (W > 0).sum(0).astype(D)
    if probe is not None:
        probe["wsum"] = wsum
    out = (W[..., None] * CQ).sum(0) / wsum[..., None]
    bound = _mean_bound(W, DW, CQ, EQ, out, wsum, n)
    if v is None:
        return out, bound, None, None
    VQ, EVQ = np.array(VQ), np.array(EVQ)
    W2 = W if mutant == "variance-sum-wt" else W * W
    terms = W2 * VQ
    rel = np.where((terms < FLUSH) & (terms > 0), 1.0, (1.0 + DW) ** 2 * (1.0 + U) ** 2 - 1.0)
    vs = terms.sum(0)
    evs = (terms * rel).sum(0) + (W2 * EVQ).sum(0)
    evs = evs + (n - 1.0) * U * (vs + evs)
    rel_wsum = (W * DW).sum(0) / wsum + (n - 1.0) * U
    ww, rel_ww = (wsum, rel_wsum) if mutant == "variance-by-wsum" else (wsum * wsum, (1.0 + rel_wsum) ** 2 * (1.0 + U) - 1.0)
    vout = vs / ww
    top = (vs + evs) / (ww * (1.0 - rel_ww))
    return out, bound, vout, (top - vout) + U * top


def _params(params):
    p = dict(sigma_color=0.0, sigma_depth=0.0, sigma_normal=0.0, same_object=False, sigma_luminance=0.0, epsilon=EPSILON, prefilter=False,
             albedo_floor=FLOOR)
    p.update(params)
    return p


def ref_atrous_level64(c, guides, i, params, mutant=None):
    """Level i of include/rtw.h "a-trous filter" on the float32 colour c [h][w][3]: (value, bound), both [h][w][3] float64.
    guides: dict(depth, normal, ids); params: sigma_color (the call's: the level halves it i times), sigma_depth, sigma_normal,
    same_object."""
    c = np.asarray(c, D)
    out, bound, _, _ = _level(c, np.zeros_like(c), None, None, guides, i, _params(params), mutant)
    return out, SAFETY * bound


def ref_svgf_level64(c, v, guides, i, params, mutant=None, v_call=None):
    """Level i of include/rtw.h "variance-steered a-trous filter" on the float32 colour c and variance v [h][w], the 3 x 3 prefilter
    inside: ((colour, bound), (variance, bound)).  params as ref_atrous_level64 plus sigma_luminance, epsilon, prefilter.  v_call: the
    call's input variance, which only the wrong rule "prefilter-reads-call-input" reads."""
    c, v = np.asarray(c, D), np.asarray(v, D)
    out, bound, vout, vbound = _level(c, np.zeros_like(c), v, np.zeros_like(v), guides, i, _params(params), mutant, v_call)
    return (out, SAFETY * bound), (vout, SAFETY * vbound)


def _demodulate(frame, albedo, emitted, p, mutant):
    """C0 = (in - e) / a with its error, a, e, and la*la with its relative error."""
    frame = np.asarray(frame, D)
    floor = float(F(p["albedo_floor"]))
    a = np.where(np.asarray(albedo, D) >= floor, albedo, floor if mutant == "albedo-floor-divides" else 1.0).astype(D)
    e = np.asarray(emitted, D) if emitted is not None else np.zeros_like(frame)
    if mutant == "emission-after-division":
        c0 = frame / a - e
    else:
        c0 = (frame - e) / a
    ec0 = ((1.0 + U) ** 2 - 1.0) * np.abs(c0)                                   # the subtraction and the division
    la, ela = _lum(a, np.zeros_like(a), LUM_601 if mutant == "rec601" else LUM_709)
    la2, ela2 = _sq(la, ela)
    return c0, ec0, a, e, la, la2, ela2 / la2


def _remodulate(out, bound, a, e):
    prod = out * a
    eprod = bound * a + U * (np.abs(prod) + bound * a)
    res = prod + e
    return res, eprod + U * (np.abs(res) + eprod)


def ref_atrous_call64(frame, guides, albedo, emitted, params, mutant=None):
    """A whole call of the a-trous filter at levels = 1 with albedo (and emission): demodulate, level 0, remodulate as one bounded
    step.  (value, bound)."""
    p = _params(params)
    c0, ec0, a, e, _, _, _ = _demodulate(frame, albedo, emitted, p, mutant)
    out, bound, _, _ = _level(c0, ec0, None, None, guides, 0, p, mutant)
    res, eres = _remodulate(out, bound, a, e)
    return res, SAFETY * eres


def ref_svgf_call64(frame, variance, guides, albedo, emitted, params, mutant=None):
    """A whole call of the variance-steered filter at levels = 1 with albedo (and emission): ((colour, bound), (variance, bound))."""
    p = _params(params)
    c0, ec0, a, e, la, la2, rel_la2 = _demodulate(frame, albedo, emitted, p, mutant)
    variance = np.asarray(variance, D)
    v0 = np.where(variance > 0, variance / la2, 0.0)
    ev0 = v0 / (1.0 - rel_la2) * (1.0 + U) - v0
    out, bound, vout, vbound = _level(c0, ec0, v0, ev0, guides, 0, p, mutant, v_call=v0)
    res, eres = _remodulate(out, bound, a, e)
    back, rel_back = (la, rel_la2) if mutant == "variance-remodulated-by-la" else (la2, rel_la2)
    vres = vout * back
    top = (vout + vbound) * back * (1.0 + rel_back) * (1.0 + U)
    return (res, SAFETY * eres), (vres, SAFETY * (top - vres))


def _moment_variance(m1, e1, m2, e2):
    """V = m2 - m1*m1, clamped at 0 (the clamp moves no error)."""
    sq, esq = _sq(m1, e1)
    v, ev = _sub(m2, e2, sq, esq)
    return np.maximum(v, 0.0), ev


def ref_variance64(moments, length, guides, params, mutant=None):
    """include/rtw.h "variance estimate", both branches: (value, bound) [h][w].  params: min_history, radius, sigma_depth, sigma_normal,
    same_object."""
    p = _params(params)
    moments, n = np.asarray(moments, D), np.asarray(length, D)
    h, w = n.shape
    m1, m2 = moments[..., 0], moments[..., 1]
    zero = np.zeros((h, w))
    vt, evt = _moment_variance(m1, zero, m2, zero)
    W, DW, Q1, Q2 = [], [], [], []
    for _dx, _dy, qy, qx, inside in _taps(h, w, int(p["radius"]), 1):
        a, ea, _ = _guide_terms(zero, zero, guides, p, qy, qx, 1.0, True)
        wt = np.exp(-a)
        dw = np.where(wt < FLUSH, 1.0, np.exp(ea) * (1.0 + 2.0 * EXP_ULP * U) - 1.0)
        if p["same_object"]:
            wt = np.where(guides["ids"][qy, qx] != guides["ids"], 0.0, wt)
        counted = inside if mutant == "holes-enter" else inside & (n[qy, qx] > 0)
        W.append(np.where(counted, wt, 0.0))
        DW.append(dw)
        Q1.append(m1[qy, qx])
        Q2.append(m2[qy, qx])
    W, DW, Q1, Q2 = np.array(W), np.array(DW), np.array(Q1), np.array(Q2)
    ws, taps = W.sum(0), (W > 0).sum(0).astype(D)
    safe = np.where(ws > 0, ws, 1.0)
    M1, M2 = (W * Q1).sum(0) / safe, (W * Q2).sum(0) / safe
    e1 = _mean_bound(W, DW, Q1, np.zeros_like(Q1), M1, safe, taps)
    e2 = _mean_bound(W, DW, Q2, np.zeros_like(Q2), M2, safe, taps)
    if mutant == "per-tap-variances":
        vsp, evsp = (W * np.maximum(Q2 - Q1 * Q1, 0.0)).sum(0) / safe, zero
    else:
        vsp, evsp = _moment_variance(M1, e1, M2, e2)
    boost = 1.0 if mutant == "no-boost" else float(p["min_history"]) / np.where(n >= 1, n, 1.0)
    spatial = vsp * boost
    espatial = (vsp + evsp) * boost * (1.0 + U) ** 2 - spatial                  # the division and the product
    spatial, espatial = np.where(ws > 0, spatial, 0.0), np.where(ws > 0, espatial, 0.0)
    long_enough = n > p["min_history"] if mutant == "spatial-at-min-history" else n >= p["min_history"]
    return np.where(long_enough, vt, spatial), SAFETY * np.where(long_enough, evt, espatial)


def _blend_factors(n_frames, alpha, max_history):
    """a_k of frame k = 1 .. n_frames: 1 / k while the length has not saturated and 1 / k is not below the floor, the floor after."""
    alpha = float(F(alpha))
    return [max(1.0 / min(k, max_history), alpha) for k in range(1, n_frames + 1)]


def _closed_form(x, factors):
    """x [frames]...: the running mean of the first K frames, K the last k with a_k = 1 / k, then the exponential average with the
    constant factor a* of the frames after:  (1 - a*)^(N - K) mean(x_1 .. x_K) + sum_{k > K} a* (1 - a*)^(N - k) x_k."""
    N = len(factors)
    K = max(k for k in range(1, N + 1) if factors[k - 1] == 1.0 / k)
    if K == N:
        return x[:K].mean(0)
    a = factors[K]
    assert all(f == a for f in factors[K:])                                     # (once at the floor the factor stays there)
    return (1.0 - a) ** (N - K) * x[:K].mean(0) + sum(a * (1.0 - a) ** (N - k) * x[k - 1] for k in range(K + 1, N + 1))


def _blend_error(eh, hval, x, ex, a):
    """The error of h + (x - h) * a given the history's eh and the sample's ex: the history's share (1 - a) of the old error, the
    sample's share, the roundings of the subtraction, of a = 1 / n and of the product (each u on |x - h| a), and of the sum."""
    d = np.abs(x - hval) + eh + ex
    out = hval + (x - hval) * a
    e = eh * (1.0 - a) + ex * a + 3.0 * U * a * d
    return out, e + U * (np.abs(out) + e)


def ref_temporal_stats64(frames, alpha, alpha_moments, max_history, mutant=None):
    """What include/rtw.h "temporal accumulation" promises of frames [n][h][w][3] under a static camera with every guide test off: each
    pixel's one tap of weight 1 is its own history, so after n frames
      colour  = the closed form (_closed_form) of the frames with the factors of alpha,
      moments = the same of L_k and L_k^2, L = lum(frame), with the factors of alpha_moments,
      variance = m2 - m1^2 when > 0 else 0,  length = min(n, max_history).
    dict(color, moments, variance, len) of (value, bound); the bounds follow the recurrence step by step (_blend_error)."""
    frames = np.asarray(frames, D)
    N = len(frames)
    fc = _blend_factors(N, alpha, max_history)
    fm = fc if mutant == "moments-use-alpha" else _blend_factors(N, alpha_moments, max_history)
    L, eL = _lum(frames, np.zeros_like(frames))
    L2, eL2 = _sq(L, eL)
    color, m1, m2 = _closed_form(frames, fc), _closed_form(L, fm), _closed_form(L2, fm)
    hc, ec, h1, e1, h2, e2 = frames[0], np.zeros_like(frames[0]), L[0], eL[0], L2[0], eL2[0]
    for k in range(1, N):
        hc, ec = _blend_error(ec, hc, frames[k], 0.0, fc[k])
        h1, e1 = _blend_error(e1, h1, L[k], eL[k], fm[k])
        x2, ex2 = (L2[k], eL2[k]) if mutant != "m2-from-blended-colour" else _sq(*_lum(hc, ec))
        h2, e2 = _blend_error(e2, h2, x2, ex2, fm[k])
    if mutant == "m2-from-blended-colour":
        m2 = h2                                                                  # (the wrong rule has no closed form: its recurrence)
    else:                                                                        # the closed form is the rule's recurrence, to float64's roundings:
        eps = 4.0 * N * np.finfo(D).eps                                          # a subtraction, a product, a sum and a_k per step
        assert np.abs(hc - color).max() <= eps * frames.max() and np.abs(h1 - m1).max() <= eps * L.max() and np.abs(h2 - m2).max() <= eps * L2.max()
    var, evar = _moment_variance(m1, e1, m2, e2)
    length = np.full(frames.shape[1:3], float(min(N, max_history)))
    return dict(color=(color, SAFETY * ec), moments=(np.stack([m1, m2], -1), SAFETY * np.stack([e1, e2], -1)),
                variance=(var, SAFETY * evar), len=(length, np.zeros_like(length)))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(h, w):
    """A finite noisy frame with values in [0, 1] over three objects and a miss region (idx -1, normal 0 0 0, albedo 0 0 0, the far
    depth), one firefly of 40 and one run of equal pixels; depth and normals in the style of tests/atrous_common.py; albedo channels
    below, at and above the floor; emission on one object.  Read-only arrays."""
    rng = np.random.default_rng(64000 + h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    ids = (((yy if h <= w else xx) * 4) // min(h, w)).astype(np.int32) - 1                          # -1 (miss), 0, 1, 2 in bands along the longer side,
    miss = ids < 0                                                                                 # so that a tap 16 pixels away can lie on the same object
    depth = (4.0 + 0.05 * xx + 0.11 * yy + 3.0 * ids + 0.02 * rng.standard_normal((h, w))).astype(F)
    depth[miss] = F(1600.0)
    normal = rng.standard_normal((h, w, 3)).astype(F) * F(0.15) + np.eye(3, dtype=F)[np.clip(ids, 0, 2)]
    normal = (normal / np.sqrt((normal * normal).sum(-1, keepdims=True))).astype(F)
    normal[miss] = 0.0
    albedo = (0.2 + 0.7 * rng.random((h, w, 3))).astype(F)
    albedo[miss] = 0.0
    emitted = np.zeros((h, w, 3), F)
    emitted[ids == 2] = rng.random((int((ids == 2).sum()), 3)).astype(F) * F(0.25)
    below, above = np.nextafter(F(FLOOR), F(0.0)), np.nextafter(F(FLOOR), F(1.0))
    flat = lambda a: a.reshape(-1, a.shape[-1]) if a.ndim == 3 else a.reshape(-1)
    n = h * w
    if n >= 15:
        spots = rng.choice(n, 4, replace=False)
        flat(albedo)[spots[0]] = (below, F(FLOOR), above)
        flat(albedo)[spots[1]] = (F(FLOOR), F(0.01), below)
        flat(albedo)[spots[2]] = (F(0.03), F(0.6), F(0.04))
    else:
        albedo[0, 0] = (below, F(FLOOR), 0.3)
    frame = (albedo * (0.3 + 0.5 * rng.random((h, w, 3))) + emitted + np.where(miss[..., None], 0.3 + 0.1 * rng.random((h, w, 3)), 0.0)).astype(F)
    if n >= 15:
        flat(frame)[spots[3]] = 40.0                                     # a firefly
        y, x = h // 2, max(0, w // 2 - 1)
        frame[y, x:x + 3] = frame[y, x]                                  # a run of equal pixels
    assert frame.min() >= 0.0 and ((frame > 1.0) == (frame == 40.0)).all()
    return _frozen(dict(frame=frame, depth=depth, normal=normal, ids=ids, albedo=albedo, emitted=emitted))


@functools.lru_cache(maxsize=None)
def variance_plane(h, w):
    """The filter's variance: 10^(-6 .. 1) per pixel, exact zeros over a block and at scattered pixels, the ends 1e-6 and 10 present."""
    rng = np.random.default_rng(65000 + h * 131 + w)
    v = (10.0 ** rng.uniform(-6.0, 1.0, (h, w))).astype(F)
    v[rng.random((h, w)) < 0.1] = 0.0
    v[h // 3:h // 3 + 3, w // 3:w // 3 + 4] = 0.0
    if h * w >= 15:
        v[0, 0], v[h - 1, w - 1], v[h - 1, 0] = 1e-6, 10.0, 0.0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def history(h, w):
    """(moments [h][w][2], length [h][w]) of the estimate: lengths 0 (holes), 1 .. 6 and fractions between, 4 (MIN_HISTORIES' larger
    entry) among them; the moments are those of ceil(length) samples base * (1 + 0.3 noise) of a luminance, a hole's are 0; two bright
    pixels of mean luminance about 40 with a variance of about 0.01, one with a long history and one with a short one."""
    rng = np.random.default_rng(66000 + h * 131 + w)
    lengths = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.0, 5.0, 6.0, 1.5, 2.25, 3.75, 4.5], F)
    length = lengths[rng.integers(0, len(lengths), (h, w))]
    base = 0.05 + 0.95 * rng.random((h, w))
    noise = 0.3 * rng.standard_normal((6, h, w))
    if h * w >= 15:
        for k, at in enumerate(rng.choice(h * w, 2, replace=False)):
            at = np.unravel_index(at, (h, w))
            base[at], noise[(slice(None),) + at], length[at] = 40.0, 0.0025 * rng.standard_normal(6), (6.0, 2.0)[k]
    else:
        length[0, 0] = 2.0
    samples = np.abs(base * (1.0 + noise))
    count = np.ceil(length).astype(int)
    use = np.arange(6)[:, None, None] < count
    m1 = (samples * use).sum(0) / np.maximum(count, 1)
    m2 = (samples * samples * use).sum(0) / np.maximum(count, 1)
    moments = np.stack([m1, m2], -1).astype(F)
    moments.setflags(write=False)
    length.setflags(write=False)
    return moments, length


@functools.lru_cache(maxsize=None)
def temporal_frames(h, w):
    """N_FRAMES noisy copies of inputs(h, w)'s frame, [n][h][w][3] float32, all positive; the firefly's pixel varies by a quarter of a
    percent only, a bright pixel with a small variance.  Read-only."""
    rng = np.random.default_rng(67000 + h * 131 + w)
    base = inputs(h, w)["frame"].astype(D)
    noise = 0.3 * rng.standard_normal((N_FRAMES, h, w, 3))
    noise[:, base.max(-1) > 1.0] *= 0.0025 / 0.3
    frames = np.abs(base * (1.0 + noise)).astype(F)
    frames.setflags(write=False)
    return frames


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------------
def guides_of(h, w):
    g = inputs(h, w)
    return dict(depth=g["depth"], normal=g["normal"], ids=g["ids"])


def rule_params(terms, prefilter=False):
    """The references' params of a term set."""
    t = LEVEL_TERMS[terms]
    return dict({k: t[k] for k in ("sigma_color", "sigma_depth", "sigma_normal", "same_object", "sigma_luminance")}, epsilon=EPSILON,
                prefilter=bool(prefilter), albedo_floor=FLOOR)


def library_kwargs(h, w, terms, levels, prefilter=False, albedo=False, emitted=False):
    """The keyword arguments of atrous_filter / svgf_filter (host form or Renderer) for a term set: a guide whose term is off is None."""
    t, g = LEVEL_TERMS[terms], inputs(h, w)
    kw = dict(depth=g["depth"] if t["sigma_depth"] > 0 else None, normal=g["normal"] if t["sigma_normal"] > 0 else None,
              ids=g["ids"] if t["same_object"] else None, albedo=g["albedo"] if albedo else None, emitted=g["emitted"] if emitted else None,
              levels=levels, sigma_color=t["sigma_color"], sigma_depth=t["sigma_depth"], sigma_normal=t["sigma_normal"],
              same_object=t["same_object"], albedo_floor=FLOOR)
    if t["svgf"]:
        kw.update(sigma_luminance=t["sigma_luminance"], epsilon=EPSILON, prefilter=bool(prefilter))
    return kw


def level_cases():
    """(terms, prefilter) of every chain of levels: the prefilter on and off wherever the luminance term reads it."""
    return [(name, pre) for name, t in LEVEL_TERMS.items() for pre in ((0, 1) if t["sigma_luminance"] > 0 else (0,))]


def call_cases():
    """(name, terms, emitted, prefilter) of the calls at levels = 1 with albedo."""
    return [(name, terms, emi, pre) for name, (terms, emi) in CALL_TERMS.items() for pre in ((0, 1) if LEVEL_TERMS[terms]["sigma_luminance"] > 0 else (0,))]


def variance_cases():
    return [(terms, mh, r) for terms in VARIANCE_TERMS for mh in MIN_HISTORIES for r in RADII]


def variance_params(terms, min_history, radius):
    sd, sn, same = VARIANCE_TERMS[terms]
    return dict(min_history=min_history, radius=radius, sigma_depth=sd, sigma_normal=sn, same_object=same)


def variance_library_kwargs(h, w, terms, min_history, radius):
    sd, sn, same = VARIANCE_TERMS[terms]
    g = inputs(h, w)
    return dict(depth=g["depth"] if sd > 0 else None, normal=g["normal"] if sn > 0 else None, ids=g["ids"] if same else None,
                min_history=min_history, radius=radius, sigma_depth=sd, sigma_normal=sn, same_object=same)


def check_level(terms, prefilter, h, w, i, c_in, v_in, c_out, v_out, v_call=None, mutant=None):
    """What every test of a level asserts: (c_out, v_out), the float32 outputs at levels = i + 1, against level i of the reference applied
    to the float32 (c_in, v_in), the outputs at levels = i.  Returns [(what, got, value, bound)]."""
    p, g = rule_params(terms, prefilter), guides_of(h, w)
    if not LEVEL_TERMS[terms]["svgf"]:
        return [("colour", c_out) + ref_atrous_level64(c_in, g, i, p, mutant)]
    (c, bc), (v, bv) = ref_svgf_level64(c_in, v_in, g, i, p, mutant, v_call)
    return [("colour", c_out, c, bc), ("variance", v_out, v, bv)]


@functools.lru_cache(maxsize=None)
def reference_chain(h, w, terms, prefilter):
    """The N_LEVELS levels of a term set chained through the reference alone: [(c_in, v_in, [(what, value, bound)])] per level, each
    level's float32 inputs the rounded values of the level before (the frame and variance_plane for level 0).  No library call: the
    inputs of the condition's test and of the wrong rules' test."""
    c, v = inputs(h, w)["frame"], variance_plane(h, w)
    chain = []
    for i in range(N_LEVELS):
        res = [(what, value, bound) for what, _, value, bound in check_level(terms, prefilter, h, w, i, c, v, None, None)]
        chain.append((c, v, res))
        c = res[0][1].astype(F)
        v = res[1][1].astype(F) if len(res) > 1 else v
    return chain


def offcentre_share(terms, prefilter, h, w, i, c_in, v_in):
    """Per pixel, the share of level i's weight sum that the taps beside the centre carry (the centre's weight is K[0]*K[0] = 9/64)."""
    c, probe = np.asarray(c_in, D), {}
    v = np.asarray(v_in, D) if LEVEL_TERMS[terms]["svgf"] else None
    _level(c, np.zeros_like(c), v, None if v is None else np.zeros_like(v), guides_of(h, w), i, _params(rule_params(terms, prefilter)), probe=probe)
    return 1.0 - 0.375 * 0.375 / probe["wsum"]


def window_max(x, reach, step):
    """The largest |x| over the taps of each pixel's window that lie inside the frame (all channels of a colour)."""
    x = np.abs(np.asarray(x, D))
    x = x.max(-1) if x.ndim == 3 else x
    h, w = x.shape
    out = np.zeros((h, w))
    for _dx, _dy, qy, qx, inside in _taps(h, w, reach, step):
        out = np.maximum(out, np.where(inside, x[qy, qx], 0.0))
    return out


def over_the_line(bound, scale):
    """The share of pixels with a bound (in any channel) above CONDITION_LINE times the largest absolute value in their window."""
    bound = bound.max(-1) if bound.ndim == 3 else bound
    return float((bound > CONDITION_LINE * scale).mean())


# ---- running a pass against its reference: the host forms and the kernels go through the same lines ---------------------------------------
def run_levels(atrous, svgf, h, w, terms, prefilter):
    """The N_LEVELS levels one at a time (module docstring): [(what, got, value, bound)].  atrous(frame, **kw) -> (out, ..), svgf(frame,
    variance, **kw) -> (out, out_variance, ..); each level's inputs are the callables' own outputs at one level less."""
    frame, variance = inputs(h, w)["frame"], variance_plane(h, w)
    is_svgf = LEVEL_TERMS[terms]["svgf"]
    c_in, v_in, rows = frame, variance, []
    for i in range(N_LEVELS):
        kw = library_kwargs(h, w, terms, i + 1, prefilter)
        if is_svgf:
            c_out, v_out = (np.asarray(a) for a in svgf(frame, variance, **kw)[:2])
        else:
            c_out, v_out = np.asarray(atrous(frame, **kw)[0]), None
        rows += [(f"{what} of level {i}", got, value, bound)
                 for what, got, value, bound in check_level(terms, prefilter, h, w, i, c_in, v_in, c_out, v_out, v_call=variance)]
        c_in, v_in = c_out, v_out
    return rows


def check_call(h, w, terms, emitted, prefilter, c_out, v_out, mutant=None):
    """A call at levels = 1 with albedo against ref_atrous_call64 / ref_svgf_call64: [(what, got, value, bound)]."""
    g, p = inputs(h, w), rule_params(terms, prefilter)
    emi = g["emitted"] if emitted else None
    if not LEVEL_TERMS[terms]["svgf"]:
        return [("colour", c_out) + ref_atrous_call64(g["frame"], guides_of(h, w), g["albedo"], emi, p, mutant)]
    (c, bc), (v, bv) = ref_svgf_call64(g["frame"], variance_plane(h, w), guides_of(h, w), g["albedo"], emi, p, mutant)
    return [("colour", c_out, c, bc), ("variance", v_out, v, bv)]


def run_call(atrous, svgf, h, w, terms, emitted, prefilter):
    kw = library_kwargs(h, w, terms, 1, prefilter, albedo=True, emitted=emitted)
    if LEVEL_TERMS[terms]["svgf"]:
        c_out, v_out = (np.asarray(a) for a in svgf(inputs(h, w)["frame"], variance_plane(h, w), **kw)[:2])
    else:
        c_out, v_out = np.asarray(atrous(inputs(h, w)["frame"], **kw)[0]), None
    return check_call(h, w, terms, emitted, prefilter, c_out, v_out)


def run_variance(estimate, h, w, terms, min_history, radius):
    moments, length = history(h, w)
    got = np.asarray(estimate(moments, length, **variance_library_kwargs(h, w, terms, min_history, radius))[0])
    return [("variance", got) + ref_variance64(moments, length, guides_of(h, w), variance_params(terms, min_history, radius))]


def run_temporal(accumulate, h, w, alpha, alpha_moments, max_history):
    """accumulate(cur, history, alpha=, alpha_moments=, max_history=) -> (history, variance, ..) over temporal_frames(h, w)."""
    frames, hist, var = temporal_frames(h, w), None, None
    for cur in frames:
        hist, var = accumulate(cur, hist, alpha=alpha, alpha_moments=alpha_moments, max_history=max_history)[:2]
    ref = ref_temporal_stats64(frames, alpha, alpha_moments, max_history)
    got = dict(color=hist["color"], moments=hist["moments"], len=hist["len"], variance=var)
    return [(k, np.asarray(got[k])) + ref[k] for k in ("color", "moments", "variance", "len")]


def assert_rows(rows, label):
    """Every entry of every row within its bound.  Returns the worst error as a share of its bound over the entries whose float64 value
    is a normal float32 (2^-126 and above) or 0: below that the float32 side may hold a flushed 0 against a bound of twice the value,
    and that share of exactly 1/2 says nothing about the arithmetic.  The assertion leaves no entry out."""
    worst = 0.0
    for what, got, value, bound in rows:
        assert holds(got, value, bound), f"{label}, {what}: {where_worst(got, value, bound)}"
        normal = (np.abs(value) >= TINY) | (value == 0)
        if normal.any():
            worst = max(worst, share(np.asarray(got)[normal], value[normal], bound[normal]))
    return worst
