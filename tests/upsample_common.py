"""What the tests of the guide-steered upsampling share (tests/test_upsample_cpu.py, tests/test_gpu_upsample.py): a numpy float32
restatement of the rule of include/rtw.h ("guided upsampling"), a float64 reference with an error bound, the case lists, the inputs, the
edge-value frames and the refusals.

restate is vectorised per tap, in tap order (ky outer, kx inner), over all output pixels; a tap that is not taken is left out through
np.where.  Every numpy operation on float32 arrays rounds once, so each pixel sees the host form's operation sequence, with the library's
own exp_plain (pinned by tests/test_guided_cpu.py).  The footprint is formed with Python's integers: N = 2 i + 1 - s, I0 = N // (2 s).
"The same" is the same bits, or NaN on both sides (tests/atrous_common.py).

ref64 is the same rule in float64 from the float32 inputs taken as exact, and beside it a bound on |float32 rule - float64 value| per
channel, in the rounding model of tests/filter_f64_common.py (u = 2^-24 per written operation, exp_plain 0.95 ulp, SAFETY 2 on the mean):
  L = (lo - e) / a      the subtraction rounds on |lo - e| <= |lo| + |e|, the divide on |L|:  e_L = (u (|lo| + |e|) / a + u |L|)(1 + u)
  t = rem / D           one rounding (none when D is a power of two);  wx = k' -+ t: u t + u |wx|; hw = wx * wy one more
  a (the exponent)      d = zq - zp: u|d|; times inv_s (itself rounded): 2u more; the square (2|x| + e) e + u x^2; inv_x = 0.5 / (s * s) two
                        roundings and the product one; the normal term's three squares and two sums likewise; each a = a + term rounds on a
  wt = hw * g           1 + dw = exp(e_a)(1 + 2 * 0.95 u)(1 + u)(1 + d_hw); dw = 1 where the float64 weight is below 2^-120 (may be flushed)
  the weighted mean     2 (sum(w dw |c - out|) / sum(w) + (n + 3) u sum(w |c|) / sum(w) + sum(w e_L) / sum(w) + n 2^-126 / sum(w))
  out = C * ah + eh     e_C |ah| + u (|C| + e_C) |ah| + u (|C ah| + e_C |ah| + |eh|)
and where the fallback is taken (no tap counts) the value is L itself with e_L."""
import ctypes as C
import functools
import itertools

import numpy as np

import rtw_amd as R
from tests.atrous_common import mismatch, same_bits  # noqa: F401  (re-exported)

F, D64 = np.float32, np.float64
U = 2.0 ** -24
EXP_ULP, SAFETY, FLUSH, TINY = 0.95, 2.0, 2.0 ** -120, 2.0 ** -126
SIZES = [(1, 1), (5, 4), (13, 7), (33, 17)]                 # (w, h) of the output
SCALES = [1, 2, 3, 4, 8]
RADII = [1, 2]
TERMS = list(itertools.product((False, True), repeat=4))    # (depth, normal, idx, albedo + emission)
SIGMA_DEPTH, SIGMA_NORMAL, FLOOR = 0.5, 0.6, 0.05
TILE_SIZES = [(32, 16), (33, 17), (31, 15), (65, 33), (64, 16)]
TILE_SCALES = [2, 3, 4]
EDGE_IDS = ["nan", "+inf", "-inf", "3e38", "denormal", "-0"]


def lo_size(w, h, s):
    return -(-w // s), -(-h // s)


def term_kw(terms):
    depth, normal, idx, _ = terms
    return dict(sigma_depth=SIGMA_DEPTH if depth else 0.0, sigma_normal=SIGMA_NORMAL if normal else 0.0, same_object=bool(idx), albedo_floor=FLOOR)


# ---- the rule in numpy float32 ---------------------------------------------------------------------------------------------------------------
def foot(n, s):
    """(I0, t) of output coordinates 0 .. n-1: Python integers and one float32 divide."""
    i = np.arange(n, dtype=np.int64)
    N, Dn = 2 * i + 1 - s, 2 * s
    I0 = N // Dn                                            # (floor division)
    return I0, (N - I0 * Dn).astype(F) / F(Dn)


def tent(k, radius, t):
    return F(radius + k) - t if k <= 0 else F(radius - k) + t


def _exp_plain(x):
    return R.exp_plain(np.ascontiguousarray(x, F).reshape(-1)).reshape(x.shape)


def _modulation(g, shape, floor):
    albedo, emitted = (g or {}).get("albedo"), (g or {}).get("emitted")
    a = np.ones(shape, F) if albedo is None else np.where(np.asarray(albedo, F) >= F(floor), np.asarray(albedo, F), F(1.0)).astype(F)
    e = np.zeros(shape, F) if emitted is None else np.asarray(emitted, F)
    return a, e


def restate(frame_lo, size, lo=None, hi=None, scale=2, radius=1, sigma_depth=0.0, sigma_normal=0.0, same_object=False, albedo_floor=FLOOR):
    """(out [h][w][3], wsum [h][w]): include/rtw.h's rule, every operation a float32 one in the written order."""
    frame_lo = np.asarray(frame_lo, F)
    h_lo, w_lo, _ = frame_lo.shape
    w, h = size
    s = int(scale)
    with np.errstate(all="ignore"):
        a_lo, e_lo = _modulation(lo, frame_lo.shape, albedo_floor)
        L = ((frame_lo - e_lo) / a_lo).astype(F)
        I0, tx = foot(w, s)
        J0, ty = foot(h, s)
        inv_s = F(1.0) / F(s)
        sum_ = np.zeros((h, w, 3), F)
        wsum = np.zeros((h, w), F)
        for ky in range(-(radius - 1), radius + 1):
            qy = J0 + ky
            vy, wy = (qy >= 0) & (qy < h_lo), tent(ky, radius, ty)
            QY = np.clip(qy, 0, h_lo - 1)[:, None]
            for kx in range(-(radius - 1), radius + 1):
                qx = I0 + kx
                vx, wx = (qx >= 0) & (qx < w_lo), tent(kx, radius, tx)
                QX = np.clip(qx, 0, w_lo - 1)[None, :]
                hw = (wx[None, :] * wy[:, None]).astype(F)
                acc = np.zeros((h, w), F)
                if sigma_depth > 0:
                    inv = F(0.5) / (F(sigma_depth) * F(sigma_depth))
                    dz = (np.asarray(lo["depth"], F)[QY, QX] - np.asarray(hi["depth"], F)) * inv_s
                    acc = acc + inv * (dz * dz)
                if sigma_normal > 0:
                    inv = F(0.5) / (F(sigma_normal) * F(sigma_normal))
                    d = np.asarray(lo["normal"], F)[QY, QX] - np.asarray(hi["normal"], F)
                    acc = acc + inv * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                g = np.where(acc >= 0, _exp_plain(-acc), F(0.0)).astype(F)
                if same_object:
                    g = np.where(np.asarray(lo["idx"])[QY, QX] != np.asarray(hi["idx"]), F(0.0), g)
                wt = (hw * g).astype(F)
                Lq = L[QY, QX]
                take = (vy[:, None] & vx[None, :]) & (wt > 0) & np.isfinite(Lq).all(-1)
                sum_ = np.where(take[..., None], sum_ + Lq * wt[..., None], sum_).astype(F)
                wsum = np.where(take, wsum + wt, wsum).astype(F)
        cover = L[(np.arange(h) // s)[:, None], (np.arange(w) // s)[None, :]]
        Cc = np.where((wsum > 0)[..., None], sum_ / wsum[..., None], cover).astype(F)
        a_hi, e_hi = _modulation(hi, (h, w, 3), albedo_floor)
        return (Cc * a_hi + e_hi).astype(F), wsum


def taps_inside(size, scale, radius):
    w, h = size
    w_lo, h_lo = lo_size(w, h, scale)

    def along(n, n_lo):
        I0, _ = foot(n, scale)
        return sum(int(((I0 + k >= 0) & (I0 + k < n_lo)).sum()) for k in range(-(radius - 1), radius + 1))
    return along(w, w_lo) * along(h, h_lo)


# ---- the rule in float64, with a bound -------------------------------------------------------------------------------------------------------
def ref64(frame_lo, size, lo=None, hi=None, scale=2, radius=1, sigma_depth=0.0, sigma_normal=0.0, same_object=False, albedo_floor=FLOOR):
    """(out, bound), both [h][w][3] float64 (module docstring).  For finite inputs."""
    frame_lo = np.asarray(frame_lo, F).astype(D64)
    h_lo, w_lo, _ = frame_lo.shape
    w, h = size
    s = int(scale)
    a_lo, e_lo = (x.astype(D64) for x in _modulation(lo, frame_lo.shape, albedo_floor))
    L = (frame_lo - e_lo) / a_lo
    eL = (U * (np.abs(frame_lo) + np.abs(e_lo)) / a_lo + U * np.abs(L)) * (1.0 + U)
    I0, _ = foot(w, s)
    J0, _ = foot(h, s)
    tx = ((2 * np.arange(w) + 1 - s) - I0 * 2 * s) / (2.0 * s)
    ty = ((2 * np.arange(h) + 1 - s) - J0 * 2 * s) / (2.0 * s)
    pow2 = s & (s - 1) == 0

    def tent64(k, t):
        wv = (radius + k) - t if k <= 0 else (radius - k) + t
        e = (0.0 if pow2 else U * t) + U * np.abs(wv)
        return wv, np.where(wv > 0, e / np.where(wv > 0, wv, 1.0), 0.0)

    f32 = lambda x: float(F(x))
    num = np.zeros((h, w, 3))
    den = np.zeros((h, w))
    e_w = np.zeros((h, w, 3))          # sum(w dw |c - out|) needs out: keep the taps and finish below
    taps = []
    for ky in range(-(radius - 1), radius + 1):
        qy = J0 + ky
        vy = (qy >= 0) & (qy < h_lo)
        wy, dwy = tent64(ky, ty)
        QY = np.clip(qy, 0, h_lo - 1)[:, None]
        for kx in range(-(radius - 1), radius + 1):
            qx = I0 + kx
            vx = (qx >= 0) & (qx < w_lo)
            wx, dwx = tent64(kx, tx)
            QX = np.clip(qx, 0, w_lo - 1)[None, :]
            hw = wx[None, :] * wy[:, None]
            dhw = (1.0 + dwx[None, :]) * (1.0 + dwy[:, None]) * (1.0 + U) - 1.0
            a = np.zeros((h, w))
            ea = np.zeros((h, w))
            if sigma_depth > 0:
                inv = 0.5 / (f32(sigma_depth) * f32(sigma_depth))
                x = (np.asarray(lo["depth"], F).astype(D64)[QY, QX] - np.asarray(hi["depth"], F).astype(D64)) / s
                ex = 3.0 * U * np.abs(x)
                term = inv * x * x
                ea = ea + inv * ((2.0 * np.abs(x) + ex) * ex + U * x * x) * (1.0 + 3.0 * U) + 3.0 * U * term
                a = a + term
                ea = ea + U * a
            if sigma_normal > 0:
                inv = 0.5 / (f32(sigma_normal) * f32(sigma_normal))
                d = np.asarray(lo["normal"], F).astype(D64)[QY, QX] - np.asarray(hi["normal"], F).astype(D64)
                ed = U * np.abs(d)
                sq = (d * d).sum(-1)
                esq = (((2.0 * np.abs(d) + ed) * ed + U * d * d).sum(-1)) * (1.0 + 2.0 * U) + 2.0 * U * sq
                term = inv * sq
                ea = ea + inv * esq * (1.0 + 3.0 * U) + 3.0 * U * term
                a = a + term
                ea = ea + U * a
            g = np.exp(-a)
            if same_object:
                g = np.where(np.asarray(lo["idx"])[QY, QX] != np.asarray(hi["idx"]), 0.0, g)
            wt = np.where(vy[:, None] & vx[None, :], hw * g, 0.0)
            dw = np.where(wt < FLUSH, 1.0, np.exp(ea) * (1.0 + 2.0 * EXP_ULP * U) * (1.0 + U) * (1.0 + dhw) - 1.0)
            taps.append((wt, dw, L[QY, QX], eL[QY, QX]))
            num = num + wt[..., None] * L[QY, QX]
            den = den + wt
    has = den > 0
    safe = np.where(has, den, 1.0)
    out = num / safe[..., None]
    n = len(taps)
    part = np.zeros((h, w, 3))
    firm = np.zeros((h, w))                                  # the weight that cannot have been flushed
    worst = np.zeros((h, w, 3))
    for wt, dw, c, ec in taps:
        part = part + wt[..., None] * (dw[..., None] * np.abs(c - out) + (n + 3) * U * np.abs(c) + ec)
        firm = firm + np.where(wt >= FLUSH, wt, 0.0)
        worst = np.maximum(worst, np.where((wt > 0)[..., None], np.abs(c - out) + ec, 0.0))
    bound = SAFETY * (part / safe[..., None] + n * TINY / safe[..., None])
    # Every tap may have been flushed (all weights below 2^-120): the float32 side took the fallback -- the covering pixel, one of the taps --
    # or a mean of the taps whose weight survived as a subnormal of at least 2^-134 (hw >= 2^-8, exp_plain never below 2^-126), each
    # product off by at most 2^-150: n 2^-15 of the largest tap beside the distance to the farthest tap.
    cmax = np.maximum.reduce([np.abs(c) + ec for _, _, c, ec in taps])
    bound = np.where((firm > 0)[..., None], bound, worst + n * 2.0 ** -15 * cmax + SAFETY * part / safe[..., None])
    cover = (np.arange(h) // s)[:, None], (np.arange(w) // s)[None, :]
    Cc = np.where(has[..., None], out, L[cover])
    eC = np.where(has[..., None], bound, eL[cover])
    a_hi, e_hi = (x.astype(D64) for x in _modulation(hi, (h, w, 3), albedo_floor))
    val = Cc * a_hi + e_hi
    err = eC * a_hi + U * (np.abs(Cc) + eC) * a_hi + U * (np.abs(Cc * a_hi) + eC * a_hi + np.abs(e_hi))
    return val, err


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def _surface(y, x):
    """Guides of a made-up view at continuous output-pixel coordinates (y, x): three objects and a miss strip, a slanted depth."""
    y, x = np.broadcast_arrays(np.asarray(y, D64), np.asarray(x, D64))
    idx = (np.floor(x / 5.0) % 3 + 3 * (np.floor(y / 4.0) % 2)).astype(np.int32)
    idx = np.where((x + 2 * y) % 11 < 1.0, -1, idx).astype(np.int32)
    depth = (1.0 + 0.02 * x + 0.03 * y + 0.4 * (idx % 3)).astype(F)
    depth = np.where(idx < 0, F(16.0), depth).astype(F)
    ang = 0.7 * idx.astype(D64) + 0.01 * x
    normal = np.stack([np.cos(ang), np.sin(ang) * 0.8, 0.6 * np.sin(ang)], -1).astype(F)
    normal[idx < 0] = 0.0
    albedo = np.stack([0.2 + 0.1 * (idx % 3) + 0.3 * ((x + y) % 2), 0.5 + 0.0 * x, np.where(idx == 1, FLOOR * 0.99, 0.9)], -1).astype(F)
    albedo[idx == 2, 1] = F(FLOOR)                          # exactly at the floor: divided by
    albedo[idx < 0] = 0.0
    emitted = np.zeros(albedo.shape, F)
    emitted[idx == 4] = (0.5, 0.25, 2.0)
    return dict(depth=depth, normal=normal, idx=idx, albedo=albedo, emitted=emitted)


@functools.lru_cache(maxsize=None)
def inputs(w, h, s, seed=0):
    """(frame_lo, guides_lo, guides_hi) of an output of w x h at scale s: the low guides are _surface at the low pixels' centres, as a
    camera_scaled view would see them; the frame is noise times the low albedo plus the low emission.  Read-only."""
    w_lo, h_lo = lo_size(w, h, s)
    rng = np.random.default_rng(9300 + 1000 * seed + 97 * h + 13 * w + s)
    jj, ii = np.mgrid[0:h, 0:w]
    JJ, II = np.mgrid[0:h_lo, 0:w_lo]
    g_hi = _surface(jj, ii)
    g_lo = _surface(JJ * s + (s - 1) / 2.0, II * s + (s - 1) / 2.0)
    fr = ((rng.random((h_lo, w_lo, 3)) * 2.0).astype(F) * np.maximum(g_lo["albedo"], F(0.1)) + g_lo["emitted"]).astype(F)
    for a in (fr, *g_lo.values(), *g_hi.values()):
        a.setflags(write=False)
    return fr, g_lo, g_hi


def guides_for(g, terms):
    """The keys of g a case passes: albedo and emitted only with the fourth term."""
    return {k: v for k, v in g.items() if terms[3] or k not in ("albedo", "emitted")}


def edge_pixels():
    """The values the rule names: NaN, both infinities, a value the demodulation overflows, denormals and -0."""
    tiny = F(1e-45)
    return [(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (3e38, 0.5, -3e38), (tiny, -tiny, F(-0.0)), (F(-0.0), F(-0.0), F(-0.0))]


@functools.lru_cache(maxsize=None)
def edge_inputs(w, h, s, places, which):
    """inputs(w, h, s) with edge_pixels()[which] at each low pixel (J, I) of `places` that lies inside the low frame.  Read-only."""
    fr, g_lo, g_hi = inputs(w, h, s)
    fr = np.array(fr)
    for J, I in places:
        if 0 <= J < fr.shape[0] and 0 <= I < fr.shape[1]:
            fr[J, I] = np.array(edge_pixels()[which], F)
    fr.setflags(write=False)
    return fr, g_lo, g_hi


def window_places(w, h, s, radius):
    """Low pixels on the first and last row and column of the window of the workgroup that starts at output pixel (32, 16), the entries
    just outside it (its halo in the neighbours' windows), and the low frame's corners."""
    w_lo, h_lo = lo_size(w, h, s)

    def ends(first, n, n_lo):
        a = int(foot(first + n, s)[0][first]) - (radius - 1)
        b = int(foot(first + n, s)[0][first + n - 1]) + radius
        return [0, 1, a - 1, a, a + 1, b - 1, b, b + 1, n_lo - 2, n_lo - 1]
    ys, xs = ends(16, 16, h_lo), ends(32, 32, w_lo)
    return tuple(sorted({(y, x) for y in ys for x in xs if 0 <= y < h_lo and 0 <= x < w_lo and (y + x) % 3 != 1}))


@functools.lru_cache(maxsize=None)
def host_upsample(w, h, s, radius, terms, edge=None):
    """The host form's (out, wsum, taps) on inputs(w, h, s) -- or edge_inputs(w, h, s, *edge) --, computed once (read-only)."""
    fr, g_lo, g_hi = inputs(w, h, s) if edge is None else edge_inputs(w, h, s, *edge)
    out, ws, st = R.upsample_filter(fr, (w, h), lo=guides_for(g_lo, terms), hi=guides_for(g_hi, terms), scale=s, radius=radius, out_wsum=True,
                                    **term_kw(terms))
    for a in (out, ws):
        a.setflags(write=False)
    return out, ws, int(st.taps)


def check_upsample(call, w, h, s, radius, terms, edge=None, wrap=None):
    """`call` (a Renderer's upsample_filter) against the host form on one case; returns its stats."""
    wrap = wrap or (lambda a: a)
    fr, g_lo, g_hi = inputs(w, h, s) if edge is None else edge_inputs(w, h, s, *edge)
    wd = lambda g: {k: wrap(v) for k, v in guides_for(g, terms).items()}
    out, ws, st = call(wrap(fr), (w, h), lo=wd(g_lo), hi=wd(g_hi), scale=s, radius=radius, out_wsum=True, **term_kw(terms))
    host = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else a
    want = host_upsample(w, h, s, radius, terms, edge)
    assert same_bits(host(out), want[0]), ((w, h), s, radius, terms, edge, "out", mismatch(host(out), want[0]))
    assert same_bits(host(ws), want[1]), ((w, h), s, radius, terms, edge, "wsum", mismatch(host(ws), want[1]))
    assert st.taps == want[2]
    return st


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------
def guides_pod(g):
    g = g or {}
    p = lambda k: g[k].ctypes.data if g.get(k) is not None else None
    return R.RtwGuides(p("depth"), p("normal"), p("idx"), p("albedo"), p("emitted"))


def check_upsample_refusals(call, head):
    """Every refusal include/rtw.h lists: RTW_E_INVALID (-1) and the outputs untouched; then a call that is accepted, so that the arguments
    the refused ones share are known to be good."""
    w, h, s = 5, 4, 2
    w_lo, h_lo = lo_size(w, h, s)
    fr, g_lo, g_hi = inputs(w, h, s)
    fr, g_lo, g_hi = np.array(fr), {k: np.array(v) for k, v in g_lo.items()}, {k: np.array(v) for k, v in g_hi.items()}
    out, ws = np.full((h, w, 3), 7.0, F), np.full((h, w), 7.0, F)
    P = lambda a: C.c_void_p(a.ctypes.data)
    nan, inf = float("nan"), float("inf")
    GL, GH = guides_pod(g_lo), guides_pod(g_hi)

    def prm(scale=s, radius=1, sd=0.5, sn=0.6, same=1, floor=FLOOR):
        return C.byref(R.RtwUpsample(scale, radius, sd, sn, same, floor))

    def without(g, *keys):
        return guides_pod({k: v for k, v in g.items() if k not in keys})

    def refused(*args):
        assert call(*head, *args, None) == -1, args
        assert (out == 7.0).all() and (ws == 7.0).all()

    fp, op, wp = P(fr), P(out), P(ws)
    gl, gh = C.byref(GL), C.byref(GH)
    refused(None, w_lo, h_lo, gl, w, h, gh, prm(), op, wp)
    refused(fp, w_lo, h_lo, gl, w, h, gh, prm(), None, wp)
    refused(fp, w_lo, h_lo, gl, w, h, gh, None, op, wp)
    refused(fp, w_lo, h_lo, gl, 0, h, gh, prm(), op, wp)
    refused(fp, w_lo, h_lo, gl, w, 0, gh, prm(), op, wp)
    refused(fp, 0, h_lo, gl, w, h, gh, prm(), op, wp)
    refused(fp, w_lo, 0, gl, w, h, gh, prm(), op, wp)
    refused(fp, 0x7FFFFC01, 1, gl, 0x7FFFFC01, 1, gh, prm(scale=1), op, wp)
    refused(fp, 1, 0x7FFFFC01, gl, 1, 0x7FFFFC01, gh, prm(scale=1), op, wp)
    refused(fp, w_lo + 1, h_lo, gl, w, h, gh, prm(), op, wp)                 # a low size that is not the ceiling
    refused(fp, w_lo, h_lo - 1, gl, w, h, gh, prm(), op, wp)
    refused(fp, w // s, h_lo, gl, w, h, gh, prm(), op, wp)                   # (the floor)
    refused(fp, w, h, gl, w, h, gh, prm(), op, wp)
    for scale in (0, R.UPSAMPLE_MAX_SCALE + 1):
        refused(fp, w_lo, h_lo, gl, w, h, gh, prm(scale=scale), op, wp)
    for radius in (0, R.UPSAMPLE_MAX_RADIUS + 1):
        refused(fp, w_lo, h_lo, gl, w, h, gh, prm(radius=radius), op, wp)
    for bad in (-0.5, nan, inf, -inf, 1e-30):                                # (1e-30: its inv_* is not finite)
        refused(fp, w_lo, h_lo, gl, w, h, gh, prm(sd=bad), op, wp)
        refused(fp, w_lo, h_lo, gl, w, h, gh, prm(sn=bad), op, wp)
    refused(fp, w_lo, h_lo, gl, w, h, gh, prm(same=2), op, wp)
    for key, kw in (("depth", dict(sn=0.0, same=0)), ("normal", dict(sd=0.0, same=0)), ("idx", dict(sd=0.0, sn=0.0))):
        refused(fp, w_lo, h_lo, C.byref(without(g_lo, key)), w, h, gh, prm(**kw), op, wp)      # a term on whose guide is missing, either side
        refused(fp, w_lo, h_lo, gl, w, h, C.byref(without(g_hi, key)), prm(**kw), op, wp)
        refused(fp, w_lo, h_lo, None, w, h, gh, prm(**kw), op, wp)
        refused(fp, w_lo, h_lo, gl, w, h, None, prm(**kw), op, wp)
    for floor in (0.0, -1.0, nan, inf):
        refused(fp, w_lo, h_lo, gl, w, h, gh, prm(floor=floor), op, wp)
        refused(fp, w_lo, h_lo, C.byref(without(g_lo, "albedo")), w, h, gh, prm(floor=floor), op, wp)   # an albedo on one side is enough
        refused(fp, w_lo, h_lo, gl, w, h, C.byref(without(g_hi, "albedo")), prm(floor=floor), op, wp)
    refused(fp, w_lo, h_lo, gl, w, h, gh, prm(), op, op)                     # the two outputs the same buffer
    # accepted: no guides at all with every term off and a floor that is then not read; no wsum_out
    assert call(*head, fp, w_lo, h_lo, None, w, h, None, prm(sd=0.0, sn=0.0, same=0, floor=nan), op, None, None) == 0
    want = R.upsample_filter(fr, (w, h), scale=s, radius=1, sigma_depth=0.0, sigma_normal=0.0, same_object=False)[0]
    assert same_bits(out, want) and (ws == 7.0).all()
    # ... and an output that is an input that is read
    big = np.full((h, w, 3), 0.5, F)
    assert call(*head, P(big), w, h, None, w, h, None, prm(scale=1, sd=0.0, sn=0.0, same=0), P(big), None, None) == -1
    assert (big == 0.5).all()
