"""What the display-stage tests share (tests/test_display_cpu.py, tests/test_gpu_display.py): the rules of include/rtw.h "display stage"
restated in numpy, and the frames they are run on.

  * restate_histogram, restate_display: float32, operation by operation -- every numpy operation on float32 arrays rounds once, as every
    written operation of csrc/rtw_display.h does under -ffp-contract=off.  pow_plain is the library's binding (tests/test_mixed_cpu.py holds
    it to its own restatement).
  * restate_exposure: float64, Python integers for the cuts.
  * ref64_display: float64 with numpy's power, from the text of rtw.h; the float32 constants of the rule (2.51f, 0.0031308f, the f32 of
    1 / 2.4, 1.0f / gamma, 255.99f) enter as the float32 values they are, since they are the rule's data and no rounding of the arithmetic.

The float64 bound (display_bound).  u = 2^-24; inputs >= 0 (a negative x is clamped to 0 on both sides, except under REINHARD where
1 + x cancels at x = -1 and the sign of a huge quotient decides between 0 and 1: the bit-exact restatement covers those).  With every term
positive a sum's relative error is its worst operand's plus u, a product's or quotient's the sum of its operands' plus u:
    x = in * exposure                                     1 u
    NONE                                                  K = 1
    REINHARD   ww 1; x / ww 3; 1 + . 4; x * . 6; 1 + x 2; the quotient 9                                       K = 9
    REINHARD_LUMA   Y: products 2, sums 3, 4; T(Y) as above from 4: Y / ww 6, 1 + . 7, Y * . 12, 1 + Y 5, quotient 18; T / Y 23; x * . 25   K = 25
    ACES_FIT   2.51 x 2; + 0.03 3; x * . 5; 2.43 x 2; + 0.59 3; x * . 5; + 0.14 6; the quotient 12               K = 12
so the clamped v in [0, 1] is off by at most K u (relative, so absolute too).  pow_plain is good to P = POW_ULP ulp = 2 P u relative
(test_pow_plain_at_the_display_exponents re-measures it at the exponents used here), and v^y carries y K u of v's error:
    GAMMA, inv_gamma y == 1        K u
    GAMMA, y < 1                   (y K + 2 P) u <= (K + 2 P) u
    SRGB, v <= knee                12.92 v <= 0.0405:  (K + 1) u * 0.0405
    SRGB, v > knee                 1.055 p: (y K + 2 P + 1) u * 1.055;  - 0.055: + u;  plus, where the two sides take different branches, the
                                   curve's own step at the knee, SRGB_STEP (computed below in float64: about 3e-9)
The bound is the largest of those for the case, times 1.01 for the second-order terms.  For bytes two more written operations follow,
v * scale and (dither) t + d, each u relative on a value of at most 256: display_bound_bytes = bound + 2 u, in units of v; times `scale` it is
the distance from a rounding threshold within which a byte may differ (by one) from the float64 byte."""
import numpy as np

import rtw_amd as R

F = np.float32
U = 2.0 ** -24
POW_ULP = 1.5                                              # pow_plain's recorded maximum is 1.05 ulp (csrc/rtw_mixed.h); margin for other exponents
SIZES = [(1, 1), (3, 1), (5, 3), (64, 48), (257, 3)]
SIZE_IDS = lambda s: f"{s[0]}x{s[1]}"
TONES = [R.TONE_NONE, R.TONE_REINHARD, R.TONE_REINHARD_LUMA, R.TONE_ACES_FIT]
TRANSFERS = [R.TRANSFER_GAMMA, R.TRANSFER_SRGB]
QUANTISES = [R.QUANTISE_RUST, R.QUANTISE_RUST2]
FORMATS = [R.DISPLAY_RGB8, R.DISPLAY_RGBA8, R.DISPLAY_F32]
KNEE = F(0.0031308)
SRGB_EXP = F(0.4166666567325592)
SRGB_STEP = abs(12.92 * float(KNEE) - (float(F(1.055)) * float(KNEE) ** float(SRGB_EXP) - float(F(0.055))))
BAYER = np.array([[0, 32, 8, 40, 2, 34, 10, 42], [48, 16, 56, 24, 50, 18, 58, 26], [12, 44, 4, 36, 14, 46, 6, 38], [60, 28, 52, 20, 62, 30, 54, 22],
                  [3, 35, 11, 43, 1, 33, 9, 41], [51, 19, 59, 27, 49, 17, 57, 25], [15, 47, 7, 39, 13, 45, 5, 37], [63, 31, 55, 23, 61, 29, 53, 21]])


def all_params():
    """Every tone x transfer x quantise x dither x format combination, as keyword arguments of display."""
    return [dict(tone=t, transfer=x, quantise=q, dither=bool(d), out_format=f)
            for t in TONES for x in TRANSFERS for q in QUANTISES for d in (0, 1) for f in FORMATS]


def same_bits(a, b):
    """The same bits, or (float32) NaN on both sides."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


# ---- frames --------------------------------------------------------------------------------------------------------------------------------
def noise(w, h, seed=0, top=4.0):
    """A linear frame over eighteen stops: 2^uniform(-14, log2 top), a few exact zeros."""
    rng = np.random.default_rng(1000 * w + h + seed)
    f = np.exp2(rng.uniform(-14.0, np.log2(top), (h, w, 3))).astype(F)
    f[rng.random((h, w)) < 0.05] = 0.0
    return f


def bin_edge_values():
    """Luminances at every bin edge and one ulp either side, 2^-16 and 2^16 among them, subnormals, +-0, negatives, NaN, +-inf, FLT_MAX."""
    edges = np.array([np.ldexp(1.0 + (i % 8) / 8.0, i // 8 - 16) for i in range(257)], F)
    v = [edges, np.nextafter(edges, F(0)), np.nextafter(edges, F(np.inf))]
    tiny = np.array([1e-45, 1e-40, 1.1754942e-38, 1.1754944e-38, 1e-30, 0.0, -0.0, -1e-45, -1.0, -3e38, np.nan, np.inf, -np.inf, 3.4028235e38,
                     3e38, 1e38, 65535.996, 70000.0, 1e9], F)
    return np.concatenate(v + [tiny])


def bin_edge_column():
    """A [n][1][3] frame: each of bin_edge_values as a grey pixel, as green alone, and with NaN, +inf and -inf in one channel of it."""
    v = bin_edge_values()
    grey = np.stack([v, v, v], -1)
    green = np.stack([np.zeros_like(v), v, np.zeros_like(v)], -1)
    odd = []
    for c in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            px = np.array(grey[: len(v) // 8])
            px[:, c] = bad
            odd.append(px)
    return np.concatenate([grey, green] + odd).reshape(-1, 1, 3).astype(F)


def special_values():
    knee = KNEE
    one = F(1.0)
    return np.array([np.nan, np.inf, -np.inf, -1.0, -0.5, -1e-30, -0.0, 0.0, 1.0, np.nextafter(one, F(0)), np.nextafter(one, F(2)),
                     knee, np.nextafter(knee, F(0)), np.nextafter(knee, F(1)), 2.0 ** -24, 2.0 ** -25, 3e-8, 6e-8, 1.2e-7, 1e-45, 1e-38,
                     0.18, 0.5, 2.0, 4.0, 1e4, 1e30, 3.4028235e38, -3.4028235e38, np.nextafter(F(-1.0), F(0)), np.nextafter(F(-1.0), F(-2))], F)


def special_frame():
    """[4][n][3]: row c < 3 holds every special value in channel c beside 0.5 and 0.25; row 3 holds it in all three channels."""
    s = special_values()
    f = np.empty((4, len(s), 3), F)
    f[:, :, 0], f[:, :, 1], f[:, :, 2] = 0.5, 0.25, 0.75
    for c in range(3):
        f[c, :, c] = s
    f[3] = s[:, None]
    return f


# ---- the float32 restatements --------------------------------------------------------------------------------------------------------------
def luma32(r, g, b):
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def restate_histogram(frame):
    """(hist uint32[256], counts uint32[2] = black, non_finite) by the rule of rtw.h."""
    with np.errstate(all="ignore"):
        f = np.ascontiguousarray(frame, F).reshape(-1, 3)
        y = luma32(f[:, 0], f[:, 1], f[:, 2])
        non_finite = ~np.isfinite(f).all(1) | (y == np.inf)
        black = ~non_finite & (y <= 0)
        counted = ~non_finite & ~black
        bins = np.clip((y[counted].view(np.uint32) >> 20).astype(np.int64) - 888, 0, 255)
        return np.bincount(bins, minlength=256).astype(np.uint32), np.array([black.sum(), non_finite.sum()], np.uint32)


def _clamp32(v, hi):
    return np.where(np.isnan(v), v, np.where(v < 0, F(0), np.where(v > hi, F(hi), v))).astype(F)


def _reinhard32(x, ww):
    return (x * (F(1) + x / ww)) / (F(1) + x)


def restate_value(frame, **params):
    """Steps 1 to 4: the F32 output."""
    d = dict(R.DISPLAY_DEFAULTS, **params)
    with np.errstate(all="ignore"):
        x = np.ascontiguousarray(frame, F) * F(d["exposure"])
        ww = F(d["white"]) * F(d["white"])
        if d["tone"] == R.TONE_REINHARD:
            v = _reinhard32(x, ww)
        elif d["tone"] == R.TONE_REINHARD_LUMA:
            y = luma32(x[..., 0], x[..., 1], x[..., 2])
            k = _reinhard32(y, ww) / y
            v = np.where((y > 0)[..., None], x * k[..., None], x)
        elif d["tone"] == R.TONE_ACES_FIT:
            v = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        else:
            v = x
        v = _clamp32(v.astype(F), 1.0)
        if d["transfer"] == R.TRANSFER_SRGB:
            v = np.where(v <= KNEE, F(12.92) * v, F(1.055) * R.pow_plain(v, SRGB_EXP) - F(0.055))
        else:
            inv = F(1.0) / F(d["gamma"])
            if inv != F(1.0):
                v = R.pow_plain(v, inv)
        return v.astype(F)


def quantise32(v, shape_hw, quantise, dither):
    """Step 5 for bytes: [h][w][3] uint8 from the float32 v."""
    h, w = shape_hw
    with np.errstate(all="ignore"):
        t = _clamp32(v * F(255.99 if quantise == R.QUANTISE_RUST2 else 255.0), 255.0)
        if dither:
            j, i = np.mgrid[0:h, 0:w]
            dd = (BAYER[j & 7, i & 7].astype(F) + F(0.5)) * F(0.015625)
            b = np.minimum(np.floor(t + dd[..., None]), F(255))
        else:
            fl = np.trunc(t)
            b = np.where(t - fl >= F(0.5), fl + F(1), fl)
        return np.where(np.isnan(t), F(0), b).astype(np.uint8)


def restate_display(frame, **params):
    d = dict(R.DISPLAY_DEFAULTS, **params)
    v = restate_value(frame, **params)
    if d["out_format"] == R.DISPLAY_F32:
        return v
    b = quantise32(v, v.shape[:2], d["quantise"], d["dither"])
    if d["out_format"] == R.DISPLAY_RGBA8:
        b = np.concatenate([b, np.full(b.shape[:2] + (1,), 255, np.uint8)], -1)
    return b


# ---- the float64 restatement of the metering ---------------------------------------------------------------------------------------------------
def restate_exposure(hist, prev_level=None, prev_exposure=1.0, **metering):
    """(level float64, exposure float32) by the rule of rtw.h."""
    m = dict(R.METERING_DEFAULTS, **metering)
    first = prev_level is None or prev_level != prev_level
    c = [int(x) for x in hist]
    total = sum(c)
    lo, hi = total * int(m["low_permille"]) // 1000, total * int(m["high_permille"]) // 1000
    n = total - lo - hi
    if n == 0:
        return (np.float64(np.nan), F(1.0)) if first else (np.float64(prev_level), F(prev_exposure))
    for i in range(256):
        k = min(c[i], lo); c[i] -= k; lo -= k
    for i in range(255, -1, -1):
        k = min(c[i], hi); c[i] -= k; hi -= k
    S = sum(c[i] * (2 * i + 1) for i in range(256))
    mean = np.float64(S) / (np.float64(2.0) * np.float64(n))
    mean = min(max(mean, np.float64(F(m["min_level"]))), np.float64(F(m["max_level"])))
    level = mean if first else np.float64(prev_level) + np.float64(F(m["rate"])) * (mean - np.float64(prev_level))
    x = level / np.float64(8.0)
    s = np.floor(x)
    y_meter = np.ldexp(np.float64(1.0) + (x - s), int(s) - 16)
    return np.float64(level), F(np.float64(F(m["key"])) / y_meter)


# ---- the float64 reference of the display transform ----------------------------------------------------------------------------------------
def _clamp64(v, hi):
    return np.where(np.isnan(v), v, np.clip(v, 0.0, hi))


def ref64_value(frame, **params):
    """Steps 1 to 4 in float64 with numpy's power."""
    d = dict(R.DISPLAY_DEFAULTS, **params)
    c = lambda k: np.float64(F(k))                         # a float32 constant of the rule
    with np.errstate(all="ignore"):
        x = np.asarray(frame, F).astype(np.float64) * c(d["exposure"])
        ww = c(d["white"]) * c(d["white"])
        rh = lambda x: (x * (1.0 + x / ww)) / (1.0 + x)
        if d["tone"] == R.TONE_REINHARD:
            v = rh(x)
        elif d["tone"] == R.TONE_REINHARD_LUMA:
            y = (c(0.2126) * x[..., 0] + c(0.7152) * x[..., 1]) + c(0.0722) * x[..., 2]
            v = np.where((y > 0)[..., None], x * (rh(y) / y)[..., None], x)
        elif d["tone"] == R.TONE_ACES_FIT:
            v = (x * (c(2.51) * x + c(0.03))) / (x * (c(2.43) * x + c(0.59)) + c(0.14))
        else:
            v = x
        v = _clamp64(v, 1.0)
        if d["transfer"] == R.TRANSFER_SRGB:
            v = np.where(v <= np.float64(KNEE), c(12.92) * v, c(1.055) * np.power(v, np.float64(SRGB_EXP)) - c(0.055))
        else:
            inv = F(1.0) / F(d["gamma"])
            if inv != F(1.0):
                v = np.power(v, np.float64(inv))
        return v


def display_bound(**params):
    """The most |F32 output - float64 reference| can be for inputs >= 0 (module docstring)."""
    d = dict(R.DISPLAY_DEFAULTS, **params)
    K = {R.TONE_NONE: 1, R.TONE_REINHARD: 9, R.TONE_REINHARD_LUMA: 25, R.TONE_ACES_FIT: 12}[d["tone"]]
    if d["transfer"] == R.TRANSFER_SRGB:
        b = max((K + 1) * U * 0.0405, 1.055 * (K + 2 * POW_ULP + 1) * U + U + SRGB_STEP)
    else:
        inv = float(F(1.0) / F(d["gamma"]))
        assert inv <= 1.0, "the bound is written for gamma >= 1"
        b = K * U if inv == 1.0 else (K + 2 * POW_ULP) * U
    return 1.01 * b


def display_bound_bytes(**params):
    return display_bound(**params) + 2 * U


def ref64_bytes_check(got, frame, **params):
    """Every byte of `got` ([h][w][3] uint8) against the float64 byte: at most 1 apart, and apart only where the float64 value lies within
    display_bound_bytes x scale of a rounding threshold.  Returns (bytes that differ, the largest distance from a threshold among them)."""
    d = dict(R.DISPLAY_DEFAULTS, **params)
    scale = float(F(255.99 if d["quantise"] == R.QUANTISE_RUST2 else 255.0))
    v = ref64_value(frame, **params)
    t = _clamp64(v * scale, 255.0)
    h, w = t.shape[:2]
    if d["dither"]:
        j, i = np.mgrid[0:h, 0:w]
        s = t + ((BAYER[j & 7, i & 7] + 0.5) / 64.0)[..., None]
        want = np.minimum(np.floor(s), 255.0)
        dist = np.abs(s - np.rint(s))                      # thresholds at the integers
    else:
        want = np.floor(t + 0.5)                           # t >= 0: half away from zero
        dist = np.abs((t - np.floor(t)) - 0.5)             # thresholds at k + 1/2
    diff = got.astype(np.int64) - want.astype(np.int64)
    assert np.abs(diff).max() <= 1, f"a byte is {np.abs(diff).max()} from the float64 byte"
    tol = display_bound_bytes(**params) * scale
    off = diff != 0
    assert (dist[off] <= tol).all(), f"a byte differs {dist[off].max()} from a threshold, allowed {tol}"
    return int(off.sum()), float(dist[off].max()) if off.any() else 0.0
