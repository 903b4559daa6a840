"""The host forms of the display stage (rtw_luminance_histogram, rtw_exposure_from_histogram, rtw_display; include/rtw.h "display stage",
DESIGN.md 8j) without a GPU: the histogram and the display transform against the numpy float32 restatements of tests/display_common.py,
exactly; the metering against the float64 restatement on the bits of level and exposure; the display transform anchored to quantize_u8,
quantize_u8_rust2 and pow_plain; a float64 reference with a bound derived from the rule's roundings (display_common's docstring); the
dither's mean and period; every refusal with the outputs untouched; the structs' sizes."""
import numpy as np
import pytest

import rtw_amd as R
from tests.display_common import (F, FORMATS, KNEE, POW_ULP, QUANTISES, SIZE_IDS, SIZES, SRGB_EXP, TONES, TRANSFERS, U, all_params, bin_edge_column,
                                  display_bound, noise, quantise32, ref64_bytes_check, ref64_value, restate_display, restate_exposure,
                                  restate_histogram, same_bits, special_frame)

C = R.C
P = lambda a: C.c_void_p(a.ctypes.data)


# ---- 1. the histogram ----------------------------------------------------------------------------------------------------------------------
def check_histogram(fn, frame):
    hist, counts, st = fn(frame)
    want_h, want_c = restate_histogram(frame)
    assert hist.dtype == np.uint32 and counts.dtype == np.uint32
    assert np.array_equal(hist, want_h), np.flatnonzero(hist != want_h)
    assert np.array_equal(counts, want_c), (counts, want_c)
    assert int(hist.sum(dtype=np.uint64)) + int(counts.sum()) == frame.shape[0] * frame.shape[1] == st.taps
    return hist, counts


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_histogram_equals_the_restatement_on_noise(size):
    hist, counts = check_histogram(R.luminance_histogram, noise(*size))
    assert size == (1, 1) or np.count_nonzero(hist) > 1 or size[0] * size[1] < 4


def test_histogram_of_a_constant_frame_is_one_bin():
    frame = np.full((48, 64, 3), 0.18, F)
    hist, counts = check_histogram(R.luminance_histogram, frame)
    assert np.count_nonzero(hist) == 1 and hist.max() == 64 * 48 and not counts.any()
    # 0.18 = 1.44 * 2^-3: stop 13 above 2^-16, mantissa 0.44 -> third eighth
    assert hist.argmax() == 8 * 13 + 3


def test_histogram_at_every_bin_edge():
    frame = bin_edge_column()
    hist, counts = check_histogram(R.luminance_histogram, frame)
    assert counts[0] > 0 and counts[1] > 0 and hist[0] > 0 and hist[255] > 0
    one = lambda v: R.luminance_histogram(np.full((1, 1, 3), v, F))
    # grey (v, v, v) has Y within an ulp or two of v: place the known ones through green alone, whose Y = 0.7152f * g
    g = lambda y: R.luminance_histogram(np.array([[[0.0, y, 0.0]]], F))
    assert g(1e-30)[0][0] == 1 and g(1e-45)[0][0] == 1              # below 2^-16, subnormal products: bin 0
    assert g(1e9)[0][255] == 1                                       # from 2^16 up: bin 255
    # FLT_MAX: the three f32 weights sum to 1 within an ulp, so whether Y overflows (non-finite) or stays FLT_MAX (bin 255) is the
    # roundings' say: the float32 restatement decides, and it is one of the two
    top = one(3.4028235e38)
    want = restate_histogram(np.full((1, 1, 3), 3.4028235e38, F))
    assert (top[0][255], top[1][1]) == (want[0][255], want[1][1]) and top[0][255] + top[1][1] == 1
    assert one(-3.4028235e38)[1].tolist() == [1, 0]                  # ... and its negative is black either way
    assert one(0.0)[1].tolist() == [1, 0] and one(-0.0)[1].tolist() == [1, 0] and one(-1.0)[1].tolist() == [1, 0]
    assert one(np.nan)[1].tolist() == [0, 1] and one(np.inf)[1].tolist() == [0, 1] and one(-np.inf)[1].tolist() == [0, 1]


# ---- 2. the metering -------------------------------------------------------------------------------------------------------------------------
def check_exposure(hist, prev_level=None, prev_exposure=1.0, **m):
    level, exposure = R.exposure_from_histogram(hist, prev_level=prev_level, prev_exposure=prev_exposure, **m)
    wl, we = restate_exposure(hist, prev_level=prev_level, prev_exposure=prev_exposure, **m)
    assert np.float64(level).tobytes() == np.float64(wl).tobytes() or (level != level and wl != wl), (level, wl, m)
    assert F(exposure).tobytes() == F(we).tobytes(), (exposure, we, m)
    return level, exposure


def hists():
    rng = np.random.default_rng(5)
    z = np.zeros(256, np.uint32)
    one, two, three = z.copy(), z.copy(), z.copy()
    one[100] = 1000
    two[40], two[200] = 7, 13
    three[0], three[128], three[255] = 333, 4000000000, 1
    return dict(empty=z, one=one, two=two, three=three, noise=rng.integers(0, 5000, 256).astype(np.uint32),
                full=np.full(256, 0xFFFFFFFF, np.uint32), frame=restate_histogram(noise(64, 48))[0])


@pytest.mark.parametrize("name", list(hists()))
def test_exposure_equals_the_restatement(name):
    h = hists()[name]
    for low, high in ((0, 0), (50, 50), (100, 20), (500, 499), (999, 0), (0, 999), (333, 333), (1, 1)):
        for rate in (0.0, 0.5, 1.0):
            for prev in (None, float("nan"), 0.0, 37.25, 131.0625, 256.0):
                check_exposure(h, prev_level=prev, prev_exposure=0.7, low_permille=low, high_permille=high, rate=rate)
    check_exposure(h, key=0.5, min_level=100.0, max_level=120.5)
    check_exposure(h, key=1e-3, min_level=0.0, max_level=0.0)
    check_exposure(h, key=1e3, min_level=256.0, max_level=256.0)


def test_exposure_cuts_split_a_bin():
    h = np.zeros(256, np.uint32)
    h[10], h[20] = 10, 10
    # 25 % off the bottom: 5 of bin 10's pixels stay; S = 5 * 21 + 10 * 41 = 515, n = 15
    level, _ = check_exposure(h, low_permille=250, high_permille=0)
    assert level == 515.0 / 30.0
    level, _ = check_exposure(h, low_permille=250, high_permille=250)       # ... and 5 of bin 20's: S = 105 + 205 = 310, n = 10
    assert level == 15.5
    level, _ = check_exposure(h, low_permille=500, high_permille=499)       # n = 20 - 10 - 9 = 1, a pixel of bin 20
    assert level == 20.5


def test_exposure_of_nothing_counted():
    z = np.zeros(256, np.uint32)
    assert check_exposure(z, prev_level=12.0, prev_exposure=0.25) == (12.0, 0.25)
    level, exposure = check_exposure(z)
    assert level != level and exposure == 1.0


@pytest.mark.parametrize("key", [0.18, 1.0])
def test_a_constant_frame_meters_to_its_bins_centre(key):
    """A frame of luminance L at bin i's lower edge, (1 + (i % 8) / 8) * 2^(i // 8 - 16): every pixel is in bin i, the level is i + 1/2, and
    the inverse rule gives L' = (1 + ((i % 8) + 1/2) / 8) * 2^(i // 8 - 16), the bin's centre: the exposure is (float)(key / L'), exact in
    float64 but for the one division.  Y = 0.7152f * g rounds, so g is the first float whose Y is not below the edge."""
    for i in range(256):
        edge = F(np.ldexp(1.0 + (i % 8) / 8.0, i // 8 - 16))
        g = F(edge / F(0.7152))
        while F(F(0.7152) * g) < edge:
            g = np.nextafter(g, F(np.inf))
        while F(F(0.7152) * np.nextafter(g, F(0))) >= edge:
            g = np.nextafter(g, F(0))
        frame = np.zeros((3, 5, 3), F)
        frame[..., 1] = g
        hist, counts, _ = R.luminance_histogram(frame)
        assert hist[i] == 15 and hist.sum() == 15, (i, np.flatnonzero(hist))
        level, exposure = R.exposure_from_histogram(hist, key=key, low_permille=0, high_permille=0)
        centre = np.ldexp(1.0 + ((i % 8) + 0.5) / 8.0, i // 8 - 16)
        assert level == i + 0.5 and F(exposure).tobytes() == F(np.float64(F(key)) / centre).tobytes(), i


# ---- 3. the display transform, anchored to what exists -------------------------------------------------------------------------------------------
PLAIN = dict(exposure=1.0, tone=R.TONE_NONE, transfer=R.TRANSFER_GAMMA, gamma=1.0, dither=False, out_format=R.DISPLAY_RGB8)


def anchor_frames():
    rng = np.random.default_rng(11)
    yield rng.uniform(-0.25, 1.25, (48, 64, 3)).astype(F)
    yield (np.arange(0, 256 * 8 * 3, dtype=np.float64).reshape(8, 256, 3) / (256 * 8 * 3 - 1)).astype(F)     # a ramp through every byte
    yield ((np.arange(0, 255 * 3).reshape(1, 255, 3) % 255 + 0.5) / 255.0).astype(F)                          # every k + 1/2 of RUST
    yield ((np.arange(0, 255 * 3).reshape(1, 255, 3) % 255 + 0.5) / 255.99).astype(F)                         # ... and of RUST2, to an ulp
    yield special_frame()


def test_plain_display_is_quantize_u8():
    for frame in anchor_frames():
        assert np.array_equal(R.display(frame, quantise=R.QUANTISE_RUST, **PLAIN)[0], R.quantize_u8(frame))
        assert np.array_equal(R.display(frame, quantise=R.QUANTISE_RUST2, **PLAIN)[0], R.quantize_u8_rust2(frame))


@pytest.mark.parametrize("gamma", [2.0, 2.2, 0.5])
def test_gamma_display_is_quantize_u8_of_pow_plain(gamma):
    for frame in anchor_frames():
        with np.errstate(all="ignore"):
            clamped = np.where(np.isnan(frame), frame, np.clip(frame, F(0), F(1))).astype(F)
        want = R.quantize_u8(R.pow_plain(clamped, F(1.0) / F(gamma)))
        assert np.array_equal(R.display(frame, quantise=R.QUANTISE_RUST, **dict(PLAIN, gamma=gamma))[0], want)


def test_rgba8_is_rgb8_plus_255_and_f32_then_the_quantise_rule_gives_the_bytes():
    frame = noise(64, 48)
    for prm in all_params():
        if prm["out_format"] != R.DISPLAY_RGB8:
            continue
        rgb = R.display(frame, **prm)[0]
        rgba = R.display(frame, **dict(prm, out_format=R.DISPLAY_RGBA8))[0]
        f32 = R.display(frame, **dict(prm, out_format=R.DISPLAY_F32))[0]
        assert rgb.shape == (48, 64, 3) and rgba.shape == (48, 64, 4) and f32.dtype == F
        assert np.array_equal(rgba[..., :3], rgb) and (rgba[..., 3] == 255).all()
        if not prm["dither"]:
            q = R.quantize_u8 if prm["quantise"] == R.QUANTISE_RUST else R.quantize_u8_rust2
            assert np.array_equal(q(f32), rgb), prm
        assert np.array_equal(quantise32(f32, (48, 64), prm["quantise"], prm["dither"]), rgb), prm


# ---- 4. the display transform against the float32 restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_display_equals_the_restatement(size):
    frame = noise(*size)
    frame[0, 0, 0] = -0.5
    for prm in all_params():
        for extra in (dict(exposure=1.0, white=4.0, gamma=2.2), dict(exposure=0.37, white=1.5, gamma=1.0)):
            got, st = R.display(frame, **prm, **extra)
            assert same_bits(got, restate_display(frame, **prm, **extra)), (size, prm, extra)
            assert st.taps == size[0] * size[1]


def test_display_of_special_values():
    frame = special_frame()
    for prm in all_params():
        for exposure in (1.0, 0.0, 3.0):
            got = R.display(frame, exposure=exposure, **prm)[0]
            assert same_bits(got, restate_display(frame, exposure=exposure, **prm)), (prm, exposure)
    nan = np.full((1, 1, 3), np.nan, F)
    for prm in all_params():                                                                   # a NaN ends as byte 0, under every curve
        if prm["out_format"] == R.DISPLAY_RGB8:
            assert not R.display(nan, **prm)[0].any(), prm


@pytest.mark.parametrize("white", [1e-30, 1e-19, 1e-3, 1e19, 1e30])
def test_display_with_white_tiny_and_huge(white):
    frames = [special_frame(), noise(64, 48)]
    for tone in (R.TONE_REINHARD, R.TONE_REINHARD_LUMA):
        for fmt in (R.DISPLAY_RGB8, R.DISPLAY_F32):
            for frame in frames:
                prm = dict(tone=tone, white=white, out_format=fmt)
                assert same_bits(R.display(frame, **prm)[0], restate_display(frame, **prm)), prm


# ---- 5. the display transform against float64 ------------------------------------------------------------------------------------------------------
def ulps(got, want):
    """|got - want| in ulps of want's float32 binade."""
    e = np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -126)))
    return np.abs(got.astype(np.float64) - want) / np.exp2(e - 23)


def test_pow_plain_at_the_display_exponents():
    """POW_ULP, the P of display_common's bound, re-measured where the display transform calls pow_plain: v in (0, 1], exponents 1 / 2.4 and
    1 / 2.2 as float32."""
    rng = np.random.default_rng(3)
    v = np.concatenate([np.linspace(0.0, 1.0, 2 ** 20 + 1)[1:], np.exp2(rng.uniform(-20, 0, 2 ** 19))]).astype(F)
    for y in (SRGB_EXP, F(1.0) / F(2.2), F(0.5)):
        e = ulps(R.pow_plain(v, y), np.power(v.astype(np.float64), np.float64(y)))
        print(f"pow_plain(v, {float(y)!r}): max {e.max():.4f} ulp at v = {float(v[e.argmax()])!r} (the bound takes {POW_ULP})")
        assert e.max() <= POW_ULP


def f64_cases():
    return [dict(tone=t, transfer=x, gamma=g) for t in TONES for x, g in ((R.TRANSFER_GAMMA, 1.0), (R.TRANSFER_GAMMA, 2.2), (R.TRANSFER_SRGB, 2.2))]


def observed_f64_errors(frames=None):
    """{case: (largest |F32 output - float64 reference|, its bound)} over the noise frames; scripts/measure_display.py logs it."""
    frames = frames or [noise(w, h, top=16.0) for w, h in SIZES]
    out = {}
    for prm in f64_cases():
        worst = 0.0
        for frame in frames:
            got = R.display(frame, out_format=R.DISPLAY_F32, **prm)[0]
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref64_value(frame, **prm)).max()))
        out[(prm["tone"], prm["transfer"], prm["gamma"])] = (worst, display_bound(**prm))
    return out


def test_f32_output_is_within_the_bound_of_float64():
    """Bound (display_common's docstring, u = 2^-24, P = 1.5 ulp): gamma 1: K u; gamma 2.2: (K + 2 P) u; sRGB: 1.055 (K + 2 P + 1) u + u + the
    knee's step; K = 1 / 9 / 25 / 12 for NONE / REINHARD / REINHARD_LUMA / ACES_FIT; all times 1.01.  That is 6.0e-8 (NONE, gamma 1) to
    1.9e-6 (REINHARD_LUMA, sRGB).  Inputs >= 0."""
    for case, (worst, bound) in observed_f64_errors().items():
        print(f"tone {case[0]} transfer {case[1]} gamma {case[2]}: max |f32 - f64| {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound, case


def test_bytes_are_within_one_of_float64_and_only_at_a_threshold():
    """Per pixel: a byte is at most 1 from the float64 byte, and differs only where the float64 value times scale lies within
    (display_bound + 2 u) x scale of a rounding threshold (k + 1/2 without dither, an integer less the dither offset with it)."""
    frames = [noise(w, h, top=16.0) for w, h in SIZES] + [(np.arange(0, 4096 * 3).reshape(16, 256, 3) / (4096 * 3 - 1.0)).astype(F)]
    total = 0
    for prm in f64_cases():
        for q in QUANTISES:
            for dither in (False, True):
                kw = dict(prm, quantise=q, dither=dither)
                n_off = 0
                for frame in frames:
                    got = R.display(frame, out_format=R.DISPLAY_RGB8, **kw)[0]
                    n_off += ref64_bytes_check(got, frame, **kw)[0]
                total += n_off
    print(f"{total} bytes off by one over every case, each at a threshold")


# ---- 6. the dither ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantise", QUANTISES)
def test_dither_keeps_the_mean_and_has_period_8(quantise):
    scale = 255.99 if quantise == R.QUANTISE_RUST2 else 255.0
    prm = dict(PLAIN, dither=True, quantise=quantise)
    for v in (0.0, 0.001, 0.1, 0.18, 0.5, 0.7071, 0.9, 0.998, 1.0, 100.25 / 255.0, 100.5 / 255.0, 100.75 / 255.0):
        out = R.display(np.full((24, 40, 3), v, F), **prm)[0]
        t = min(float(F(F(v) * F(scale))), 255.0)
        for j in range(0, 24, 8):
            for i in range(0, 40, 8):
                mean = out[j:j + 8, i:i + 8, 0].astype(np.float64).mean()
                assert abs(mean - t) <= 1.0 / 64.0, (v, i, j, mean, t)
        assert np.array_equal(out[8:], out[:-8]) and np.array_equal(out[:, 8:], out[:, :-8])
        assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
    out = R.display(np.full((8, 8, 3), 100.5 / 255.0, F), **dict(prm, quantise=R.QUANTISE_RUST))[0]
    assert (out == 100).sum() == (out == 101).sum()                            # (half of the pattern rounds up)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def check_histogram_refusals(fn, head):
    frame = noise(5, 3)
    hist, counts = np.full(256, 7, np.uint32), np.full(2, 7, np.uint32)
    bad = [(None, 5, 3, P(hist), P(counts)), (P(frame), 5, 3, None, P(counts)), (P(frame), 5, 3, P(hist), None),
           (P(frame), 0, 3, P(hist), P(counts)), (P(frame), 5, 0, P(hist), P(counts)),
           (P(frame), 0x7FFFFC01, 1, P(hist), P(counts)), (P(frame), 1, 0x7FFFFC01, P(hist), P(counts)),
           (P(frame), 0x10000, 0x10000, P(hist), P(counts))]
    for args in bad:
        assert fn(*head, *args, None) == -1, args
        assert (hist == 7).all() and (counts == 7).all()
    big = np.zeros((20, 20, 3), F)                                             # 4800 bytes: room for a histogram inside the frame
    inside = C.c_void_p(big.ctypes.data + 64)
    before = big.copy()
    assert fn(*head, P(big), 20, 20, inside, P(counts), None) == -1
    assert fn(*head, P(big), 20, 20, P(hist), inside, None) == -1
    both = np.full(258, 7, np.uint32)
    assert fn(*head, P(frame), 5, 3, P(both), C.c_void_p(both.ctypes.data + 1020), None) == -1          # counts inside hist
    assert np.array_equal(big, before) and (both == 7).all() and (counts == 7).all()


def display_refusal_cases():
    ok = dict(R.DISPLAY_DEFAULTS)
    bad = [dict(exposure=-1.0), dict(exposure=float("nan")), dict(exposure=float("inf")), dict(gamma=0.0), dict(gamma=-2.0),
           dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=1e-40), dict(tone=4), dict(transfer=2), dict(quantise=2),
           dict(out_format=3), dict(dither=2)]
    for tone in (R.TONE_REINHARD, R.TONE_REINHARD_LUMA):
        bad += [dict(tone=tone, white=w) for w in (0.0, -1.0, float("nan"), float("inf"))]
    return ok, bad


def check_display_refusals(fn, head):
    frame = noise(5, 3)
    out = np.full((3, 5, 4), 7, np.uint32)                                     # room for every format
    ok, bad = display_refusal_cases()
    struct = lambda d: R.RtwDisplay(d["exposure"], d["tone"], d["white"], d["transfer"], d["gamma"], d["quantise"], int(d["dither"]), d["out_format"])
    good = struct(ok)
    for args in [(None, 5, 3, C.byref(good), P(out)), (P(frame), 5, 3, None, P(out)), (P(frame), 5, 3, C.byref(good), None),
                 (P(frame), 0, 3, C.byref(good), P(out)), (P(frame), 5, 0, C.byref(good), P(out)),
                 (P(frame), 0x7FFFFC01, 1, C.byref(good), P(out)), (P(frame), 0x10000, 0x10000, C.byref(good), P(out))]:
        assert fn(*head, *args, None) == -1, args
    for d in bad:
        prm = struct(dict(ok, **d))
        assert fn(*head, P(frame), 5, 3, C.byref(prm), P(out), None) == -1, d
    assert (out == 7).all()
    for tone in (R.TONE_NONE, R.TONE_ACES_FIT):                                # white is not read there: anything goes
        assert fn(*head, P(frame), 5, 3, C.byref(struct(dict(ok, tone=tone, white=float("nan")))), P(out), None) == 0
    # out overlapping in, for every format: in place, one byte into the frame, the frame's last byte
    for fmt in FORMATS:
        prm = struct(dict(ok, out_format=fmt))
        buf = np.full(5 * 3 * 3 + 64, 0.5, F)
        before = buf.copy()
        for off in (0, 1, 5 * 3 * 3 * 4 - 1):
            assert fn(*head, P(buf), 5, 3, C.byref(prm), C.c_void_p(buf.ctypes.data + off), None) == -1, (fmt, off)
        n_out = 5 * 3 * (12 if fmt == R.DISPLAY_F32 else 4 if fmt == R.DISPLAY_RGBA8 else 3)
        # a frame that starts in the output's last word
        assert fn(*head, C.c_void_p(buf.ctypes.data + n_out - 1 - (n_out - 1) % 4), 5, 3, C.byref(prm), P(buf), None) == -1, fmt
        assert np.array_equal(buf, before)
        # ... and the first byte behind the frame is no overlap
        assert fn(*head, P(buf), 5, 3, C.byref(prm), C.c_void_p(buf.ctypes.data + 5 * 3 * 3 * 4), None) == 0, fmt


def test_histogram_refusals():
    check_histogram_refusals(R.lib().rtw_luminance_histogram, ())


def test_display_refusals():
    check_display_refusals(R.lib().rtw_display, ())


def test_exposure_refusals():
    h = np.full(256, 3, np.uint32)
    level, exposure = C.c_double(7.0), C.c_float(7.0)
    fn = R.lib().rtw_exposure_from_histogram
    ok = dict(R.METERING_DEFAULTS)
    struct = lambda d: R.RtwMetering(d["low_permille"], d["high_permille"], d["key"], d["rate"], d["min_level"], d["max_level"])
    nan = float("nan")
    good = struct(ok)
    assert fn(None, C.byref(good), nan, 1.0, C.byref(level), C.byref(exposure)) == -1
    assert fn(P(h), None, nan, 1.0, C.byref(level), C.byref(exposure)) == -1
    assert fn(P(h), C.byref(good), nan, 1.0, None, C.byref(exposure)) == -1
    assert fn(P(h), C.byref(good), nan, 1.0, C.byref(level), None) == -1
    for d in (dict(low_permille=500, high_permille=500), dict(low_permille=1000, high_permille=0), dict(low_permille=0xFFFFFFFF, high_permille=2),
              dict(key=0.0), dict(key=-1.0), dict(key=nan), dict(key=float("inf")), dict(rate=-0.1), dict(rate=1.5), dict(rate=nan),
              dict(min_level=-1.0), dict(max_level=257.0), dict(min_level=nan), dict(max_level=nan), dict(min_level=10.0, max_level=9.0)):
        assert fn(P(h), C.byref(struct(dict(ok, **d))), nan, 1.0, C.byref(level), C.byref(exposure)) == -1, d
    for prev in (-1.0, 256.5, float("inf"), -float("inf")):
        assert fn(P(h), C.byref(good), prev, 1.0, C.byref(level), C.byref(exposure)) == -1, prev
    assert level.value == 7.0 and exposure.value == 7.0
    assert fn(P(h), C.byref(good), nan, 1.0, C.byref(level), C.byref(exposure)) == 0 and level.value == 128.0
    with pytest.raises(TypeError):
        R.exposure_from_histogram(h, nonsense=1)
    with pytest.raises(TypeError):
        R.display(noise(3, 1), nonsense=1)


# ---- 8. the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi():
    assert C.sizeof(R.RtwMetering) == 24 and C.sizeof(R.RtwDisplay) == 32
    assert R.lib().rtw_abi_version() == 4
    assert set(R.DISPLAY_DEFAULTS) == {"exposure", "tone", "white", "transfer", "gamma", "quantise", "dither", "out_format"}
    for name in ("rtw_luminance_histogram", "rtw_ctx_luminance_histogram", "rtw_exposure_from_histogram", "rtw_display", "rtw_ctx_display"):
        assert hasattr(R.lib(), name)
