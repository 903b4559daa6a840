"""The host form of bloom (rtw_bloom, rtw_bloom_levels; csrc/rtw_bloom.cpp) against the rule of include/rtw.h restated in numpy
(tests/bloom_common.py): bit for bit in float32 over the sizes at which a level is one pixel, odd, or one pixel past a 16-pixel tile, every
`levels`, the Karis weight on and off, the knee's cases, with and without the layer and in place; the two weight tables re-derived in float64
from the bilinear taps they multiply out; known answers; the float64 rule within a derived bound; the refusals; the ABI."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.bloom_common import (D, F, PARAM_SETS, SIZE_IDS, SIZES, UP, bloom_bound, foot, knee_curve, levels_restated, luma, noise,
                                restate_bloom, same_bits, special_frame)

P = lambda a: C.c_void_p(a.ctypes.data)


def check_against_restatement(frame, **prm):
    want_out, want_layer, taps, _ = restate_bloom(frame, **prm)
    out, layer, st = R.bloom(frame, layer=True, **prm)
    assert same_bits(out, want_out), (prm, np.argwhere(out != want_out)[:4])
    assert same_bits(layer, want_layer), (prm, np.argwhere(layer != want_layer)[:4])
    assert st.taps == taps and st.filter_ms == st.total_ms and st.avg_gradient == st.spatial == st.gradient_ms == st.table_ms == 0.0
    out2, none, _ = R.bloom(frame, **prm)                                      # without the layer
    assert none is None and same_bits(out2, want_out)
    buf = frame.copy()                                                         # out is in
    out3, layer3, _ = R.bloom(buf, out=buf, layer=True, **prm)
    assert out3 is buf and same_bits(buf, want_out) and same_bits(layer3, want_layer)
    return out, layer


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_host_form_equals_restatement(size):
    frame = noise(*size)
    for k, ps in enumerate(PARAM_SETS):
        check_against_restatement(frame, levels=(1, 2, 8, 6)[k % 4], spread=0.5, intensity=0.25, **ps)
    check_against_restatement(frame, levels=8, spread=1.25, intensity=2.0, threshold=0.25, knee=0.125, karis=True)


@pytest.mark.parametrize("levels", range(1, 9))
def test_every_levels_at_33(levels):
    frame = noise(33, 33, seed=levels)
    sizes = R.bloom_levels(33, 33, levels)
    assert sizes == [(17, 17), (9, 9), (5, 5), (3, 3), (2, 2), (1, 1)][:levels]   # the chain stops at 1 x 1
    for karis in (False, True):
        check_against_restatement(frame, levels=levels, karis=karis, threshold=0.5, knee=0.25, spread=0.75, intensity=0.5)


def test_special_values_follow_the_restatement():
    frame = special_frame()
    for ps in PARAM_SETS:
        out, layer = check_against_restatement(frame, levels=3, spread=0.5, intensity=0.25, **ps)
        assert np.isfinite(layer).all()                                         # a NaN or an infinity never spreads
        assert np.array_equal(np.isfinite(out), np.isfinite(frame))             # ... and `out` is not finite exactly where `in` was not
    big = np.full((5, 7, 3), 3e38, F)                                           # sums that round to infinity: what the float32 rule says
    big[2, 3] = 1.0
    check_against_restatement(big, levels=2, threshold=1.0, knee=0.5, karis=False, spread=0.5, intensity=0.25)
    check_against_restatement(big, levels=2, threshold=1.0, knee=0.5, karis=True, spread=0.5, intensity=0.25)


# ---- 2. the tables ---------------------------------------------------------------------------------------------------------------------------
def bilinear(img, x, y):
    """A bilinear fetch of img (float64, zero outside) at continuous (x, y), pixel k's centre at k + 0.5."""
    fx, fy = x - 0.5, y - 0.5
    x0, y0 = int(np.floor(fx)), int(np.floor(fy))
    tx, ty = fx - x0, fy - y0
    at = lambda i, j: img[j, i] if 0 <= i < img.shape[1] and 0 <= j < img.shape[0] else 0.0
    return (at(x0, y0) * (1 - tx) + at(x0 + 1, y0) * tx) * (1 - ty) + (at(x0, y0 + 1) * (1 - tx) + at(x0 + 1, y0 + 1) * tx) * ty


def test_down_table_is_the_13_bilinear_taps():
    """The rule's table D (tests/bloom_common.py's copy of include/rtw.h) against the 13 taps in float64.  This pins the rule's text, not the
    table in csrc/rtw_bloom.h: that one is held to D only through the bit-for-bit restatement tests above, which run every weight."""
    assert D.sum() == 128 and np.array_equal(D, D.T) and np.array_equal(D, D[::-1])
    # Jimenez 2014: a centre box of four taps at (+-1, +-1) weighing 1/2, four corner boxes of the nine taps at {-2, 0, 2}^2 weighing 1/8 each
    taps = [((sx, sy), 0.5 / 4) for sx in (-1, 1) for sy in (-1, 1)]
    for bx in (-1, 1):
        for by in (-1, 1):
            taps += [((bx + sx, by + sy), 0.125 / 4) for sx in (-1, 1) for sy in (-1, 1)]
    assert len(taps) == 20 and len({t for t, _ in taps}) == 13
    got = np.zeros((6, 6))
    cx = cy = 3.0                                                               # the corner between pixels 2 and 3: a = 0 is pixel 2
    for b in range(6):
        for a in range(6):
            img = np.zeros((6, 6))
            img[b, a] = 1.0
            got[b, a] = sum(wt * bilinear(img, cx + ox, cy + oy) for (ox, oy), wt in taps)
    assert np.array_equal(got, D / 128.0)


def test_up_rows_are_tent_then_bilinear():
    """The rule's two up rows and its integer footprint (bloom_common.foot, UP) against tent-then-bilinear in float64.  As above this pins the
    rule's text; csrc/rtw_bloom.h's bloom_up_foot is held to it through the restatement tests."""
    n = 37
    first, weights = foot(n)
    tent = np.array([0.25, 0.5, 0.25])
    for i in range(n):
        pos = (i + 0.5) / 2.0 - 0.5                                             # the fine pixel's centre in coarse pixel indices
        i0 = int(np.floor(pos))
        f = pos - i0
        row = np.zeros(4)
        row[0:3] += (1 - f) * tent                                              # the tent about i0 ...
        row[1:4] += f * tent                                                    # ... and about i0 + 1
        assert first[i] == i0 - 1 and np.array_equal(row * 16.0, weights[i]), i
        assert tuple(weights[i]) == UP[(2 * i - 1) % 4]
    assert first[0] == -2 and tuple(weights[0]) == UP[3]


# ---- 3. known answers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (33, 33), (64, 48)], ids=SIZE_IDS)
def test_constant_frame(size):
    w, h = size
    frame = np.full((h, w, 3), 0.75, F)
    for levels in range(1, 9):
        n = len(R.bloom_levels(w, h, levels))
        out, layer, _ = R.bloom(frame, layer=True, levels=levels, threshold=0.0, knee=0.0, karis=False, spread=0.5, intensity=0.25)
        want = F(0.75 * (2.0 - 2.0 ** (1 - n)))                                # every level is 0.75; all weights are dyadic
        assert (layer == want).all(), (levels, n)
        assert (out == F(0.75) + F(0.25) * want).all()
        assert all((lv == F(0.75)).all() for lv in restate_bloom(frame, levels=levels, threshold=0.0, knee=0.0, karis=False, spread=0.0)[3])


def test_below_the_threshold_and_zero_intensity():
    frame = noise(65, 35, top=0.4)
    assert frame.max() < 0.5
    out, layer, _ = R.bloom(frame, layer=True, threshold=1.0, knee=0.5, intensity=7.0)
    assert not layer.any() and same_bits(out, frame)                            # wholly below threshold - knee
    frame = special_frame()
    frame[0, 0] = (-0.0, 0.0, -0.0)
    out, layer, _ = R.bloom(frame, layer=True, threshold=0.0, knee=0.0, intensity=0.0)
    assert layer.any()
    assert np.array_equal(np.isnan(out), np.isnan(frame))
    keep = ~np.isnan(frame)
    assert np.array_equal(out[keep], frame[keep]) and (out[0, 0] == 0.0).all()  # -0.0 + 0 * B is 0.0: its value


def test_nan_frame():
    frame = np.full((7, 33, 3), np.nan, F)
    out, layer, _ = R.bloom(frame, layer=True)
    assert not layer.any() and np.isnan(out).all()


def test_firefly():
    frame = np.zeros((64, 64, 3), F)
    frame[31, 30] = 1e4
    prm = dict(threshold=1.0, knee=0.5, spread=0.5, intensity=1.0)
    support = []
    for levels in (1, 2, 3, 4):
        plain = R.bloom(frame, layer=True, levels=levels, karis=False, **prm)[1]
        karis = R.bloom(frame, layer=True, levels=levels, karis=True, **prm)[1]
        assert 0.0 < karis.max() < plain.max()                                  # the weight keeps the firefly down
        for layer in (plain, karis):
            # level 1's pixels (14 .. 16, 14 .. 16) hold it (2I + a = 30: I = 14, 15, 16); their up footprint on the frame and beyond it
            assert (layer[28:34, 27:33] > 0).all()
            if levels > 1:
                assert (layer[31, 20] > 0).all() and (layer[20, 30] > 0).all()
        support.append(int((plain > 0).all(-1).sum()))
    assert support[0] < support[1] < support[2] <= support[3] == 64 * 64        # the support grows with the levels, to the whole frame


def test_knee():
    """Continuity and monotony are asserted of the restatement's knee_curve (c is not an output of the library); the host form is tied to
    it at every point of the sweep, the joints and an ulp either side among them, on 1 x 1 frames, bit for bit against the restatement."""
    threshold, knee = F(1.0), F(0.25)
    lo, hi = threshold - knee, threshold + knee
    edge = []
    for v in (lo, hi):
        edge += [np.nextafter(v, F(0)), v, np.nextafter(v, F(4))]
    sweep = np.concatenate([np.array(edge, F), np.linspace(0.5, 1.5, 401).astype(F)])
    sweep.sort()
    c = knee_curve(sweep, threshold, knee, F)
    assert c.dtype == F and (np.diff(c) >= 0).all()                             # monotone, through both joints
    assert knee_curve(np.array([lo], F), threshold, knee, F)[0] == 0.0 and knee_curve(np.array([hi], F), threshold, knee, F)[0] == knee
    # the host form at those luminances, a 1 x 1 frame each (no neighbour mixes in), against the restatement
    for v in sweep.tolist():
        grey = np.full((1, 1, 3), v, F)
        prm = dict(levels=1, threshold=float(threshold), knee=float(knee), karis=False, spread=0.5, intensity=1.0)
        layer = R.bloom(grey, layer=True, **prm)[1]
        assert same_bits(layer, restate_bloom(grey, **prm)[1]), v
        assert (layer > 0).all() == (luma(grey, F)[0, 0] > lo)


# ---- 4. float64 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(5, 3), (33, 33), (65, 35), (64, 48)], ids=SIZE_IDS)
def test_host_form_against_float64(size):
    frame = noise(*size)
    assert frame.max() <= 256.0
    worst = 0.0
    for ps in PARAM_SETS:
        prm = dict(levels=8, spread=0.5, intensity=0.25, **ps)
        out, layer, _ = R.bloom(frame, layer=True, **prm)
        out64, layer64, bound_out, bound_layer = bloom_bound(frame, **prm)
        err_out, err_layer = np.abs(out - out64), np.abs(layer - layer64)
        with np.errstate(all="ignore"):
            ratio = max(np.nanmax(np.where(bound_out > 0, err_out / bound_out, 0.0)), np.nanmax(np.where(bound_layer > 0, err_layer / bound_layer, 0.0)))
        worst = max(worst, float(ratio))
        print(f"\n[bloom f64] {size[0]}x{size[1]} {ps}: max |out - f64| {err_out.max():.3e} (bound there {bound_out.flat[err_out.argmax()]:.3e}), "
              f"layer {err_layer.max():.3e} (bound {bound_layer.flat[err_layer.argmax()]:.3e}), largest error / bound {ratio:.3f}")
        assert (err_out <= bound_out).all() and (err_layer <= bound_layer).all()
    assert worst > 0.0                                                          # (the comparison saw something)


# ---- 5. levels, refusals, the ABI ------------------------------------------------------------------------------------------------------------
def test_bloom_levels():
    for other in (1, 2, 7, 300):
        for side in range(1, 301):
            for w, h in ((side, other), (other, side)):
                for levels in (1, 3, 8):
                    assert R.bloom_levels(w, h, levels) == levels_restated(w, h, levels), (w, h, levels)
    assert R.lib().rtw_bloom_levels(33, 33, 8, None) == 6                       # sizes may be NULL
    assert R.lib().rtw_bloom_levels(0x7FFFFC00, 1, 8, None) == 8
    for bad in ((0, 3, 1), (3, 0, 1), (3, 3, 0), (3, 3, 9)):
        assert R.lib().rtw_bloom_levels(*bad, None) == 0
        with pytest.raises(ValueError):
            R.bloom_levels(*bad)


def bloom_refusal_cases():
    nan, inf = float("nan"), float("inf")
    bad = [dict(levels=0), dict(levels=9), dict(knee=0.75, threshold=0.5), dict(karis=2)]
    for key in ("threshold", "knee", "spread", "intensity"):
        bad += [{key: v} for v in (-1.0, nan, inf, -inf)]
    return bad


def check_bloom_refusals(fn, head):
    """Every refusal of rtw_bloom / rtw_ctx_bloom: RTW_E_INVALID and the sentinels in out and layer_out untouched."""
    frame = noise(5, 3)
    out, layer = np.full((3, 5, 3), 7.0, F), np.full((3, 5, 3), 7.0, F)
    ok = dict(R.BLOOM_DEFAULTS)
    struct = lambda d: R.RtwBloom(d["levels"], d["threshold"], d["knee"], int(d["karis"]), d["spread"], d["intensity"])
    good = struct(ok)
    for args in [(None, 5, 3, C.byref(good), P(out), P(layer)), (P(frame), 5, 3, None, P(out), P(layer)), (P(frame), 5, 3, C.byref(good), None, P(layer)),
                 (P(frame), 0, 3, C.byref(good), P(out), P(layer)), (P(frame), 5, 0, C.byref(good), P(out), P(layer)),
                 (P(frame), 0x7FFFFC01, 1, C.byref(good), P(out), P(layer)), (P(frame), 0x10000, 0x10000, C.byref(good), P(out), P(layer))]:
        assert fn(*head, *args, None) == -1, args
    for d in bloom_refusal_cases():
        assert fn(*head, P(frame), 5, 3, C.byref(struct(dict(ok, **d))), P(out), P(layer), None) == -1, d
    assert (out == 7).all() and (layer == 7).all()
    n = 5 * 3 * 3 * 4
    buf = np.full(3 * 5 * 3 * 3 + 16, 0.5, F)                                   # room for three frames
    before = buf.copy()
    at = lambda off: C.c_void_p(buf.ctypes.data + off)
    for lay in (0, 4, n - 4):                                                   # layer_out equal to in, inside it, at its last float
        assert fn(*head, at(0), 5, 3, C.byref(good), at(n), at(lay), None) == -1, lay
    for lay in (n, n + 4, 2 * n - 4, 4):                                        # ... likewise about out (and about both)
        assert fn(*head, at(0), 5, 3, C.byref(good), at(n), at(lay), None) == -1, lay
    assert fn(*head, at(0), 5, 3, C.byref(good), at(0), at(0), None) == -1      # in place, the layer too
    for off in (4, n - 4):                                                      # out overlapping in other than being it
        assert fn(*head, at(0), 5, 3, C.byref(good), at(off), None, None) == -1, off
        assert fn(*head, at(off), 5, 3, C.byref(good), at(0), None, None) == -1, off
    assert np.array_equal(buf, before)
    assert fn(*head, at(0), 5, 3, C.byref(good), at(n), at(2 * n), None) == 0   # the first byte behind a frame is no overlap
    assert fn(*head, at(0), 5, 3, C.byref(good), at(0), at(n), None) == 0       # out == in


def test_refusals():
    check_bloom_refusals(R.lib().rtw_bloom, ())
    frame = noise(5, 3)
    with pytest.raises(TypeError):
        R.bloom(frame, nonsense=1)
    with pytest.raises(ValueError):
        R.bloom(frame, out=np.empty((3, 5, 4), F))
    with pytest.raises(ValueError):
        R.bloom(np.zeros((3, 5), F))
    with pytest.raises(R.RtwError):
        R.bloom(frame, knee=2.0)
    with pytest.raises(TypeError):
        R.DisplayTransform(None, bloom=dict(nonsense=1))


class HostRenderer:
    """The three calls DisplayTransform.step makes, as the host forms."""
    luminance_histogram = staticmethod(R.luminance_histogram)
    bloom = staticmethod(R.bloom)
    display = staticmethod(R.display)


def test_display_transform_on_the_host_forms():
    frame = noise(33, 33, top=65536.0 * 64.0)
    blm = dict(levels=3, threshold=0.8, knee=0.4)
    out, level, exposure, stats = R.DisplayTransform(HostRenderer(), bloom=blm).step(frame)
    hist = R.luminance_histogram(frame)[0]
    assert (level, exposure) == R.exposure_from_histogram(hist)
    e = F(exposure)
    bloomed = R.bloom(frame, **dict(blm, threshold=float(F(0.8) / e), knee=float(F(0.4) / e)))[0]
    assert np.array_equal(out, R.display(bloomed, exposure=exposure)[0]) and stats["bloom"].taps > 0
    plain = R.DisplayTransform(HostRenderer()).step(frame)
    assert np.array_equal(plain[0], R.display(frame, exposure=exposure)[0]) and sorted(plain[3]) == ["counts", "display", "hist", "histogram"]
    assert exposure < 1e-3
    with pytest.raises(ValueError):                                             # threshold / exposure is not finite
        R.DisplayTransform(HostRenderer(), bloom=dict(threshold=3e38, knee=0.0)).step(frame)


def test_abi():
    assert C.sizeof(R.RtwBloom) == 24
    assert R.lib().rtw_abi_version() == 4
    assert R.BLOOM_MAX_LEVELS == 8
    assert R.BLOOM_DEFAULTS == {"levels": 6, "threshold": 1.0, "knee": 0.5, "karis": True, "spread": 0.5, "intensity": 0.25}
    for name in ("rtw_bloom_levels", "rtw_bloom", "rtw_ctx_bloom"):
        assert hasattr(R.lib(), name)
