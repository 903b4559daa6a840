"""The guided (joint bilateral) filter on the host (rtw_guided_filter, include/rtw.h): exp_plain's special cases and measured
error, the host path against an independent numpy restatement byte for byte, the anchors to rtw_bilateral_filter, the isolation the guides
give, non-finite guides, the window's excluded column and row, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.guided_common import (FORMATS, GUIDE_SETS, PROXIMITIES, SHAPES, SIGMA_DEPTH, SIGMA_NORMAL, SIZES, as_f32_frame, avg_of, guides,
                                 mismatch, pick, ref_guided, ulp_error, case_image)
from tests.test_bilateral_cpu import F, random_image, smooth_image


# ---- 1. exp_plain ----------------------------------------------------------------------------------------------------------------------
# The argument sets of the two tests below, as functions: tests/test_gpu_device_math.py runs the device compile of exp_plain on them.
EXP_SPECIAL_X = np.array([0.0, -0.0, -np.inf, np.nan, -88.0, -104.0, -1e30], F)


def exp_threshold_arguments():
    """every f32 from -87 down to -88: around exp(x) = 2^-126 (x = -87.3365...), where results start to be flushed to +0"""
    lo, hi = (int(F(v).view(np.uint32)) for v in (-87.0, -88.0))
    return np.arange(lo, hi, dtype=np.uint32).view(F)


def exp_arguments():
    rng = np.random.default_rng(11)
    return np.concatenate([np.linspace(-104.0, 0.0, 2 ** 22 + 1).astype(F), (-104.0 * rng.random(2 ** 20)).astype(F),
                           -np.exp(rng.uniform(np.log(1e-30), np.log(104.0), 2 ** 18)).astype(F)])       # ... and small arguments, log-spaced


def test_exp_plain_special_cases():
    x = EXP_SPECIAL_X
    got = R.exp_plain(x)
    assert got[0] == 1.0 and got[1] == 1.0
    assert got[2] == 0.0 and not np.signbit(got[2])
    assert np.isnan(got[3])
    assert not got[4:].any() and not np.signbit(got[4:]).any()
    # nothing below 2^-126 ever comes back: around the threshold (exp(x) = 2^-126 at x = -87.3365...) every result is +0 or normal
    near = R.exp_plain(exp_threshold_arguments())
    assert ((near == 0.0) | (near >= F(2.0 ** -126))).all() and not np.signbit(near).any()
    exact = np.exp(exp_threshold_arguments().astype(np.float64))
    assert np.array_equal(near == 0.0, exact < 2.0 ** -126)


def test_exp_plain_error_bound():
    x = exp_arguments()
    got = R.exp_plain(x)
    err, early, late = ulp_error(x, got)
    assert not early.any() and not late.any()          # +0 exactly where exp(x) < 2^-126
    assert (got <= 1.0).all() and (got >= 0.0).all()
    print(f"exp_plain: max error {err.max():.4f} ulp at x = {x[np.argmax(err)]!r}")
    # measured over every f32 in [-104, 0] by scripts/sweep_exp_plain.py: 0.9022 ulp (at x = -0.34103...); rounded up to the next 0.05
    assert err.max() <= 0.95, (err.max(), x[np.argmax(err)])


# ---- 2. the host path against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gset", list(GUIDE_SETS))
@pytest.mark.parametrize("fmt", FORMATS, ids=["u8", "f32"])
@pytest.mark.parametrize("prox", PROXIMITIES, ids=["square", "edges"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{w}x{h}" for h, w in SHAPES])
def test_host_matches_restatement(h, w, size, prox, fmt, gset):
    img = case_image(h, w)
    kw = pick(gset, *guides(h, w))
    ref = ref_guided(img, size, prox == R.PROXIMITY_EDGES, avg_of(h, w), **kw)
    out, st = R.guided_filter(img if fmt == R.PIXELS_U8 else as_f32_frame(img), size, proximity=prox, **kw)
    assert np.float32(st.avg_gradient).view(np.uint32) == avg_of(h, w).view(np.uint32)
    assert st.taps == R.bilateral_filter(img, size, prox)[1].taps
    assert mismatch(out, ref) is None, mismatch(out, ref)
    if size >= 3 and h > 3:
        assert out.any() and not np.array_equal(out, R.bilateral_filter(img, size, prox)[0])     # the guides do something


# ---- 3. anchors to the reference filter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prox", PROXIMITIES)
@pytest.mark.parametrize("size", SIZES)
def test_terms_off_and_constant_guides_give_the_bilateral_bytes(size, prox):
    for h, w in SHAPES:
        img = case_image(h, w)
        plain, sp = R.bilateral_filter(img, size, prox)
        depth, normal, ids = guides(h, w)
        for kw in (dict(), dict(depth=depth, normal=normal, ids=ids)):                                  # no guides; guides given, every term off
            out, st = R.guided_filter(img, size, proximity=prox, **kw)
            assert np.array_equal(out, plain) and st.taps == sp.taps and st.avg_gradient == sp.avg_gradient
        const = dict(depth=np.full((h, w), 3.25, F), normal=np.tile(np.array([0.6, 0.0, 0.8], F), (h, w, 1)), ids=np.full((h, w), 5, np.int32))
        out, _ = R.guided_filter(img, size, proximity=prox, sigma_depth=SIGMA_DEPTH, sigma_normal=SIGMA_NORMAL, same_object=True, **const)
        assert np.array_equal(out, plain)                                                               # g = exp_plain(-0) = 1
    f32 = as_f32_frame(case_image(17, 33))
    assert np.array_equal(R.guided_filter(f32, size, proximity=prox)[0], R.bilateral_filter(f32, size, prox)[0])


# ---- 4. / 5. isolation -----------------------------------------------------------------------------------------------------------------
def halves(h, w):
    ids = np.zeros((h, w), np.int32)
    ids[:, w // 2:] = 1
    return ids


@pytest.mark.parametrize("prox", PROXIMITIES)
def test_same_object_isolates_the_halves(prox):
    """avg_gradient is given, so the range term does not couple the halves: with same_object no tap crosses the split, and rewriting every
    pixel of one half leaves the other half's output unchanged."""
    h, w = 37, 70
    img = smooth_image(h, w, 51)
    ids = halves(h, w)
    a, _ = R.guided_filter(img, 10, ids=ids, same_object=True, proximity=prox, avg_gradient=0.1)
    other = img.copy()
    other[:, w // 2:] = random_image(h, w - w // 2, 52)
    assert not (other[:, w // 2:] == img[:, w // 2:]).all(axis=2).any()        # every pixel of the half is rewritten
    b, _ = R.guided_filter(other, 10, ids=ids, same_object=True, proximity=prox, avg_gradient=0.1)
    assert np.array_equal(a[:, :w // 2], b[:, :w // 2]) and a[:, :w // 2].any()
    assert not np.array_equal(a[:, w // 2:], b[:, w // 2:])
    # without the guide the left half near the split does change
    c, _ = R.bilateral_filter(img, 10, prox, avg_gradient=0.1)
    d, _ = R.bilateral_filter(other, 10, prox, avg_gradient=0.1)
    assert not np.array_equal(c[:, :w // 2], d[:, :w // 2])


@pytest.mark.parametrize("prox", PROXIMITIES)
def test_small_sigma_depth_isolates_like_same_object(prox):
    """Piecewise-constant depth 1 | 2 and sigma_depth 0.05: across the step a = 200 and exp_plain(-200) is the flushed +0, inside a half
    a = 0 and g = 1 -- the depth guide alone gives the same_object result."""
    h, w = 37, 70
    img = smooth_image(h, w, 53)
    ids = halves(h, w)
    depth = np.where(ids == 0, F(1.0), F(2.0)).astype(F)
    assert R.exp_plain(np.array([-200.0], F))[0] == 0.0
    by_depth, _ = R.guided_filter(img, 10, depth=depth, sigma_depth=0.05, proximity=prox, avg_gradient=0.1)
    by_id, _ = R.guided_filter(img, 10, ids=ids, same_object=True, proximity=prox, avg_gradient=0.1)
    assert np.array_equal(by_depth, by_id) and by_id.any()
    assert not np.array_equal(by_id, R.bilateral_filter(img, 10, prox, avg_gradient=0.1)[0])


# ---- 6. non-finite guides --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_depth_drops_the_tap(bad):
    """A pixel with a NaN or infinite depth weighs 0 in every other pixel's window -- as if it were another object -- and as a centre it
    drops all its taps: 0 / 0 -> NaN -> byte 0."""
    h, w = 17, 33
    img = smooth_image(h, w, 54)
    spots = [(5, 9), (0, 0), (h - 2, w - 2), (8, 20)]
    depth = np.full((h, w), 2.0, F)
    ids = np.zeros((h, w), np.int32)
    for k, (y, x) in enumerate(spots):
        depth[y, x] = bad
        ids[y, x] = k + 1
    out, _ = R.guided_filter(img, 3, depth=depth, sigma_depth=1.0, avg_gradient=0.1)
    as_objects, _ = R.guided_filter(img, 3, ids=ids, same_object=True, avg_gradient=0.1)
    keep = ids == 0
    assert np.array_equal(out[keep], as_objects[keep]) and out[keep].any()
    for y, x in spots:
        assert not out[y, x].any()
    assert not np.array_equal(out, R.bilateral_filter(img, 3, avg_gradient=0.1)[0])
    assert mismatch(out, ref_guided(img, 3, False, 0.1, depth=depth, sigma_depth=1.0)) is None
    # NaN in a normal likewise
    normal = np.tile(np.array([0.0, 0.0, 1.0], F), (h, w, 1))
    for y, x in spots:
        normal[y, x, 1] = bad
    out_n, _ = R.guided_filter(img, 3, normal=normal, sigma_normal=1.0, avg_gradient=0.1)
    assert np.array_equal(out_n, out)


# ---- 7. the column and the row whose windows exclude the centre ------------------------------------------------------------------------
@pytest.mark.parametrize("gset", list(GUIDE_SETS))
def test_last_column_and_row(gset):
    """x = w - 1: the window is x - size .. x, half-open, so the centre is not in it (the bottom row likewise); their taps all lie to the
    left (above), and the guide weight is still taken against the centre's guides."""
    for h, w in SHAPES:
        img = case_image(h, w)
        kw = pick(gset, *guides(h, w))
        for prox in PROXIMITIES:
            out, _ = R.guided_filter(img, 3, proximity=prox, avg_gradient=0.2, **kw)
            ref = ref_guided(img, 3, prox == R.PROXIMITY_EDGES, 0.2, **kw)
            assert np.array_equal(out[:, -1], ref[:, -1]) and np.array_equal(out[-1, :], ref[-1, :])
    # 3x3, size 1, an object of its own in the centre pixel: the corner (2, 2) takes the single tap (1, 1), which is dropped -> 0
    img = np.full((3, 3, 3), 200, np.uint8)
    img[1, 1] = (255, 128, 8)
    ids = np.zeros((3, 3), np.int32)
    ids[1, 1] = 1
    assert R.bilateral_filter(img, 1, avg_gradient=1.0)[0][2, 2].any()
    assert not R.guided_filter(img, 1, ids=ids, same_object=True, avg_gradient=1.0)[0][2, 2].any()


# ---- 8. argument checks ----------------------------------------------------------------------------------------------------------------
def test_error_paths_host():
    img = random_image(8, 8, 1)
    out = np.empty_like(img)
    depth, normal, ids = np.ones((8, 8), F), np.ones((8, 8, 3), F), np.ones((8, 8), np.int32)
    ip, op = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    dp, np_, xp = (C.c_void_p(a.ctypes.data) for a in (depth, normal, ids))
    call = R.lib().rtw_guided_filter

    def prm(sd=0.0, sn=0.0, same=0, size=2, prox=R.PROXIMITY_SQUARE, fmt=R.PIXELS_U8, avg=0.0):
        return C.byref(R.RtwGuidedFilter(R.RtwBilateral(size, prox, fmt, avg), sd, sn, same))

    assert call(ip, 8, 8, dp, np_, xp, prm(1.0, 1.0, 1), op, None) == 0                      # stats may be NULL
    assert call(ip, 8, 8, None, None, None, prm(), op, None) == 0                             # a NULL guide whose term is off is accepted
    assert call(ip, 8, 8, None, np_, xp, prm(0.0, 1.0, 1), op, None) == 0
    assert call(ip, 8, 8, dp, None, xp, prm(1.0, 0.0, 1), op, None) == 0
    assert call(ip, 8, 8, dp, np_, None, prm(1.0, 1.0, 0), op, None) == 0
    # everything rtw_bilateral_filter refuses
    assert call(None, 8, 8, dp, np_, xp, prm(), op, None) == -1
    assert call(ip, 8, 8, dp, np_, xp, None, op, None) == -1
    assert call(ip, 8, 8, dp, np_, xp, prm(), None, None) == -1
    assert call(ip, 2, 8, dp, np_, xp, prm(), op, None) == -1
    assert call(ip, 8, 2, dp, np_, xp, prm(), op, None) == -1
    assert call(ip, 65536, 3, dp, np_, xp, prm(), op, None) == -1
    assert call(ip, 8, 8, dp, np_, xp, prm(prox=2), op, None) == -1
    assert call(ip, 8, 8, dp, np_, xp, prm(fmt=2), op, None) == -1
    assert call(ip, 8, 8, dp, np_, xp, prm(size=R.BILATERAL_MAX_SIZE + 1), op, None) == -1
    for v in (-1.0, float("nan"), float("inf")):
        assert call(ip, 8, 8, dp, np_, xp, prm(avg=v), op, None) == -1
    # the sigmas: negative, not finite, or so small that 0.5 / sigma^2 is not finite
    for v in (-1.0, -0.0 - 1e-30, float("nan"), float("inf"), float("-inf"), 1e-20, 1e-30):
        assert call(ip, 8, 8, dp, np_, xp, prm(sd=v), op, None) == -1, v
        assert call(ip, 8, 8, dp, np_, xp, prm(sn=v), op, None) == -1, v
    assert call(ip, 8, 8, dp, np_, xp, prm(sd=1e-19, sn=1e-19), op, None) == 0               # 0.5 / 1e-38 = 5e37: finite
    # a term that is on without its guide
    assert call(ip, 8, 8, None, np_, xp, prm(sd=1.0), op, None) == -1
    assert call(ip, 8, 8, dp, None, xp, prm(sn=1.0), op, None) == -1
    assert call(ip, 8, 8, dp, np_, None, prm(same=1), op, None) == -1
    assert call(ip, 8, 8, dp, np_, xp, prm(same=2), op, None) == -1
    # the Python layer: guides are shape-checked against the image
    with pytest.raises(ValueError):
        R.guided_filter(img, 2, depth=np.ones((8, 7), F), sigma_depth=1.0)
    with pytest.raises(ValueError):
        R.guided_filter(img, 2, normal=np.ones((8, 8), F), sigma_normal=1.0)
    with pytest.raises(ValueError):
        R.guided_filter(img, 2, ids=np.ones((7, 8), np.int32), same_object=True)
    with pytest.raises(R.RtwError):
        R.guided_filter(img, 2, sigma_depth=1.0)
    assert R.guided_filter(random_image(3, 3, 2), R.BILATERAL_MAX_SIZE, ids=np.zeros((3, 3), np.int32), same_object=True)[0].shape == (3, 3, 3)


def test_pod_layout():
    assert C.sizeof(R.RtwGuidedFilter) == 28 and R.RtwGuidedFilter.sigma_depth.offset == 16 and R.RtwGuidedFilter.same_object.offset == 24
    assert R.lib().rtw_abi_version() == 4
