"""The host form of the guide-steered upsampling (rtw_upsample_filter, rtw_camera_scaled; include/rtw.h "guided upsampling"):
against the numpy float32 restatement of tests/upsample_common.py bit for bit over the size, scale, radius and term matrix; known
answers whose arithmetic is exact; the fallback and wsum_out; non-finite low pixels; floors and signed zero; every refusal; camera_scaled
against pixel_rays; and a float64 reference with a bound derived from the rule's roundings.  No GPU."""
import numpy as np
import pytest

import rtw_amd as R
from tests.upsample_common import (EDGE_IDS, F, FLOOR, RADII, SCALES, SIZES, TERMS, U, check_upsample_refusals, edge_inputs, edge_pixels, guides_for,
                                   host_upsample, inputs, lo_size, mismatch, ref64, restate, same_bits, taps_inside, term_kw)

SIZE_IDS = lambda s: f"{s[0]}x{s[1]}"
OFF = dict(sigma_depth=0.0, sigma_normal=0.0, same_object=False)


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_host_form_equals_the_restatement(size, scale):
    w, h = size
    fr, g_lo, g_hi = inputs(w, h, scale)
    for radius in RADII:
        for terms in TERMS:
            out, ws, taps = host_upsample(w, h, scale, radius, terms)
            want, wws = restate(fr, size, guides_for(g_lo, terms), guides_for(g_hi, terms), scale, radius, **term_kw(terms))
            assert same_bits(out, want), (size, scale, radius, terms, mismatch(out, want))
            assert same_bits(ws, wws), (size, scale, radius, terms, "wsum", mismatch(ws, wws))
            assert taps == taps_inside(size, scale, radius)


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_scale_1_radius_1_without_terms_is_the_identity(size):
    w, h = size
    fr = inputs(w, h, 1)[0]
    out, ws, _ = R.upsample_filter(fr, size, scale=1, radius=1, out_wsum=True, **OFF)
    assert out.tobytes() == fr.tobytes() and (ws == 1.0).all()


@pytest.mark.parametrize("scale", [1, 2, 4, 8])
def test_small_integers_give_the_exact_clamped_bilinear_value(scale):
    """lo = 4 I + 64 J (+ the channel): with a power-of-two scale every weight is a multiple of 1/16, every product and sum an integer
    over 256 well inside 24 bits, and the weights of a pixel sum to 1 -- or, on the first and last rows and columns, to the part inside
    the frame, which the division takes out again: the bilinear value with clamped coordinates, exactly."""
    for w, h in ((33, 17), (13, 7), (16, 8)):
        w_lo, h_lo = lo_size(w, h, scale)
        JJ, II = np.mgrid[0:h_lo, 0:w_lo]
        fr = np.stack([4.0 * II + 64.0 * JJ + c for c in range(3)], -1).astype(F)
        out, ws, _ = R.upsample_filter(fr, (w, h), scale=scale, radius=1, out_wsum=True, **OFF)
        x = np.clip((np.arange(w) + 0.5) / scale - 0.5, 0.0, w_lo - 1.0)
        y = np.clip((np.arange(h) + 0.5) / scale - 0.5, 0.0, h_lo - 1.0)
        want = np.stack([4.0 * x[None, :] + 64.0 * y[:, None] + c for c in range(3)], -1)
        assert np.array_equal(out.astype(np.float64), want), (scale, (w, h), np.abs(out - want).max())
        assert (ws > 0).all()


def test_a_single_matching_tap_is_remodulated_with_the_pixels_own_albedo():
    """Scale 2, small integers and powers of two: output pixel (3, 3) sits between low pixels (1..2, 1..2); its id matches low pixel (2, 1)
    alone, so C = L[1][2] = (lo - e) / a there, and out = C * albedo_hi + emitted_hi."""
    w, h, s = 8, 6, 2
    w_lo, h_lo = lo_size(w, h, s)
    fr = np.full((h_lo, w_lo, 3), 100.0, F)
    lo = dict(idx=np.zeros((h_lo, w_lo), np.int32), albedo=np.full((h_lo, w_lo, 3), 0.5, F), emitted=np.zeros((h_lo, w_lo, 3), F))
    hi = dict(idx=np.zeros((h, w), np.int32), albedo=np.full((h, w, 3), 0.25, F), emitted=np.zeros((h, w, 3), F))
    fr[1, 2] = (7.0, 12.0, 20.0)
    lo["idx"][1, 2], lo["albedo"][1, 2], lo["emitted"][1, 2] = 9, (2.0, 4.0, 8.0), (1.0, 4.0, 4.0)       # L = (3, 2, 2)
    hi["idx"][3, 3], hi["albedo"][3, 3], hi["emitted"][3, 3] = 9, (0.5, 8.0, FLOOR / 2), (16.0, 1.0, 3.0)
    out, ws, _ = R.upsample_filter(fr, (w, h), lo=lo, hi=hi, scale=s, radius=1, sigma_depth=0.0, sigma_normal=0.0, same_object=True,
                                   albedo_floor=FLOOR, out_wsum=True)
    assert out[3, 3].tolist() == [3.0 * 0.5 + 16.0, 2.0 * 8.0 + 1.0, 2.0 * 1.0 + 3.0]                     # (blue: below the floor, not multiplied)
    assert ws[3, 3] == F(0.75) * F(0.25)                                                                  # tx = 3/4 towards I0 + 1 = 2, ty = 3/4 towards 2
    others = np.ones((h, w), bool)
    others[3, 3] = False
    assert (out[others] == 200.0 * 0.25).all()                                                            # elsewhere the flat 100 / 0.5 times 0.25


# ---- 3. the fallback -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("scale", [2, 3])
def test_a_pixel_no_tap_reaches_takes_its_covering_low_pixel(scale, radius):
    w, h = 13, 7
    fr, g_lo, g_hi = inputs(w, h, scale)
    ids_hi = np.zeros((h, w), np.int32)
    lonely = [(0, 0), (3, 6), (h - 1, w - 1), (2, 11)]
    for n, (j, i) in enumerate(lonely):
        ids_hi[j, i] = 100 + n
    lo, hi = dict(idx=np.zeros_like(g_lo["idx"])), dict(idx=ids_hi)
    out, ws, _ = R.upsample_filter(fr, (w, h), lo=lo, hi=hi, scale=scale, radius=radius, sigma_depth=0.0, sigma_normal=0.0, same_object=True,
                                   out_wsum=True)
    zero = np.zeros((h, w), bool)
    for j, i in lonely:
        zero[j, i] = True
        assert same_bits(out[j, i], fr[j // scale, i // scale])
    assert np.array_equal(ws == 0.0, zero)
    want, wws = restate(fr, (w, h), lo, hi, scale, radius, same_object=True)
    assert same_bits(out, want) and same_bits(ws, wws)


# ---- 4. values that are not finite -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4), ids=EDGE_IDS[:4])
def test_a_low_pixel_that_is_not_finite_is_dropped_from_every_footprint(which):
    """A bad low pixel away from the frame's edge shares every footprint it lies in with good pixels that carry weight -- but for the centre
    pixel of its block at scale 3 and radius 1, whose footprint is that one tap (tx = ty = 0) -- so the output is finite everywhere else;
    where it is the only tap it is the fallback and passes through, and wsum is 0 exactly there.  At scale 1 and radius 1 that is every pixel
    of a bad low pixel.  (3e38 is finite until it is demodulated: divided by an albedo of 0.5 it is not.)"""
    w, h = 33, 17
    px = np.array(edge_pixels()[which], F)
    bad = ~np.isfinite(px / F(0.5))
    for scale, radius in ((2, 1), (2, 2), (3, 1), (3, 2), (1, 2)):
        w_lo, h_lo = lo_size(w, h, scale)
        places = ((1, 1), (h_lo // 2, w_lo // 2), (h_lo - 2, w_lo - 2))
        fr = edge_inputs(w, h, scale, places, which)[0]
        lo = dict(albedo=np.full((h_lo, w_lo, 3), 0.5, F))
        out, ws, _ = R.upsample_filter(fr, (w, h), lo=lo, scale=scale, radius=radius, albedo_floor=FLOOR, out_wsum=True, **OFF)
        alone = np.zeros((h, w), bool)
        if (scale, radius) == (3, 1):
            for J, I in places:
                alone[3 * J + 1, 3 * I + 1] = True
        assert np.array_equal(ws == 0.0, alone), (scale, radius)
        assert np.array_equal(~np.isfinite(out), alone[..., None] & bad[None, None, :]), (scale, radius)
        want, wws = restate(fr, (w, h), lo, None, scale, radius)
        assert same_bits(out, want) and same_bits(ws, wws)
        other = np.array(fr)                                                   # dropped: what the bad value is does not matter
        for J, I in places:
            other[J, I] = np.nan
        again = R.upsample_filter(other, (w, h), lo=lo, scale=scale, radius=radius, albedo_floor=FLOOR, **OFF)[0]
        assert same_bits(again[~alone], out[~alone])
    w_lo, h_lo = lo_size(w, h, 1)
    places = ((0, 0), (h_lo // 2, w_lo // 2), (h_lo - 1, w_lo - 1))
    fr = edge_inputs(w, h, 1, places, which)[0]
    lo = dict(albedo=np.full((h_lo, w_lo, 3), 0.5, F))
    out, ws, _ = R.upsample_filter(fr, (w, h), lo=lo, scale=1, radius=1, albedo_floor=FLOOR, out_wsum=True, **OFF)
    at = np.zeros((h, w), bool)
    for J, I in places:
        at[J, I] = True
    assert np.array_equal(ws == 0.0, at)
    assert np.array_equal(~np.isfinite(out), at[..., None] & bad[None, None, :])
    assert same_bits(out, (fr / F(0.5)).astype(F))                           # (no albedo on the output side)


# ---- 5. floors and signed zero -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [4, 5], ids=EDGE_IDS[4:])
def test_denormals_and_negative_zero_keep_the_restatements_bytes(which):
    w, h = 13, 7
    for scale in (1, 2, 3):
        w_lo, h_lo = lo_size(w, h, scale)
        places = ((0, 0), (h_lo // 2, w_lo // 2), (h_lo - 1, w_lo - 1), (1, 2))
        fr, g_lo, g_hi = edge_inputs(w, h, scale, places, which)
        for radius in RADII:
            for terms in (TERMS[0], TERMS[-1], (False, False, False, True)):
                out, ws, _ = R.upsample_filter(fr, (w, h), lo=guides_for(g_lo, terms), hi=guides_for(g_hi, terms), scale=scale, radius=radius,
                                               out_wsum=True, **term_kw(terms))
                want, wws = restate(fr, (w, h), guides_for(g_lo, terms), guides_for(g_hi, terms), scale, radius, **term_kw(terms))
                assert same_bits(out, want), (scale, radius, terms, mismatch(out, want))
                assert same_bits(ws, wws)


def test_an_albedo_below_the_floor_neither_divides_nor_multiplies():
    w, h, s = 4, 4, 1
    fr = np.full((h, w, 3), 6.0, F)
    below, at = np.nextafter(F(FLOOR), F(0.0)), F(FLOOR)
    lo = dict(albedo=np.tile(np.array([below, at, 2.0], F), (h, w, 1)))
    hi = dict(albedo=np.tile(np.array([4.0, below, at], F), (h, w, 1)))
    out = R.upsample_filter(fr, (w, h), lo=lo, hi=hi, scale=s, radius=1, albedo_floor=FLOOR, **OFF)[0]
    want = np.array([F(6.0) * F(4.0), F(6.0) / at, F(3.0) * at], F)           # r: in untouched, out times 4; g: in divided, out untouched; b: both
    assert same_bits(out, np.tile(want, (h, w, 1)))
    for zero in (0.0, -0.0):                                                   # a zero albedo is below every floor
        lo = dict(albedo=np.full((h, w, 3), zero, F))
        assert same_bits(R.upsample_filter(fr, (w, h), lo=lo, hi=lo, scale=s, radius=1, albedo_floor=FLOOR, **OFF)[0], fr)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_error_paths_host():
    check_upsample_refusals(R.lib().rtw_upsample_filter, ())


def test_python_surface_checks_shapes():
    fr, g_lo, g_hi = inputs(5, 4, 2)
    with pytest.raises(ValueError):
        R.upsample_filter(fr[..., :2], (5, 4), scale=2, **OFF)
    with pytest.raises(ValueError):
        R.upsample_filter(fr, (5, 4), lo=dict(g_lo, depth=g_hi["depth"]), hi=g_hi, scale=2, sigma_depth=0.5)
    with pytest.raises(R.RtwError):
        R.upsample_filter(fr, (5, 4), lo={}, hi=g_hi, scale=2)                # a term on whose guide is missing
    with pytest.raises(R.RtwError):
        R.upsample_filter(fr, (6, 4), scale=3, **OFF)                         # not the ceiling
    assert R.UPSAMPLE_DEFAULTS["radius"] in (1, 2)


# ---- 7. camera_scaled --------------------------------------------------------------------------------------------------------------------------
def _camera():
    cam, _ = R.default_view(R.SCENE_C2)
    return cam


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_camera_scaled_pixel_centres_are_the_block_centres(scale):
    """Offset (0.5, 0.5) of low pixel (I, J) against offset (0, 0) of pixel (s I + s / 2, s J + s / 2): delta * s is exact for a power of
    two, and (delta s)(I + 0.5) and delta (s I + s / 2) are the same product scaled by that power, so they round alike."""
    cam = _camera()
    for w, h in ((64, 48), (50, 37)):
        w_lo, h_lo = lo_size(w, h, scale)
        W, H = w_lo * scale, h_lo * scale                                     # (the last block may reach beyond the frame)
        low = R.pixel_rays(R.camera_scaled(cam, scale), w_lo, h_lo, (0.5, 0.5)).reshape(h_lo, w_lo, 6)
        full = R.pixel_rays(cam, W, H, (0.0, 0.0)).reshape(H, W, 6)
        assert same_bits(low, full[scale // 2::scale, scale // 2::scale])


def test_camera_scaled_restated():
    cam = _camera()
    for scale in (1, 3, 5, 8):
        c = R.camera_scaled(cam, scale)
        for name, _ in R.RtwCamera._fields_:
            a, b = np.array(getattr(c, name), F), np.array(getattr(cam, name), F)
            want = (b * F(scale)).astype(F) if name in ("delta_u", "delta_v") else b
            assert same_bits(a, want), (scale, name)
        w_lo, h_lo = 7, 5
        rays = R.pixel_rays(c, w_lo, h_lo, (0.5, 0.5)).reshape(h_lo, w_lo, 6)
        du, dv, p00 = (np.array(getattr(c, k), F) for k in ("delta_u", "delta_v", "pixel00"))
        for J in range(h_lo):
            for I in range(w_lo):
                want = (p00 + du * (F(I) + F(0.5))) + dv * (F(J) + F(0.5))
                assert same_bits(rays[J, I, 3:], want) and same_bits(rays[J, I, :3], np.array(cam.origin, F))
    out = R.RtwCamera()
    L = R.lib()
    for bad in (0, R.UPSAMPLE_MAX_SCALE + 1):
        assert L.rtw_camera_scaled(R.C.byref(cam), bad, R.C.byref(out)) == -1
        with pytest.raises(R.RtwError):
            R.camera_scaled(cam, bad)
    assert L.rtw_camera_scaled(None, 2, R.C.byref(out)) == -1 and L.rtw_camera_scaled(R.C.byref(cam), 2, None) == -1


# ---- 8. float64 --------------------------------------------------------------------------------------------------------------------------------
SHARES = {}


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("size", SIZES[1:], ids=SIZE_IDS)
def test_host_form_lies_within_the_derived_bound_of_the_float64_rule(size, scale):
    """The bound is tests/upsample_common.py's, derived from the rule's roundings before any output was looked at.  The largest share of it
    that the host form uses, over the whole matrix, is recorded in DESIGN.md 8i."""
    w, h = size
    fr, g_lo, g_hi = inputs(w, h, scale)
    worst = 0.0
    for radius in RADII:
        for terms in TERMS:
            out = host_upsample(w, h, scale, radius, terms)[0]
            val, err = ref64(fr, size, guides_for(g_lo, terms), guides_for(g_hi, terms), scale, radius, **term_kw(terms))
            diff = np.abs(out.astype(np.float64) - val)
            assert (diff <= err).all(), (size, scale, radius, terms, float((diff / np.maximum(err, 1e-300)).max()))
            loose = err > 2.0 ** -12 * max(1.0, float(np.abs(val).max()))       # a bound above this is no statement: flushed weights
            assert loose.mean() <= 0.10, (size, scale, radius, terms, float(loose.mean()))
            diff = np.where(loose, 0.0, diff)
            worst = max(worst, float((diff / np.maximum(err, 1e-300)).max()))
    SHARES[(size, scale)] = worst
    print(f"upsample f64: {size} scale {scale}: largest share of the bound {worst:.3f}")
