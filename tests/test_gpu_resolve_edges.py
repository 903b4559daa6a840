"""The resolve (rtw_kernels.hip resolve_kernel: sum in sample order, / n, powf(mean, 1 / gamma)) at the edges of its values.

Values get in through the background of an empty scene: under RTW_INTEGRATOR_RUST2 at depth 0 every sample of every pixel IS the background
colour (rtw.h), so an 8 x 8 frame carries three chosen f32 values through the bank, the sum, the division and the gamma step.

Bar (DESIGN.md "Parity"): gamma 1 is the oracle's frame on the bits; any other gamma is within 2 units of the last place of a plain f64
np.power rounded to f32, and of the oracle's glibc powf, with the same NaN / +-inf / +-0 wherever the reference has one.  No value and no
gamma of render_limits_common.RESOLVE_VALUES / RESOLVE_GAMMAS is left out: zeros, subnormals, FLT_MAX, infinities, negatives and NaN under
gammas 0, +inf, negative and NaN included.  A -0 background never reaches the gamma step as -0: the sum starts from +0, and +0 + -0 is +0.

Measured on an MI355X over the whole grid (7 frames x 11 gammas x 2 counts): at most 1 ulp from the f64 reference and at most 1 ulp from the
oracle, the one subnormal result included (1e-20 at gamma 0.5), and the same class at every special input; each case prints its own figures.

The order of the sum is part of the image's definition: it is checked against numpy alone on equal samples, for every unit length, in one
band and in several, and under RTW_FLAG_CHUNK_SUMS against the association rtw.h documents."""
import numpy as np
import pytest

import rtw_amd as R
from tests import render_limits_common as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(rtw):
    """A context of this module's own: the options of the sum's tests never reach another test."""
    with rtw.Renderer(0) as r:
        yield r


@pytest.mark.parametrize("k", range(len(X.RESOLVE_FRAMES)))
def test_resolve_value_edges(ctx, oracle, k):
    background = X.RESOLVE_FRAMES[k]
    scene, cam = X.empty_scene(background), X.pixel_camera()
    ctx.set_scene(scene)
    misses, worst_ref, worst_orc = [], 0, 0
    for n in X.RESOLVE_SAMPLES:
        # 1. gamma 1: the oracle's frame on the bits (every NaN equal, the sign of zero included)
        p = X.resolve_params(1.0, n)
        L, st = ctx.render(cam, p)
        ref, st_ref = oracle.render(cam, scene, p, 1)
        assert X.same_bits(L, ref), (background, n, L[0, 0], ref[0, 0])
        assert st.camera_rays == st_ref.camera_rays == 64 * n
        assert st.nan_pixels == X.nan_pixel_count(L) == st_ref.nan_pixels, (background, n, st.nan_pixels, st_ref.nan_pixels)
        assert (L == L[0, 0]).all() or np.isnan(L[0, 0]).any()        # (every pixel carries the same three values)
        for gamma in X.RESOLVE_GAMMAS[1:]:
            p = X.resolve_params(gamma, n)
            img, st = ctx.render(cam, p)
            orc, st_orc = oracle.render(cam, scene, p, 1)
            want = X.pow_reference(L, gamma)
            # 2. against the plain f64 reference
            classes, worst, finite = X.compare_pow(img, want)
            worst_ref = max(worst_ref, worst)
            line = f"background {background} n {n} gamma {gamma}: device {img[0, 0]} f64 {want[0, 0]} oracle {orc[0, 0]}"
            print(f"{line}; ulp vs f64 {worst}", end="")
            if not (classes and finite and worst <= X.RESOLVE_ULP):
                misses.append(("f64", line, classes, finite, worst))
            # 3. against the oracle (glibc powf)
            classes, worst, finite = X.compare_pow(img, orc)
            worst_orc = max(worst_orc, worst)
            print(f", vs oracle {worst}")
            if not (classes and finite and worst <= X.RESOLVE_ULP):
                misses.append(("oracle", line, classes, finite, worst))
            # 4. nan_pixels: the device's own frame, and the oracle's count
            if not (st.nan_pixels == X.nan_pixel_count(img) == st_orc.nan_pixels):
                misses.append(("nan_pixels", line, st.nan_pixels, X.nan_pixel_count(img), st_orc.nan_pixels))
            if gamma == X.INF and st.nan_pixels != 0:                 # pow(x, 0) is 1, for a NaN mean too
                misses.append(("nan_pixels at gamma inf", line, st.nan_pixels))
    print(f"frame {k}: worst distance vs f64 {worst_ref} ulp, vs the oracle {worst_orc} ulp")
    assert not misses, misses


@pytest.mark.parametrize("flags", [0, R.FLAG_CHUNK_SUMS])
@pytest.mark.parametrize("bands", [1, 2])
@pytest.mark.parametrize("chunk_len", X.SUM_CHUNK_LENS)
def test_sum_is_added_in_sample_order(ctx, chunk_len, bands, flags):
    """Equal samples b: every pixel is (((0 + b) + b) + ..) / n on the bits, whatever the unit length and however many bands -- or, under
    RTW_FLAG_CHUNK_SUMS, the chunks of four added left to right and the chunks' sums in chunk order."""
    ctx.set_scene(X.empty_scene(X.SUM_BACKGROUND))
    cam = X.field_camera(9, 9)
    want_of = X.mean_chunk_sums if flags else X.mean_in_order
    try:
        ctx.set_option(R.OPT_CHUNK_LEN, chunk_len)
        for n in X.SUM_COUNTS:
            # 9 x 9 is two tile rows of two tiles: a budget of one tile row's bank renders it in two bands
            slots = (n + X.SUM_CHUNK - 1) // X.SUM_CHUNK if flags else n
            ctx.set_option(R.OPT_SAMPLE_BANK_GB, X.bank_gb_for_band(2, slots, 1) if bands == 2 else 48)
            img, st = ctx.render(cam, X.sum_params(n, flags))
            want = want_of(X.SUM_BACKGROUND, n)
            assert st.camera_rays == 81 * n and st.nan_pixels == 0
            assert X.same_bits(img, np.broadcast_to(want, img.shape)), (chunk_len, bands, flags, n, img[0, 0], img[8, 8], want)
    finally:
        ctx.set_option(R.OPT_CHUNK_LEN, 0)
        ctx.set_option(R.OPT_SAMPLE_BANK_GB, 48)
