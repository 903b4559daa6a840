"""Conditions on the inputs of test_gpu_render_limits.py and test_gpu_resolve_edges.py, checked with the oracle and numpy alone: the cases
reach what they are meant to reach, and the references are defined everywhere.  No GPU."""
import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests import render_limits_common as X

f32 = np.float32


# ---- A ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.FRAMES))
def test_every_frame_is_accepted_by_the_oracle_and_looks_into_the_sphere_field(name):
    w, h, n, part, rows = X.FRAMES[name]
    img, st = X.frame_oracle(name)                                    # (O.render asserts the oracle's status)
    assert img.shape == (rows, w, 3) and st.rows == rows
    assert st.camera_rays == rows * w * n
    assert st.segments > 1.1 * st.camera_rays, (name, st.segments / st.camera_rays)       # more than a tenth of the paths hit something
    assert st.nan_pixels == 0 and np.isfinite(img).all()
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > rows * w // 4     # (not a flat frame: a shifted or truncated pixel id would show)


def test_frames_reach_the_packed_fields():
    assert X.DIM_MAX == 0xFFFF and X.SAMPLES_MAX == 0xFFFFFF
    # the far corner's pixel id needs all 32 bits, and its row the upper half of the (column, row) register
    assert (X.DIM_MAX - 1) * X.DIM_MAX + (X.DIM_MAX - 1) == 0xFFFE0000 > 1 << 31             # j * width + i of pixel (65534, 65534)
    assert (X.DIM_MAX - 1) | (X.DIM_MAX - 1) << 16 == 0xFFFEFFFE == 4294901758                 # ... and its packed (column, row)
    assert (X.DIM_MAX + 7) // 8 == 8192


def test_part_rows_of_the_corner_cases():
    L = R.lib()
    assert L.rtw_part_rows(X.DIM_MAX, 1, X.DIM_MAX - 1, X.DIM_MAX) == 1 == X.FRAMES["corner row"][4]
    assert L.rtw_part_rows(X.DIM_MAX, 8, 8191, 8192) == 7 == X.FRAMES["corner block"][4]
    # ... and they are the image's last rows: the oracle's partial frames are the tail of nothing else
    assert [r for r in range(X.DIM_MAX) if (r // 8) % 8192 == 8191] == list(range(65528, 65535))
    # the three contexts of the 24-row frame: blocks of 8, and the ragged blocks of 5
    assert [L.rtw_part_rows(24, 8, k, 3) for k in range(3)] == [8, 8, 8]
    assert [L.rtw_part_rows(24, 5, k, 3) for k in range(3)] == [10, 9, 5]


def test_band_budget_of_the_tall_frame():
    """1 x 65535 at 1 spp: 8192 tile rows of one tile; bands of 100 tile rows are 82 bands, the last one 92 tile rows."""
    gb = X.bank_gb_for_band(1, 1, 100)
    bank_bytes = int(gb * (1 << 30))
    per_band = (bank_bytes // 12) // 64                               # the shim's rule: slots the budget holds / slots per tile row
    assert per_band == 100
    bands, last = -(-8192 // per_band), 8192 % per_band
    assert 32 <= bands <= 128 and 0 < last < per_band


# ---- B ------------------------------------------------------------------------------------------------------------------------------
def test_sampler_count_boundaries_by_arithmetic():
    for integ, sampler, samples, rays in X.SAMPLE_CASES:
        if samples == 0:
            assert rays is None
            continue
        n, root = X.sampler_count(sampler, samples)
        if rays is None:
            assert n >= 1 << 24, (sampler, samples, n)                 # refused: the count does not fit beside the samples left
        else:
            assert n == rays <= X.SAMPLES_MAX and root <= X.ROOT_MAX, (sampler, samples, n)
    assert X.sampler_count(R.SAMPLER_STRATIFIED, X.ROOT_MAX ** 2) == (X.ROOT_MAX ** 2, X.ROOT_MAX)
    assert X.sampler_count(R.SAMPLER_STRATIFIED, X.ROOT_MAX ** 2 + 1)[1] == X.ROOT_MAX + 1
    assert X.sampler_count(R.SAMPLER_CENTRES, X.SAMPLES_MAX)[1] == X.ROOT_MAX          # sqrtf(16777215) rounds below 4096
    assert X.sampler_count(R.SAMPLER_CENTRES, 1 << 24)[1] == X.ROOT_MAX + 1


@pytest.mark.parametrize("sampler,integ", [(R.SAMPLER_ROW, R.INTEGRATOR_GRADIENT), (R.SAMPLER_STRATIFIED, R.INTEGRATOR_GRADIENT),
                                           (R.SAMPLER_CENTRES, R.INTEGRATOR_RUST2)])
def test_sampler_count_is_the_oracles_at_small_counts(sampler, integ):
    """camera_rays of the oracle on a 1 x 1 frame: the same rule the arithmetic above applies at the large counts."""
    for samples in (1, 2, 3, 4, 5, 8, 9, 10, 15, 16, 17, 99, 100, 101):
        _, st = O.render(X.pixel_camera(), X.empty_scene(), X.pixel_params(integ, sampler, samples), 1)
        assert st.camera_rays == X.sampler_count(sampler, samples)[0], (sampler, samples)
        assert st.segments == st.camera_rays                          # every path is one query that misses


# ---- C ------------------------------------------------------------------------------------------------------------------------------
def test_every_value_and_gamma_is_in_the_grid():
    flat = [v for frame in X.RESOLVE_FRAMES for v in frame]
    assert len(X.RESOLVE_FRAMES) == 7 and all(len(fr) == 3 for fr in X.RESOLVE_FRAMES)
    bits = {f32(v).view(np.uint32).item() for v in flat if v == v}
    want = [0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 1e-30, 1e-3, 0.18, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 2.0, 255.0, 1e30, X.FLT_MAX,
            X.INF, -1e-30, -0.5, -X.INF]
    assert all(f32(v).view(np.uint32).item() in bits for v in want) and sum(1 for v in flat if v != v) == 1
    assert f32(2.0 ** -149) > 0 and f32(1.0 - 2.0 ** -24) < 1 < f32(1.0 + 2.0 ** -23)          # (the values survive the trip to f32)
    assert len(X.RESOLVE_GAMMAS) == 12 and X.RESOLVE_GAMMAS[0] == 1.0 and X.RESOLVE_SAMPLES == (1, 4)


def test_reference_defines_every_value_gamma_pair():
    """np.power in f64 gives each (mean, gamma) a class (NaN, +-inf, +-0) or a finite non-zero f32; numpy raises nothing with its warnings
    silenced.  The means are those of 1 and of 4 equal samples, formed as the resolve forms them."""
    classes = set()
    subnormal = 0
    for n in X.RESOLVE_SAMPLES:
        with np.errstate(all="ignore"):
            L = f32([X.mean_in_order(frame, n) for frame in X.RESOLVE_FRAMES])
        for g in X.RESOLVE_GAMMAS[1:]:
            ref = X.pow_reference(L, g)
            assert ref.dtype == f32 and ref.shape == L.shape
            c = X.value_class(ref)
            fin = c == 0
            assert np.isfinite(ref[fin]).all() and (ref[fin] != 0).all()
            classes |= set(c.ravel().tolist())
            subnormal += int((np.abs(ref[fin]) < np.finfo(f32).tiny).sum())
    assert classes >= {0, 1, 2, 4}                                   # finite, NaN, +inf and +0 all occur
    assert subnormal >= 1                                             # the subnormal range of the result is reached (1e-20 at gamma 0.5)
    # a NaN mean under gamma +inf is 1: pow(x, 0) is 1 for every x
    assert X.pow_reference(f32([X.NAN]), X.INF)[0] == 1.0


def test_the_oracle_resolves_the_background_as_given():
    """RUST2 at depth 0 hands the resolve the background's bits, -0 and NaN included: at gamma 1 the oracle's frame is the mean of n equal samples."""
    for frame in X.RESOLVE_FRAMES:
        for n in X.RESOLVE_SAMPLES:
            img, st = O.render(X.pixel_camera(), X.empty_scene(frame), X.resolve_params(1.0, n), 1)
            with np.errstate(all="ignore"):
                want = np.broadcast_to(X.mean_in_order(frame, n), img.shape)
            assert X.same_bits(img, want), (frame, n)
            assert st.camera_rays == 64 * n and st.segments == 0
            assert st.nan_pixels == X.nan_pixel_count(img)


def test_the_order_of_the_sum_shows():
    """The in-order f32 sum differs from the exact mean for some n, and from the chunked association for some n: a wrong order is visible."""
    exact = f32(X.SUM_BACKGROUND)
    differs = [n for n in X.SUM_COUNTS if not np.array_equal(X.mean_in_order(X.SUM_BACKGROUND, n), exact)]
    assert differs, "every in-order mean is exact: the test of the order would show nothing"
    apart = [n for n in X.SUM_COUNTS if not np.array_equal(X.mean_in_order(X.SUM_BACKGROUND, n), X.mean_chunk_sums(X.SUM_BACKGROUND, n))]
    assert apart, "the two associations agree everywhere"
    # ... and a reversed or pairwise sum would differ too at the large count
    b = np.full(1000, f32(0.1), f32)
    assert f32(np.sum(b)) / f32(1000) != X.mean_in_order((0.1,), 1000)[0]


@pytest.mark.parametrize("flags", [0, R.FLAG_CHUNK_SUMS])
def test_numpy_sums_are_the_oracles(flags):
    """The oracle adds in the order numpy's accumulate does, under both associations."""
    want_of = X.mean_chunk_sums if flags else X.mean_in_order
    for n in X.SUM_COUNTS:
        img, _ = O.render(X.pixel_camera(), X.empty_scene(X.SUM_BACKGROUND), X.sum_params(n, flags, 3, 2), 1)
        assert X.same_bits(img, np.broadcast_to(want_of(X.SUM_BACKGROUND, n), img.shape)), (flags, n)
