"""The ambient-occlusion sampling rule on the host (rtw_ao_rays, csrc/rtw_ao.h): its bits against a restatement of the rule's text, its
distribution against the cosine lobe's moments, known answers through the host any-hit form, and -- with the CPU oracle -- the proof that
the point sets tests/test_gpu_ao.py runs exercise every outcome.  No GPU."""
import numpy as np
import pytest

import rtw_amd as R
from tests import ao_common as AO
from tests import refit_common as RC

F = np.float32
E_INVALID = -1


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule():
    """256 random points, and the rule's text at 1024 samples under two seeds (the whole stream of every point, computed once)."""
    p, n = AO.random_points(256, 1)
    return p, n, {seed: AO.rule_rays(p, n, 1024, seed) for seed in (0, 0xDEADBEEF)}


@pytest.mark.parametrize("samples", [1, 16, 1024])
def test_rays_equal_the_rule_bit_for_bit(rule, samples):
    p, n, want = rule
    for seed in want:
        got = R.ao_rays(p, n, samples, seed)
        assert got.shape == (256, samples, 6)
        # ray [i][k] does not depend on `samples`: the rule at 1024 samples holds every shorter stream as a prefix
        assert AO.same(got, np.ascontiguousarray(want[seed][:, :samples])), (samples, seed)
        assert AO.same(got[:, :, :3], np.repeat(p[:, None, :], samples, 1)), "the origin is the point as given"


def test_seeds_differ_and_prefixes_agree(rule):
    p, n, want = rule
    a, b = R.ao_rays(p, n, 16, 0), R.ao_rays(p, n, 16, 0xDEADBEEF)
    assert not np.any(np.all(a[:, :, 3:] == b[:, :, 3:], axis=2)), "two seeds share a direction"
    assert AO.same(R.ao_rays(p, n, 16, 2 ** 32 + 5), R.ao_rays(p, n, 16, 5))             # (the seed is 32 bits)
    for m in (1, 3, 64, 255):                                                            # ray [i][k] does not depend on n
        assert AO.same(R.ao_rays(p[:m], n[:m], 16, 0), a[:m]), m
    # ... but on i: the same point and normal at another index draws another stream
    moved = R.ao_rays(p[1:], n[1:], 16, 0)
    assert not np.any(np.all(moved[:, :, 3:] == a[1:, :, 3:], axis=2))
    assert AO.same(moved, AO.rule_rays(p[1:], n[1:], 16, 0))


def test_skipped_points_and_statuses():
    p, n = AO.random_points(8, 2)
    n[0] = 0.0
    n[3] = [0.0, -0.0, 0.0]                                                              # (-0 == 0: skipped)
    n[5] = [0.0, np.nan, 0.0]                                                            # (a NaN is not zero: it flows)
    n[6] = [0.0, 0.0, 1e-10]                                                             # (tiny is not zero either)
    rays = R.ao_rays(p, n, 16, 0)
    assert not rays[0].any() and not rays[3].any() and AO.same(rays[0], np.zeros((16, 6), F))
    assert np.isnan(rays[5, :, 3:]).all() and AO.same(rays[5, :, :3], np.repeat(p[5:6], 16, 0))
    assert np.isfinite(rays[6]).all() and rays[6, :, 3:].any()
    assert AO.same(rays, AO.rule_rays(p, n, 16, 0))
    L = R.lib()
    out = np.full((8, 16, 6), 7.0, F)
    pp, nn, oo = p.ctypes.data, n.ctypes.data, out.ctypes.data
    assert L.rtw_ao_rays(None, nn, 8, 16, 0, oo) == E_INVALID
    assert L.rtw_ao_rays(pp, None, 8, 16, 0, oo) == E_INVALID
    assert L.rtw_ao_rays(pp, nn, 8, 16, 0, None) == E_INVALID
    assert L.rtw_ao_rays(pp, nn, 0, 16, 0, oo) == E_INVALID
    for samples in (0, 3, 2048):
        assert L.rtw_ao_rays(pp, nn, 8, samples, 0, oo) == E_INVALID, samples
        with pytest.raises(R.RtwError):
            R.ao_rays(p, n, samples)
    assert (out == 7.0).all(), "a refused call wrote"
    assert L.rtw_ao_rays(pp, nn, 8, 16, 0, oo) == R.RTW_OK and AO.same(out, rays)


# ---- the distribution -----------------------------------------------------------------------------------------------------------------------
# Cosine-weighted about w = unit(n): pdf(theta) = 2 cos sin, so E[cos] = 2/3 and E[cos^2] = 1/2, Var[cos] = 1/2 - 4/9 = 1/18; the azimuth is
# uniform, so a component along any tangent is positive with probability 1/2 (a Bernoulli share: sigma = 0.5 / sqrt(N)).  N = 65 536 rays:
# 64 points with the one normal at 1024 samples.  |dir| = 1 to a few roundings of three unit vectors and a sqrt: 4e-7 is 3.4 ulp of 1.
NORMALS = {"+x": (1.0, 0.0, 0.0), "-y": (0.0, -1.0, 0.0), "+z": (0.0, 0.0, 1.0), "|w.x| > 0.9": (-0.95, 0.2, -0.1),
           "oblique": (0.3, -0.5, 0.8), "non-unit": (30.0, 40.0, -120.0)}


@pytest.mark.parametrize("which", list(NORMALS))
def test_directions_follow_the_cosine_lobe(which):
    n = np.array(NORMALS[which], np.float64)
    w = n / np.linalg.norm(n)
    assert (abs(w[0]) > 0.9) == (which in ("+x", "|w.x| > 0.9")), "the case does not take the ONB branch it names"
    N = 65536
    rays = R.ao_rays(np.zeros((64, 3), F), np.tile(n.astype(F), (64, 1)), 1024, 9).reshape(N, 6)
    d = rays[:, 3:].astype(np.float64)
    cos = d @ w
    assert cos.min() >= -1e-6, cos.min()
    sigma = np.sqrt(1.0 / 18.0) / np.sqrt(N)
    assert abs(cos.mean() - 2.0 / 3.0) <= 4 * sigma, (cos.mean(), sigma)
    for axis in np.eye(3):
        t = np.cross(w, axis)
        if np.linalg.norm(t) < 0.5:
            continue
        share = float(np.mean(d @ t > 0.0))
        assert abs(share - 0.5) <= 4 * 0.5 / np.sqrt(N), (axis, share)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 4e-7


# ---- known answers on the host ----------------------------------------------------------------------------------------------------------------
def test_known_answers_inside_an_icosphere():
    v, f, _, _ = RC.mesh("icosphere2")                                 # radius 1 about the origin: every face lies between its inradius and 1
    tris = RC.triangles_of(v, f)
    v = np.asarray(v, np.float64)
    inradius = min(abs(np.dot(np.cross(v[b] - v[a], v[c] - v[a]) / np.linalg.norm(np.cross(v[b] - v[a], v[c] - v[a])), v[a])) for a, b, c in f)
    assert 0.9 < inradius < 1.0
    p = np.zeros((4, 3), F)
    n = np.array([[0, 1, 0], [1, 0, 0], [0, 0, -1], [0.5, 0.5, 0.7]], F)
    rays = R.ao_rays(p, n, 64, 3).reshape(-1, 6)
    occ, _ = R.triangle_occluded(tris, rays, 1e-3, 1.5)                # beyond the radius: every ray from the centre meets the shell
    assert occ.all()
    occ, _ = R.triangle_occluded(tris, rays, 1e-3, float(inradius) * 0.99)          # below the inradius: none does
    assert not occ.any()


# ---- the GPU tests' inputs exercise every outcome (the CPU oracle) -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["geom", "field"])
def test_the_point_sets_exercise_every_outcome(oracle, name):
    p, n = AO.points_of(oracle, name)
    counts, ao = AO.reference(oracle, name)
    share = counts.sum() / (len(p) * AO.SAMPLES)
    partly, free = int(((counts > 0) & (counts < AO.SAMPLES)).sum()), int((counts == 0).sum())
    print(f"\n[ao] {name}: {len(p)} points, radius {AO.RADIUS[name]}: {share:.1%} of the AO rays occluded, {partly} points partly, {free} not at all")
    assert 0.2 <= share <= 0.8
    assert partly >= 50 and free >= 20
    assert not AO.skipped(n).any() and np.isfinite(p).all()
    assert ao.min() >= 0.0 and ao.max() == 1.0 and len(np.unique(ao)) >= 8


def test_the_moving_point_set(oracle):
    """forty_spheres() at TIME (the MOVING build): both outcomes, many partly occluded points."""
    counts, _ = AO.reference(oracle, "forty")
    assert 0.2 <= counts.mean() / AO.SAMPLES <= 0.8 and ((counts > 0) & (counts < AO.SAMPLES)).sum() >= 50
