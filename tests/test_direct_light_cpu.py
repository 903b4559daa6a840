"""The direct-lighting rule on the host (rtw_light_samples / rtw_light_reduce, csrc/rtw_direct.h): its bits against a restatement of the
rule's text, the distribution of its samples, known answers derived by hand with the CPU oracle as the any-hit answer, the statuses, and --
with the oracle -- the proof that the point sets tests/test_gpu_direct_light.py runs exercise every outcome.  No GPU."""
import numpy as np
import pytest

import rtw_amd as R
from tests import ao_common as AO
from tests import direct_light_common as DL
from tests.test_gpu_scene_hits import geom_scene, oracle_hits

F = np.float32
E_INVALID = -1
RULE_LIGHTS = [(R.LIGHT_QUAD, 1), (R.LIGHT_SPHERE, 2)]               # of geom_scene(): AO.random_points lie about its objects


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule():
    """256 random points, and the rule's text at 1024 samples under two seeds (the whole stream of every item, computed once)."""
    p, n = AO.random_points(256, 1)
    scene = geom_scene()
    return scene, p, n, {seed: DL.rule_samples(scene, RULE_LIGHTS, p, n, 1024, seed) for seed in (0, 0xDEADBEEF)}


@pytest.mark.parametrize("samples", [1, 16, 1024])
def test_samples_equal_the_rule_bit_for_bit(rule, samples):
    scene, p, n, want = rule
    for seed in want:
        rays, w = R.light_samples(scene, RULE_LIGHTS, p, n, samples, seed)
        assert rays.shape == (256, 2, samples, 6) and w.shape == (256, 2, samples)
        # sample [i][l][k] does not depend on `samples`: the rule at 1024 samples holds every shorter stream as a prefix
        assert DL.same(rays, np.ascontiguousarray(want[seed][0][:, :, :samples])), (samples, seed)
        assert DL.same(w, np.ascontiguousarray(want[seed][1][:, :, :samples])), (samples, seed)
        cast = DL.cast_mask(rays)
        assert 0.1 < cast.mean() < 0.9, "the points do not exercise both outcomes of the cast rule"
        assert DL.same(rays[cast][:, :3], np.broadcast_to(p[:, None, None, :], rays.shape[:3] + (3,))[cast]), "the origin is the point as given"
        assert not rays[~cast].any() and not w[~cast].any() and not np.signbit(w[~cast]).any(), "a sample that is not cast writes zeros"
        assert (w[cast] >= 0.0).all() and np.isfinite(w).all()


def test_prefixes_agree_and_the_index_and_the_light_position_matter(rule):
    scene, p, n, want = rule
    a, wa = R.light_samples(scene, RULE_LIGHTS, p, n, 16, 0)
    b, _ = R.light_samples(scene, RULE_LIGHTS, p, n, 16, 0xDEADBEEF)
    both = DL.cast_mask(a) & DL.cast_mask(b)
    assert both.any() and not np.any(np.all(a[both][:, 3:] == b[both][:, 3:], axis=1)), "two seeds share a direction"
    assert DL.same(R.light_samples(scene, RULE_LIGHTS, p, n, 16, 2 ** 32 + 5)[0], R.light_samples(scene, RULE_LIGHTS, p, n, 16, 5)[0])
    for m in (1, 3, 64, 255):                                                            # sample [i][l][k] does not depend on n
        r, w = R.light_samples(scene, RULE_LIGHTS, p[:m], n[:m], 16, 0)
        assert DL.same(r, a[:m]) and DL.same(w, wa[:m]), m
    # ... nor on the number of lights: a longer list holds the shorter one's items
    three = RULE_LIGHTS + [(R.LIGHT_QUAD, 0)]
    r3, w3 = R.light_samples(scene, three, p, n, 16, 0)
    assert DL.same(np.ascontiguousarray(r3[:, :2]), a) and DL.same(np.ascontiguousarray(w3[:, :2]), wa)
    r1, w1 = R.light_samples(scene, RULE_LIGHTS[:1], p, n, 16, 0)
    assert DL.same(r1, np.ascontiguousarray(a[:, :1])) and DL.same(w1, np.ascontiguousarray(wa[:, :1]))
    assert DL.same(r3, DL.rule_samples(scene, three, p, n, 16, 0)[0])
    # ... but on i: the same point and normal at another index draws another stream
    moved, wm = R.light_samples(scene, RULE_LIGHTS, p[1:], n[1:], 16, 0)
    both = DL.cast_mask(moved) & DL.cast_mask(a[1:])
    assert both.any() and not np.any(np.all(moved[both][:, 3:] == a[1:][both][:, 3:], axis=1))
    want_m = DL.rule_samples(scene, RULE_LIGHTS, p[1:], n[1:], 16, 0)
    assert DL.same(moved, want_m[0]) and DL.same(wm, want_m[1])
    # ... and on l: the same light at another place of the list draws another stream
    swapped, ws = R.light_samples(scene, RULE_LIGHTS[::-1], p, n, 16, 0)
    both = DL.cast_mask(swapped[:, 1]) & DL.cast_mask(a[:, 0])
    assert both.any() and not np.any(np.all(swapped[:, 1][both][:, 3:] == a[:, 0][both][:, 3:], axis=1))
    want_s = DL.rule_samples(scene, RULE_LIGHTS[::-1], p, n, 16, 0)
    assert DL.same(swapped, want_s[0]) and DL.same(ws, want_s[1])


def test_samples_that_are_not_cast():
    scene = geom_scene()
    p, n = AO.random_points(8, 2)
    p[:, 1] = 1.0                                                                        # above the floor quad, light 0
    n[:] = [0.0, -1.0, 0.0]                                                              # ... and facing it
    n[0] = 0.0
    n[3] = [0.0, -0.0, 0.0]                                                              # (-0 == 0: not cast)
    n[5] = [0.0, np.nan, 0.0]                                                            # (a NaN fails the comparison)
    n[6] = [0.0, -1e-10, 0.0]                                                            # (tiny is not zero)
    n[7] = [0.0, 1.0, 0.0]                                                               # (faces away)
    p[4] = [np.nan, 1.0, 0.0]                                                            # (a NaN point: a NaN direction fails too)
    rays, w = R.light_samples(scene, RULE_LIGHTS[:1], p, n, 16, 0)
    for i in (0, 3, 4, 5, 7):
        assert DL.same(rays[i], np.zeros((1, 16, 6), F)) and DL.same(w[i], np.zeros((1, 16), F)), i
    for i in (1, 2, 6):
        assert DL.cast_mask(rays[i]).all() and (w[i] > 0.0).all() and np.isfinite(rays[i]).all(), i
    want = DL.rule_samples(scene, RULE_LIGHTS[:1], p, n, 16, 0)
    assert DL.same(rays, want[0]) and DL.same(w, want[1])


@pytest.mark.parametrize("samples", [1, 2, 64, 128, 1024])
def test_reduce_equals_the_association(samples):
    rng = np.random.default_rng(samples)
    w = (rng.uniform(0.0, 1.0, (32, samples)) ** 8).astype(F)                            # a wide range of magnitudes
    w[1, ::3] = 0.0
    w[2] = 0.0
    got = R.light_reduce(w)
    want = np.array([DL.rule_reduce(row) for row in w], F)
    assert got.shape == (32,) and DL.same(got, want)
    if samples >= 64:
        left = np.zeros(32, F)
        for k in range(samples):
            left = (left + w[:, k]).astype(F)
        left = (left * (F(1.0) / F(samples))).astype(F)
        assert np.any(got != left), "the association cannot be told from a left-to-right sum on this input"
    assert R.light_reduce(np.ones(samples, F)) == 1.0 and R.light_reduce(np.ones((2, 3, samples), F)).shape == (2, 3)


# ---- the distribution -----------------------------------------------------------------------------------------------------------------------
N_DIST = 65536                                                                           # 64 items of 1024 samples


def dist_samples(sphere=None, quad=None, p=(0.0, 0.0, 0.0), n=(0.0, 1.0, 0.0)):
    """(scene, rays [65536][6], weights) of one light seen from 64 copies of one point: 64 streams of 1024 samples."""
    scene = R.Scene([sphere] if sphere else (), quads=[quad] if quad else ())
    light = [(R.LIGHT_SPHERE, 0)] if sphere else [(R.LIGHT_QUAD, 0)]
    rays, w = R.light_samples(scene, light, np.tile(np.array(p, F), (64, 1)), np.tile(np.array(n, F), (64, 1)), 1024, 9)
    return scene, rays.reshape(N_DIST, 6), w.reshape(64, 1024)


def test_quad_samples_lie_in_the_quad_uniformly():
    o, u, v = np.array([-0.5, 2.0, -0.75]), np.array([1.5, 0.0, 0.5]), np.array([0.25, 0.5, 1.0])
    _, rays, _ = dist_samples(quad=R.Quad.new(tuple(o), tuple(u), tuple(v)))              # (the point is the origin: y is the direction itself)
    assert DL.cast_mask(rays).all()
    y = rays[:, 3:].astype(np.float64) - o
    st, res, _, _ = np.linalg.lstsq(np.stack([u, v], 1), y.T, rcond=None)
    s, t = st
    assert np.abs(y.T - np.stack([u, v], 1) @ st).max() <= 1e-6, "a sample leaves the quad's plane"
    assert s.min() >= -1e-6 and s.max() <= 1.0 and t.min() >= -1e-6 and t.max() <= 1.0, (s.min(), s.max(), t.min(), t.max())
    sigma = np.sqrt(1.0 / 12.0) / np.sqrt(N_DIST)
    assert abs(s.mean() - 0.5) <= 4 * sigma and abs(t.mean() - 0.5) <= 4 * sigma, (s.mean(), t.mean(), sigma)


def test_sphere_samples_lie_on_the_facing_hemisphere():
    c, r = np.array([0.5, 0.75, -0.5]), 1.0
    _, rays, _ = dist_samples(sphere=R.Sphere.new(tuple(c), r, (1.0, 1.0, 1.0), R.SCATTER_M), n=tuple(c))
    assert DL.cast_mask(rays).all()
    y = rays[:, 3:].astype(np.float64)                                                   # (the point is the origin)
    dist = np.linalg.norm(y - c, axis=1)
    assert np.abs(dist - r).max() <= 4e-7 * r, np.abs(dist - r).max()
    assert ((y - c) @ (0.0 - c) >= -1e-6).all(), "a sample lies on the far hemisphere"
    # uniform over the hemisphere's area: the component along the axis towards the point is uniform in [0, r]
    h = (y - c) @ (0.0 - c) / np.linalg.norm(c)
    assert abs(h.mean() - 0.5 * r) <= 4 * r * np.sqrt(1.0 / 12.0) / np.sqrt(N_DIST)


# ---- known answers: derived, the oracle is the any-hit answer ---------------------------------------------------------------------------------
def host_outputs(O, scene, rays, w, samples):
    cast = DL.cast_mask(rays)
    occ = np.zeros(cast.shape, bool)
    if cast.any():
        occ[cast] = oracle_hits(O, scene, rays[cast], 0.0, DL.LO, DL.HI)[1] >= 0
    return DL.outputs(w, cast, occ, samples) + (cast,)


def test_a_point_facing_an_unoccluded_quad_light(oracle):
    o, u, v = np.array([-0.5, 2.0, -0.75]), np.array([1.5, 0.0, 0.5]), np.array([0.25, 0.5, 1.0])
    nrm = np.array([0.0, 1.0, 0.0])
    scene, rays, w = dist_samples(quad=R.Quad.new(tuple(o), tuple(u), tuple(v)), n=tuple(nrm))
    vis, irr, _, cast = host_outputs(oracle, scene, rays.reshape(64, 1, 1024, 6), w.reshape(64, 1, 1024), 1024)
    assert cast.all() and (vis == 1.0).all()
    # the same integrand by the midpoint rule in float64: G = (n . d) |g . d| / (d . d)^2 over the unit square of the two parameters
    m = (np.arange(512) + 0.5) / 512
    S, T = np.meshgrid(m, m, indexing="ij")
    d = o[None, None, :] + S[..., None] * u + T[..., None] * v
    g = np.cross(u, v)
    want = np.mean((d @ nrm) * np.abs(d @ g) / np.sum(d * d, axis=-1) ** 2)
    se = w.astype(np.float64).std(ddof=1) / np.sqrt(N_DIST)
    got = irr.astype(np.float64).mean()
    print(f"\n[direct] quad: irr {got:.6f}, quadrature {want:.6f}, standard error {se:.2e}")
    assert abs(got - want) <= 4 * se, (got, want, se)


def test_a_point_below_an_unoccluded_sphere_light(oracle):
    r, D = 0.5, 2.0
    c = np.array([0.25, D, -0.5])
    p = c - [0.0, D, 0.0]
    scene, rays, w = dist_samples(sphere=R.Sphere.new(tuple(c), r, (1.0, 1.0, 1.0), R.SCATTER_M), p=tuple(p), n=(0.0, 1.0, 0.0))
    vis, irr, v, cast = host_outputs(oracle, scene, rays.reshape(64, 1, 1024, 6), w.reshape(64, 1, 1024), 1024)
    assert cast.all()
    # the light hides its own facing hemisphere beyond the horizon: those samples weigh 0 and its near side blocks them
    want = np.pi * r * r / (D * D)                                                       # a sphere of unit radiance: pi sin^2 of its half angle
    masked = irr.astype(np.float64).mean()
    se = w.astype(np.float64).std(ddof=1) / np.sqrt(N_DIST)
    print(f"\n[direct] sphere: irr {masked:.6f}, pi r^2 / D^2 {want:.6f}, standard error {se:.2e}, vis {vis.mean():.4f}, cap {1 - r / D:.4f}")
    assert abs(masked - want) <= 4 * se, (masked, want, se)
    q = 1.0 - r / D                                                                      # the visible cap's share of the hemisphere's area
    share = v.sum() / N_DIST
    sigma = np.sqrt(q * (1.0 - q) / N_DIST)
    assert q - 4 * sigma <= share <= q + 4 * sigma, (share, q, sigma)
    assert np.mean(w > 0.0) <= q + 4 * sigma, "a sample beyond the horizon weighs something"


def test_a_normal_that_faces_away_and_a_wall_in_between(oracle):
    light = R.Quad.new((-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    wall = R.Quad.new((-5.0, 1.0, -5.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0))
    scene = R.Scene((), quads=[light, wall])
    p = np.zeros((2, 3), F)
    n = np.array([[0.0, -1.0, 0.0], [0.0, 1.0, 0.0]], F)
    rays, w = R.light_samples(scene, [(R.LIGHT_QUAD, 0)], p, n, 64, 0)
    vis, irr, _, cast = host_outputs(oracle, scene, rays, w, 64)
    assert not cast[0].any() and not rays[0].any() and vis[0, 0] == 0.0 and irr[0, 0] == 0.0, "the normal faces away: no ray is cast"
    assert cast[1].all() and (w[1] > 0.0).all() and vis[1, 0] == 0.0 and irr[1, 0] == 0.0, "the wall stops every ray"
    clear = R.Scene((), quads=[light])
    vis, irr, _, _ = host_outputs(oracle, clear, rays, w, 64)
    assert vis[1, 0] == 1.0 and irr[1, 0] > 0.0


# ---- the GPU tests' inputs exercise every outcome (the CPU oracle) -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "geom"])
def test_the_point_sets_exercise_every_outcome(oracle, name):
    p, n = DL.points_of(oracle, name)
    vis, irr, v, cast = DL.reference(oracle, name)
    S = DL.SAMPLES
    blocked = (cast.sum() - v.sum()) / cast.sum()
    partly, full = int(((v > 0) & (v < S)).sum()), int((v == S).sum())
    some, none = int(((cast > 0) & (cast < S)).sum()), int((cast == 0).sum())
    print(f"\n[direct] {name}: {len(p)} points x {vis.shape[1]} lights: {blocked:.1%} of the cast rays blocked, {partly} items partly visible, "
          f"{full} fully, {some} with some samples cast, {none} with none")
    assert 0.1 <= blocked <= 0.9
    assert partly >= 30 and full >= 10 and some >= 10 and none >= 10
    assert np.isfinite(p).all() and np.isfinite(irr).all() and (irr[v == 0] == 0.0).all() and (irr[v > 0] > 0.0).any()


def test_the_moving_point_set(oracle):
    """forty_spheres() at TIME (the MOVING build): both outcomes, partly visible items."""
    _, _, v, cast = DL.reference(oracle, "forty")
    assert 0.1 <= (cast.sum() - v.sum()) / cast.sum() <= 0.9 and ((v > 0) & (v < DL.SAMPLES)).sum() >= 20


# ---- statuses -----------------------------------------------------------------------------------------------------------------------------------
def test_statuses_of_the_host_forms():
    import ctypes as C
    L = R.lib()
    scene = geom_scene()
    p, n = AO.random_points(8, 2)
    arr, nl = R._light_array(RULE_LIGHTS)
    rays, w = np.full((8, 2, 16, 6), 7.0, F), np.full((8, 2, 16), 7.0, F)
    sc, pp, nn, rr, ww = C.byref(scene.pod), p.ctypes.data, n.ctypes.data, rays.ctypes.data, w.ctypes.data

    def call(scene_=sc, lights=arr, n_lights=nl, points=pp, normals=nn, count=8, samples=16, r_out=rr, w_out=ww):
        return L.rtw_light_samples(scene_, lights, n_lights, points, normals, count, samples, 0, r_out, w_out)

    bad_kind, _ = R._light_array([(2, 0), RULE_LIGHTS[1]])
    bad_sphere, _ = R._light_array([RULE_LIGHTS[0], (R.LIGHT_SPHERE, scene.n_spheres)])
    bad_quad, _ = R._light_array([(R.LIGHT_QUAD, scene.n_quads)])
    many, _ = R._light_array([RULE_LIGHTS[0]] * 17)
    for what, rc in (("scene", call(scene_=None)), ("lights", call(lights=None)), ("no lights", call(lights=None, n_lights=0)),
                     ("n_lights 0", call(n_lights=0)), ("17 lights", call(lights=many, n_lights=17)), ("kind", call(lights=bad_kind)),
                     ("sphere index", call(lights=bad_sphere)), ("quad index", call(lights=bad_quad, n_lights=1)),
                     ("points", call(points=None)), ("normals", call(normals=None)), ("n", call(count=0)), ("rays_out", call(r_out=None)),
                     ("weight_out", call(w_out=None)), ("samples 0", call(samples=0)), ("samples 3", call(samples=3)),
                     ("samples 2048", call(samples=2048))):
        assert rc == E_INVALID, what
    assert (rays == 7.0).all() and (w == 7.0).all(), "a refused call wrote"
    for samples in (0, 3, 2048):
        with pytest.raises(R.RtwError):
            R.light_samples(scene, RULE_LIGHTS, p, n, samples)
    with pytest.raises(R.RtwError):
        R.light_samples(scene, [], p, n, 16)
    assert call() == R.RTW_OK
    want = R.light_samples(scene, RULE_LIGHTS, p, n, 16, 0)
    assert DL.same(rays, want[0]) and DL.same(w, want[1])
    out = np.full(2, 7.0, F)
    ones = np.ones(16, F)
    for what, rc in (("weights", L.rtw_light_reduce(None, 16, out.ctypes.data)), ("out", L.rtw_light_reduce(ones.ctypes.data, 16, None)),
                     ("samples 0", L.rtw_light_reduce(ones.ctypes.data, 0, out.ctypes.data)),
                     ("samples 12", L.rtw_light_reduce(ones.ctypes.data, 12, out.ctypes.data)),
                     ("samples 2048", L.rtw_light_reduce(ones.ctypes.data, 2048, out.ctypes.data))):
        assert rc == E_INVALID, what
    assert (out == 7.0).all()
    assert L.rtw_light_reduce(ones.ctypes.data, 16, out.ctypes.data) == R.RTW_OK and out[0] == 1.0 and out[1] == 7.0
    with pytest.raises(R.RtwError):
        R.light_reduce(np.ones(12, F))
    assert L.rtw_ctx_light_count(None) == 0
