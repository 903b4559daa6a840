"""The inputs of tests/test_gpu_any_hit_edges.py reach the edges they are named for: proved here with the CPU oracle and the host forms
(rtw_ao_rays, rtw_light_samples, rtw_light_reduce).  Each condition below is what makes the GPU assertion of the same name bite; a set that
stops reaching its edge fails here, on a machine without a GPU."""
import numpy as np
import pytest

import rtw_amd as R
from tests import any_hit_edges_common as AE
from tests import ao_common as AO
from tests import direct_light_common as DL
from tests import query_edges_common as QE
from tests.test_gpu_scene_hits import MAXT, MINT, depth_camera, oracle_hits

F = np.float32


# ---- 1. seeds ---------------------------------------------------------------------------------------------------------------------------------
def test_the_seeds_give_other_answers_and_seed_0_the_committed_ones(oracle):
    assert (0x61C88647 + 0x9E3779B9) & 0xFFFFFFFF == 0, "the fourth seed is the one whose first hash input wraps to 0"
    for samples, n in AE.POINTS_AT.items():
        for name in ("field", "forty"):
            answers = [AE.ao_oracle(oracle, name, n, samples, seed)[0] for seed in (0,) + AE.SEEDS]
            for a in range(len(answers)):
                for b in range(a):
                    assert np.any(answers[a] != answers[b]), (name, samples, "two seeds give one answer: a seed ignored on both sides would pass")
        for name in ("golden", "forty"):
            answers = [AE.dl_oracle(oracle, name, n, samples, seed)[:2] for seed in (0,) + AE.SEEDS]
            for a in range(len(answers)):
                for b in range(a):
                    assert np.any(answers[a][0] != answers[b][0]) and np.any(answers[a][1] != answers[b][1]), (name, samples)
    for name in ("field", "forty"):
        assert np.array_equal(AE.ao_oracle(oracle, name, 257, 16)[0], AO.reference(oracle, name)[0][:257])
    for name in ("golden", "forty"):
        assert DL.same(AE.dl_oracle(oracle, name, 257, 16)[0], np.ascontiguousarray(DL.reference(oracle, name)[0][:257]))
        assert DL.same(AE.dl_oracle(oracle, name, 257, 16)[1], np.ascontiguousarray(DL.reference(oracle, name)[1][:257]))


def test_the_host_forms_read_32_bits_of_the_seed(oracle):
    scene, lights, _, _, p, n = AE.dl_set(oracle, "golden")
    assert AO.same(R.ao_rays(p[:9], n[:9], 16, 2 ** 32 + 5), R.ao_rays(p[:9], n[:9], 16, 5))
    assert DL.same(R.light_samples(scene, lights, p[:9], n[:9], 16, 2 ** 32 + 5)[0], R.light_samples(scene, lights, p[:9], n[:9], 16, 5)[0])
    assert not AO.same(R.ao_rays(p[:9], n[:9], 16, 0x61C88647), R.ao_rays(p[:9], n[:9], 16, 0))


@pytest.mark.parametrize("samples,width,height", AE.MAP_SIZES)
def test_the_camera_forms_points_tell_seeds_and_ranges_apart(oracle, samples, width, height):
    scene, lights = AO.case("geom")[0], DL.GEOM_LIGHTS
    p, faced, hit = AE.map_points_by_the_oracle(oracle, scene, depth_camera("geom", width, height), width, height, 0.0, MINT, MAXT)
    assert 8 <= hit.sum() < len(hit)
    (lo, hi), skip = AE.MAP_RANGE, AO.skipped(faced)

    def ao(seed, mint, radius):
        rays = R.ao_rays(p, faced, samples, seed)
        return (oracle_hits(oracle, scene, np.ascontiguousarray(rays[~skip]).reshape(-1, 6), 0.0, mint, radius)[1] >= 0).reshape(-1, samples).sum(axis=1)

    aos = [ao(seed, AO.AO_MINT, 5.0) for seed in (0,) + AE.SEEDS] + [ao(1, lo, AE.MAP_RADIUS)]
    viss = [AE.dl_answer(oracle, scene, lights, p, faced, samples, seed, 0.0, DL.LO, DL.HI)[0] for seed in (0,) + AE.SEEDS]
    viss.append(AE.dl_answer(oracle, scene, lights, p, faced, samples, 1, 0.0, lo, hi)[0])
    for a in range(len(aos)):
        for b in range(a):
            assert np.any(aos[a] != aos[b]) and np.any(viss[a] != viss[b]), (a, b)


# ---- 2. ranges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 0x61C88647, 0xFFFFFFFF])
def test_the_flat_scene_turns_at_one_half_exactly(oracle, seed):
    scene, lights, _, _, p, n = AE.dl_set(oracle, "flat")
    rays, _ = R.light_samples(scene, lights, p, n, 16, seed)
    assert DL.cast_mask(rays).all() and (rays[..., 4] == F(2.0)).all() and (rays[..., 1] == 0.0).all(), "d.y is not 2.0f exactly"
    occluded = {what: int(AE.dl_oracle(oracle, "flat", 64, 16, seed, None, *rng)[4].sum()) for what, rng in AE.FLAT_RANGES.items()}
    print(f"\n[edges] flat, seed {seed:#x}: occluded of 1024: {occluded}")
    for what in AE.FLAT_CLOSED:
        assert occluded[what] >= 256, (what, "at a closed edge at least a quarter of the segments are occluded")
    for what in AE.FLAT_OPEN:
        assert occluded[what] == 0, (what, "one ulp outside, none is")
    assert occluded["lo = 0"] == occluded["lo = -1"] == occluded["hi at the blocker"]
    assert occluded["hi = 1"] == 1024, "at hi = 1 the light's own plane (t == 1 exactly) stops every segment"


def test_the_range_takes_the_sphere_lights_own_surface_in(oracle):
    v = [AE.dl_oracle(oracle, "surface", 257, 16, 0, None, DL.LO, hi)[2] for hi in AE.SURFACE_HI]
    lit = v[0] > 0
    fell = (v[2] < v[0]) & lit
    print(f"\n[edges] surface: lit items {int(lit.sum())}, visible segments at hi = 1 - 1e-3 / 1 / 1 + 1e-3: {[int(x.sum()) for x in v]}")
    assert lit.sum() >= 50 and fell.sum() * 2 >= lit.sum()
    # (with its surface in range the light stops every segment to it but one that grazes it: a sample on the horizon, where the rounded
    # discriminant may be negative)
    assert v[0].sum() > v[1].sum() > v[2].sum() and 100 * v[2].sum() <= v[0].sum(), "at hi = 1 the rounding of each root decides"


@pytest.mark.parametrize("name", ["field", "forty"])
def test_the_ao_edge_rays_have_one_hit_and_the_edges_turn_it(oracle, name):
    scene, _, time, p, n, radius = AE.ao_set(oracle, name)
    edges = AE.ao_edge_reference(oracle, name)
    assert len(edges) == AE.AO_EDGE_RAYS
    rays = R.ao_rays(p[:AE.AO_EDGE_POINTS], n[:AE.AO_EDGE_POINTS], 16, 0)
    flips = 0
    for i, k, t, cases in edges:
        got_t, idx, _ = oracle_hits(oracle, scene, rays[i, k][None, :], time, AO.AO_MINT, radius)
        assert idx[0] >= 0 and float(got_t[0]) == t
        assert oracle_hits(oracle, scene, rays[i, k][None, :], time, QE.above(t), 1e30)[1][0] < 0, "something lies behind the hit"
        (_, _, at_hi, c_hi), (_, _, below_hi, c_below), (_, _, at_lo, c_lo), (_, _, above_lo, c_above) = cases
        turned = at_hi and not below_hi and at_lo and not above_lo
        flips += turned
        if turned:
            assert c_hi - c_below == 1 and c_lo - c_above == 1, "the point's count moves by more than the chosen ray"
    assert 2 * flips >= len(edges), (name, flips)


def test_the_ao_range_classes(oracle):
    for name in ("field", "forty"):
        assert not AE.ao_oracle(oracle, name, 65, 16, 0, None, 1.0, 0.5)[0].any(), "mint > radius occludes"
        free, far = AE.ao_oracle(oracle, name, 65, 16)[0], AE.ao_oracle(oracle, name, 65, 16, 0, None, AO.AO_MINT, QE.INF)[0]
        assert far.sum() > free.sum(), "an unbounded radius finds nothing more"
        assert np.array_equal(far, AE.ao_oracle(oracle, name, 65, 16, 0, None, AO.AO_MINT, 1e30)[0])
    for cls, (mint, maxt) in QE.RANGES.items():
        counts = AE.ao_oracle(oracle, "field", 129, 16, 0, None, mint, maxt)[0]
        assert 0 < counts.sum() < 16 * 129, cls


# ---- 3. time ----------------------------------------------------------------------------------------------------------------------------------
def test_the_time_outside_the_shutter_changes_the_answers(oracle):
    n = AE.FALLBACK_POINTS
    inside = AE.ao_oracle(oracle, "forty", n, 16)[0]
    for tm in (-0.5, 1.5, 0.0, 1.0):
        assert np.any(AE.ao_oracle(oracle, "forty", n, 16, 0, tm)[0] != inside), tm
    inside = AE.dl_oracle(oracle, "moving 38+9", n, 16)[2]
    for tm in (-0.5, 1.5, 0.0, 1.0):
        assert np.any(AE.dl_oracle(oracle, "moving 38+9", n, 16, 0, tm)[2] != inside), tm


# ---- 4. a light that moves --------------------------------------------------------------------------------------------------------------------
def test_a_moving_light_is_sampled_where_it_stood_and_met_where_it_stands(oracle):
    changed = {}
    for key in ("5", "1", "9"):
        scene, lights, _, _, p, n = AE.dl_set(oracle, "moving " + key)
        sphere = scene._spheres[lights[0][1]]
        assert any(float(x) != 0.0 for x in sphere.velocity), key
        a, b = (AE.dl_oracle(oracle, "moving " + key, AE.MOVING_POINTS, 16, 0, tm) for tm in (0.0, 1.0))
        assert np.array_equal(a[3], b[3]), "the rule reads the centre at time 0: the cast segments do not depend on the time"
        changed[key] = (int((a[4] != b[4]).sum()), int(a[3].sum()))
    print(f"\n[edges] moving lights: segments whose answer differs between time 0 and time 1, of the cast ones: {changed}")
    assert changed["5"][0] >= 8 and changed["5"][1] >= 1000
    assert changed["1"][0] >= 1 and changed["9"][0] >= 1


# ---- 5. geometry at the edges -----------------------------------------------------------------------------------------------------------------
def spoiler_rays(kind):
    scene = AE.edge_scene()[0]
    lights, p, n = AE.spoiled(kind)
    rays, w = R.light_samples(scene, lights, p, n, 16, 0)
    return scene, lights, rays[AE.SPOILED], w[AE.SPOILED]


def test_the_spoilers_leave_the_plain_range_of_d_dot_d():
    scene, lights, rays, w = spoiler_rays("a far light")
    cast = DL.cast_mask(rays)
    assert cast.all(), "a far spoiler casts every sample"
    assert (QE.dd_of(rays[cast]) > F(2.0 ** 20)).all() and not QE.a_plain(rays[cast]).any()
    assert QE.q_ordinary(rays[cast], QE.scene_span(scene)).all(), "... and stays a ray the tree serves"
    scene, lights, rays, w = spoiler_rays("a tiny near light")
    cast = DL.cast_mask(rays[:, 2])
    assert cast.all() and (QE.dd_of(rays[:, 2][cast]) < F(2.0 ** -20)).all() and not QE.a_plain(rays[:, 2][cast]).any()
    assert QE.a_plain(rays[:, :2][DL.cast_mask(rays[:, :2])]).all(), "its other lights are ordinary"
    assert QE.q_ordinary(rays[:, 2][cast], QE.scene_span(scene)).all()
    p, n = AE.edge_points()
    plain, _ = R.light_samples(scene, lights, p, n, 16, 0)
    cast = DL.cast_mask(plain)
    assert cast.mean() > 0.3 and QE.a_plain(plain[cast]).all(), "an unspoiled wave takes sphere_root's plain sequence"


def test_the_spoilers_weights():
    _, _, rays, w = spoiler_rays("in the plane of the quad light")
    assert DL.cast_mask(rays[:, 0]).all() and (rays[:, 0, :, 4] == 0.0).all() and (w[:, 0] == 0.0).all(), "g.d == 0: the weight is a zero"
    _, _, rays, w = spoiler_rays("inside the sphere light")
    cast = DL.cast_mask(rays[:, 1])
    assert 0.1 < cast.mean() < 1.0 and np.isfinite(w[:, 1]).all()
    assert (np.linalg.norm(rays[:, 1][cast][:, 3:].astype(np.float64), axis=1) < 2.0 * AE.BULB[1]).all()
    scene, _, rays, w = spoiler_rays("so far that dd * dd overflows")
    cast = DL.cast_mask(rays)
    with np.errstate(over="ignore"):
        dd = QE.dd_of(rays[cast])
        assert cast.all() and np.isinf((dd * dd).astype(F)).all() and (w == 0.0).all() and not np.signbit(w).any()
    assert not QE.q_ordinary(rays[cast], QE.scene_span(scene)).any(), "such a ray walks the list"
    _, _, rays, w = spoiler_rays("so near that dd * dd underflows")
    cast = DL.cast_mask(rays[:, 2])
    dd = QE.dd_of(rays[:, 2][cast])
    assert cast.all() and (dd > 0.0).all() and ((dd * dd).astype(F) == 0.0).all() and not np.isfinite(w[:, 2]).any()
    irr = R.light_reduce(w[:, 2])
    assert np.isnan(irr).all() or np.isinf(irr).all(), "x / 0: the item's host answer is not a number the sum could hide"


def test_the_unspoiled_edge_launch_exercises_both_outcomes(oracle):
    for which in (0, 1):
        vis, irr, v, cast, _ = AE.edge_oracle(oracle, which)
        assert 0.1 < (cast.sum() - v.sum()) / cast.sum() < 0.9 and ((v > 0) & (v < 16)).sum() >= 20
        assert np.isfinite(irr).all() and irr.max() > 0.0
    assert len(np.unique((3 * AE.SPOILED + 2) % 4)) == 4 and len(np.unique((3 * AE.SPOILED + 2) // 4)) == len(AE.SPOILED)


def test_a_degenerate_light_at_the_point_casts_nothing(oracle):
    """u == v == 0 and the point at the quad's origin corner: d == 0, so dot(n, d) > 0 fails and no sample is cast -- the rule never hands
    the walk a zero direction.  The constructors refuse nothing: the setters' behaviour is the GPU module's to find out.  As an occluder
    such a quad stops every ray: its plane is NaN, and a NaN passes every comparison of the reference's quad test."""
    scene, lights = AE.degenerate_scene()
    q, m = AE.edge_points()
    assert not AE.dl_answer(oracle, scene, lights, q, m, 16, 0, 0.0, DL.LO, DL.HI)[2].any()
    p = np.array([[1.0, 0.25, -1.0], [1.0, 0.0, -1.0]], F)
    n = np.tile(AE.UP, (2, 1))
    rays, w = R.light_samples(scene, lights, p, n, 16, 0)
    assert not DL.cast_mask(rays[0, 2]).any() and not w[0, 2].any(), "d == 0 is cast"
    assert DL.cast_mask(rays[1, 2]).all() and (rays[1, 2, :, 3:] == F([0.0, 0.25, 0.0])).all(), "from below every sample is the corner itself"
    assert np.isnan(w[1, 2]).all() or (w[1, 2] == 0.0).all()


# ---- 6. the sum's association -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", AE.ASSOC_SAMPLES)
def test_the_corner_points_weights_tell_the_associations_apart(oracle, samples):
    scene, lights, _, _, p, n = AE.dl_set(oracle, "corner")
    _, w = R.light_samples(scene, lights, p, n, samples, 0)
    vis, irr, v, cast, occ = AE.dl_oracle(oracle, "corner", len(p), samples)
    masked = np.where(occ, F(0.0), w).astype(F).reshape(-1, samples)
    assert cast.all() and (v > 0).all() and (v < samples).any(), "every item sees the light, some through the blocker's edge"
    span = np.array([np.log2(row[row > 0].max() / row[row > 0].min()) for row in masked])
    rule = np.array([DL.rule_reduce(row) for row in masked], F)
    assert DL.same(rule, irr.reshape(-1))
    plain = np.array([AE.ascending_sum(row) for row in masked], F)
    rounds = np.array([AE.round_major_sum(row) for row in masked], F)
    print(f"\n[edges] corner, {samples} samples: weights span {span.min():.1f} .. {span.max():.1f} binades; of {len(rule)} items an ascending sum "
          f"differs in {int((plain != rule).sum())}, a round-major one in {int((rounds != rule).sum())}")
    assert span.min() >= 8.0
    assert 4 * (plain != rule).sum() >= len(rule), "an ascending sum cannot be told from the rule's on this input"
    if samples > 64:
        assert 4 * (rounds != rule).sum() >= len(rule), "a round-major sum cannot be told from the rule's on this input"
    else:
        assert DL.same(rounds, rule), "one round: the round-major order is the rule's"
