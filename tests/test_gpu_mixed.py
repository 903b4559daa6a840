"""Rust2's MixedMaterial on the GPU (the mixed build of the render kernels, RTW_FLAG_MIXED_MATERIAL): every frame against the numpy
restatement of tests/mixed_common.py bit for bit, through every kernel of the build; the unchanged defaults; tree == list, row partition and
two contexts; the error returns.  Frames are small: the restatement traces every pixel in Python."""
import numpy as np
import pytest

import rtw_amd as R
from tests import lights_common as LC
from tests import mixed_common as MC
from tests import oracle_binding as O
from tests.test_gpu_lights import status_of, variants

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 40, 30
ALL = (R.INTEGRATOR_RUST2, R.INTEGRATOR_LIGHT_BIASED, R.INTEGRATOR_LIGHT_CAST)
E_INVALID, E_UNSUPPORTED = -1, -5                       # rtw.h


def flagged(ms, w, h, integ, depth, **kw):
    p = ms.params(w, h, integ, depth, **kw)
    p.flags = R.FLAG_MIXED_MATERIAL
    return p


def compare(gpu, ms, cam, p, lds_geom=False, want_tree=False, build=None):
    """The frame of p through every closest-hit path == the restatement, bit for bit, with its segment count."""
    ref, seg, info = MC.render(ms, cam, p)
    assert np.isfinite(ref).all() and ref.max() > 0 and info["mixed_hits"] > 0
    res = variants(gpu, cam, p, lds_geom=lds_geom, build=build)
    if want_tree:
        assert res["tree, lds nodes"][1].node_tests > 0 and res["tree, global nodes"][1].node_tests > 0 and res["list"][1].node_tests == 0
    for name, (img, st) in res.items():
        print(f"integrator {p.integrator} sampler {p.sampler} [{name}]: {int((img != ref).sum())} values differ, segments {st.segments} / {seg}, "
              f"{info['mixed_hits']} mixed hits")
        assert np.array_equal(img, ref), (p.integrator, p.sampler, name, int((img != ref).sum()))
        assert st.segments == seg and st.camera_rays == p.width * p.height, (name, st.segments, seg)
    return ref, info


# ---- the golden scene: the three integrators, two samplers, list walk and the GEOM tree builds ---------------------------------------------
@pytest.mark.parametrize("sampler", [R.SAMPLER_NO_RAND, R.SAMPLER_ROW])
def test_restatement_golden_scene(gpu, sampler):
    ms, g = MC.golden()
    cam = LC.camera_no_rand(g, W, H)
    gpu.set_scene(ms.scene)
    gpu.set_lights(ms.lights, ms.weight)
    for integ, depth in ((R.INTEGRATOR_RUST2, g["depth_light_biased"]), (R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"]),
                         (R.INTEGRATOR_LIGHT_CAST, g["depth_light_cast"])):
        compare(gpu, ms, cam, flagged(ms, W, H, integ, depth, seed=3, sampler=sampler))    # (one sphere: the tree is a single leaf, no node visits)


def field_scene(moving, box=True):
    """The golden box with lights_common.sphere_field on its floor, every fourth sphere of the field mixed (exp 0, 2, 5, 30 in turn), and a
    rotated mixed box instance; moving: every third sphere of the field has a velocity."""
    ms0, g = MC.golden()
    sp = LC.sphere_field(g)
    rng = np.random.default_rng(4)
    for k, s in enumerate(sp[len(g["spheres"]):]):
        if k % 4 == 0:
            s["material"], s["exp"] = "mixed", [0.0, 2.0, 5.0, 30.0][(k // 4) % 4]
        if moving and k % 3 == 0:
            s["velocity"] = [0.0, float(rng.uniform(0.1, 0.4)), float(rng.uniform(-0.2, 0.2))]
    boxes = [{"a": [-0.5, -0.5, -0.5], "b": [0.5, 0.5, 0.5], "material": "mixed", "exp": 4.0, "color": [0.9, 0.8, 0.3],
              "rotation": [0.3, 0.5, 0.0], "translation": [0.9, -1.2, 3.4]}] if box else []
    return MC.MixedScene(sp, g["quads"], ms0.lights, g["background"], weight=g["biased_weight"], boxes=boxes), g


@pytest.mark.parametrize("moving", [False, True])
def test_restatement_geom_builds_sphere_field_and_box_instance(gpu, moving):
    """GEOM builds (quads + a rotated mixed box instance) over a sphere field: list walk, tree with global and with LDS nodes; MOVING under
    RTW_SAMPLER_ROW with a shutter, so paths run at non-zero ray.time until a mixed surface sends them on at time 0."""
    ms, g = field_scene(moving)
    cam = LC.camera_no_rand(g, W, H)
    if moving:
        cam.time0, cam.shutter = 0.3, 0.5
    gpu.set_scene(ms.scene, 0.0, 1.0)
    gpu.set_lights(ms.lights, ms.weight)
    for integ in (R.INTEGRATOR_LIGHT_BIASED, R.INTEGRATOR_RUST2):
        p = flagged(ms, W, H, integ, 9, seed=5, sampler=R.SAMPLER_ROW if moving else R.SAMPLER_NO_RAND)
        _, info = compare(gpu, ms, cam, p, want_tree=True, build=(10, moving, True))
        assert (info["nonzero_time_queries"] > 0) == moving


def sphere_only(moving):
    """test_gpu_lights' sphere-only scene with a mixed ground (exp 2) and every fourth small sphere mixed: the builds without the quad stage."""
    rng = np.random.default_rng(21)
    sp = [{"origin": [0.0, -101.0, 4.0], "radius": 100.0, "material": "mixed", "exp": 2.0, "color": [0.6, 0.6, 0.5], "emitted": [0, 0, 0]},
          {"origin": [-0.8, 0.6, 3.5], "radius": 0.25, "material": "lambertian", "color": [1, 1, 1], "emitted": [6.0, 5.0, 3.0]},
          {"origin": [1.0, 0.2, 4.5], "radius": 0.2, "material": "lambertian", "color": [1, 1, 1], "emitted": [2.0, 3.0, 6.0]}]
    for k in range(56):
        s = {"origin": [float(rng.uniform(-2.5, 2.5)), float(rng.uniform(-0.9, -0.3)), float(rng.uniform(2.0, 7.0))],
             "radius": float(rng.uniform(0.08, 0.25)), "material": ["lambertian", "mirror", "glass", "mixed"][k % 4], "exp": float(1 + k % 7),
             "color": [float(x) for x in rng.uniform(0.3, 1.0, 3)], "emitted": [0.0, 0.0, 0.0]}
        if moving and k % 3 == 0:
            s["velocity"] = [0.0, float(rng.uniform(0.1, 0.5)), float(rng.uniform(-0.3, 0.3))]
        sp.append(s)
    return MC.MixedScene(sp, [], [(R.LIGHT_SPHERE, 1), (R.LIGHT_SPHERE, 2)], (0.05, 0.06, 0.08), weight=100.0)


@pytest.mark.parametrize("moving", [False, True])
def test_restatement_sphere_only_builds_and_the_time_of_the_scattered_ray(gpu, moving):
    """The builds without quads (list, global nodes, LDS nodes, spheres in LDS or not), static and MOVING.  MOVING: RTW_SAMPLER_ROW with
    time0 = 0.4, shutter = 0.5 -- a path that leaves a mixed surface goes on at ray.time 0 (Ray::new), and the frame restated WITHOUT that
    quirk is a different frame."""
    ms = sphere_only(moving)
    _, g = MC.golden()
    cam = LC.camera_no_rand(g, W, H)
    if moving:
        cam.time0, cam.shutter = 0.4, 0.5
    gpu.set_scene(ms.scene, 0.0, 1.0)
    gpu.set_lights(ms.lights, ms.weight)
    for integ in (R.INTEGRATOR_LIGHT_BIASED, R.INTEGRATOR_RUST2):
        p = flagged(ms, W, H, integ, 9, seed=8, sampler=R.SAMPLER_ROW if moving else R.SAMPLER_NO_RAND)
        ref, info = compare(gpu, ms, cam, p, lds_geom=True, want_tree=True, build=(10, moving, False))
        if moving:
            assert info["time_reset"] > 0
            MC.KEEP_TIME = True
            try:
                other = MC.render(ms, cam, p)[0]
            finally:
                MC.KEEP_TIME = False
            assert not np.array_equal(other, ref)


# ---- the unchanged defaults ----------------------------------------------------------------------------------------------------------------
def counters(st):
    return (st.camera_rays, st.segments, st.sphere_tests, st.node_tests, st.quad_tests, tuple(st.phase_steps), tuple(st.phase_lanes))


def test_flag_without_a_mixed_object_is_the_render_without_the_flag(gpu):
    """No object with opacity < 0: the flag selects nothing -- the same frame and the same counters (the context exposes no kernel name; the
    counters of the existing build, node visits and scheduler steps included, are its fingerprint)."""
    ls, g = LC.golden()
    sp = LC.sphere_field(g)
    ls = LC.LightScene(sp, g["quads"], ls.lights, g["background"], weight=g["biased_weight"])
    w, h = 40, 30
    cam = LC.camera(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    for integ in ALL:
        for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
            p = ls.params(w, h, integ, 9, seed=2, sampler=R.SAMPLER_CENTRES, samples=4, accel=accel)
            plain, st0 = gpu.render(cam, p)
            p.flags = R.FLAG_MIXED_MATERIAL
            img, st1 = gpu.render(cam, p)
            assert np.array_equal(img, plain, equal_nan=True), (integ, accel)
            assert counters(st0)[:5] == counters(st1)[:5], (integ, accel)
            if accel == R.ACCEL_BRUTE:
                assert counters(st0) == counters(st1), (integ, accel)


def test_without_the_flag_opacity_below_zero_means_what_it_meant(gpu):
    """Flag clear, objects with opacity < 0: the oracle's RTW_INTEGRATOR_RUST2 frame, bit for bit (Lambertian / Mirror by metallicness)."""
    ms, g = field_scene(False, box=False)
    w, h = 40, 30
    cam = LC.camera(g, w, h)
    p = ms.params(w, h, R.INTEGRATOR_RUST2, 9, seed=4, sampler=R.SAMPLER_CENTRES, samples=4)
    ref, st_ref = O.render(cam, ms.scene, p, 16)
    assert ref.max() > 0
    gpu.set_scene(ms.scene)
    for name, (img, st) in variants(gpu, cam, p).items():
        assert np.array_equal(img, ref), name
        assert st.segments == st_ref.segments, name
    p.flags = R.FLAG_MIXED_MATERIAL
    assert not np.array_equal(gpu.render(cam, p)[0], ref)                      # ... and with the flag the walls are another material


# ---- tree == list, row partition, two contexts ---------------------------------------------------------------------------------------------
def test_tree_equals_list_at_the_reference_sampler(gpu):
    ms, g = field_scene(True)
    w, h = 40, 30
    cam = LC.camera(g, w, h)
    cam.time0, cam.shutter = 0.2, 0.6
    gpu.set_scene(ms.scene, 0.0, 1.0)
    gpu.set_lights(ms.lights, ms.weight)
    for integ in ALL:
        for sampler, samples in ((R.SAMPLER_CENTRES, 9), (R.SAMPLER_ROW, 5)):
            p = flagged(ms, w, h, integ, 9, seed=6, sampler=sampler, samples=samples)
            res = variants(gpu, cam, p)
            assert res["tree, lds nodes"][1].node_tests > 0 and res["list"][1].node_tests == 0
            for name, (img, st) in res.items():
                assert np.array_equal(img, res["list"][0], equal_nan=True) and st.segments == res["list"][1].segments, (integ, sampler, name)


def test_row_partition_and_two_contexts(gpu):
    ms, g = MC.golden()
    w, h = 40, 30
    cam = LC.camera(g, w, h)
    gpu.set_scene(ms.scene)
    gpu.set_lights(ms.lights, ms.weight)
    for integ in ALL:
        p = flagged(ms, w, h, integ, 9, seed=2, sampler=R.SAMPLER_CENTRES, samples=9, gamma=2.0)
        whole, _ = gpu.render(cam, p)
        rows = np.empty_like(whole)
        for k in range(3):
            q = R.RtwParams.from_buffer_copy(p)
            q.part_index, q.part_count = k, 3
            rows[[r for r in range(h) if (r // 8) % 3 == k]] = gpu.render(cam, q)[0]
        assert np.array_equal(rows, whole, equal_nan=True), integ
        with R.MultiRenderer([0, 0]) as m:
            m.set_scene(ms.scene)
            m.set_lights(ms.lights, ms.weight)
            out = m.render(cam, p)
            img = out[0] if isinstance(out, tuple) else out
            assert np.array_equal(img, whole, equal_nan=True), integ
        q = R.RtwParams.from_buffer_copy(p)
        q.flags = 0
        assert not np.array_equal(gpu.render(cam, q)[0], whole)


# ---- error returns ---------------------------------------------------------------------------------------------------------------------------
def test_error_returns(gpu):
    ms, g = MC.golden()
    cam = LC.camera(g, 16, 12)
    gpu.set_scene(ms.scene)
    for integ in (R.INTEGRATOR_GRADIENT, R.INTEGRATOR_BG_COLOR, R.INTEGRATOR_NORMAL, R.INTEGRATOR_FLAG):
        assert status_of(lambda: gpu.render(cam, flagged(ms, 16, 12, integ, 3))) == E_UNSUPPORTED
        assert status_of(lambda: gpu.render(cam, ms.params(16, 12, integ, 3))) == R.RTW_OK
    for bad in (-1.0, float("inf"), float("nan")):
        q = [dict(x) for x in g["quads"]]
        q[0]["exp"] = bad
        s = MC.MixedScene(g["spheres"], q, ms.lights, g["background"])
        gpu.set_scene(s.scene)
        assert status_of(lambda: gpu.render(cam, flagged(s, 16, 12, R.INTEGRATOR_RUST2, 3))) == E_INVALID
        assert status_of(lambda: gpu.render(cam, s.params(16, 12, R.INTEGRATOR_RUST2, 3))) == R.RTW_OK
    tri = R.Triangle.new([0.0, 0.0, 3.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], color=(0.5, 0.5, 0.5))
    s = R.Scene([ms.scene._spheres[0]], quads=[ms.scene._quads[k] for k in range(len(ms.quads))], triangles=[tri])
    gpu.set_scene(s)
    assert status_of(lambda: gpu.render(cam, flagged(ms, 16, 12, R.INTEGRATOR_RUST2, 3))) == E_UNSUPPORTED
    gpu.set_scene(ms.scene)
    assert status_of(lambda: gpu.render(cam, flagged(ms, 16, 12, R.INTEGRATOR_RUST2, 3))) == R.RTW_OK
