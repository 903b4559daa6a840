"""The light build (SPEC 9) and the mixed build (SPEC 10) of the render kernels at their edges: several samples per pixel under every
sampler, instances under lights (static and MOVING: the GEOM kernels of the light build), the light list up to RTW_MAX_LIGHTS, depth 0 and
1, and what nothing guards (a hit point that is a light's mid-point, odd weights, the ends of the mixed exponent's domain, a lobe seen from
behind, grazing hits on a light).  Every frame is the restatement's frame -- bit-equal, or NaN in both -- with its segment and camera-ray
counts, through every closest-hit path of test_gpu_lights.variants, the list walk first.  No tolerance anywhere.  The scenes, the cases and the
proofs that each case reaches its edge are in tests/test_light_edges_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests import lights_common as LC
from tests import mixed_common as MC
from tests import test_light_edges_cpu as E
from tests.test_gpu_lights import variants
from tests.test_gpu_mixed import counters

pytestmark = pytest.mark.gpu
F = np.float32
CAST, BIASED, RUST2 = E.CAST, E.BIASED, E.RUST2
TREE = ("tree, lds nodes", "tree, global nodes")


def compare(gpu, ms, cam, p, lds_geom=False, what="", build=None):
    """The frame of p through every closest-hit path (list walk first) == the restatement: bit-equal or NaN in both, segments, camera rays.
    The scene and the lights are set by the caller.  Returns (reference frame, restatement's info, {variant: (image, stats)})."""
    ref, seg, info = MC.render(ms, cam, p)
    rays = p.width * p.height * LC.sampler_count(p.sampler, p.samples)[0]
    res = variants(gpu, cam, p, lds_geom=lds_geom, build=build)
    assert list(res)[0] == "list"
    for name, (img, st) in res.items():
        diff = ~((img.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(img) & np.isnan(ref)))
        print(f"{what} integrator {p.integrator} sampler {p.sampler} x {p.samples} depth {p.depth} flags {p.flags} [{name}]: {int(diff.sum())} values "
              f"differ, {int(np.isnan(ref).sum())} NaN in the reference, segments {st.segments} / {seg}, camera rays {st.camera_rays} / {rays}")
        assert not diff.any(), (what, p.integrator, p.sampler, p.samples, p.depth, p.flags, name, int(diff.sum()))
        assert st.segments == seg and st.camera_rays == rays, (what, name, st.segments, seg, st.camera_rays, rays)
    return ref, info, res


def install(gpu, ms, t0=0.0, t1=0.0):
    gpu.set_scene(ms.scene, t0, t1)
    gpu.set_lights(ms.lights, ms.weight)


# ---- 1. several samples per pixel, and the reference's sampler -------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["light", "mixed"])
def test_multi_sample_frames_under_every_sampler(gpu, scene):
    """The golden light / mixed scene under LIGHT_CAST, LIGHT_BIASED and RUST2: CENTRES at 4 and 9 samples, ROW and STRATIFIED at 3 and 10,
    and RTW_FLAG_CHUNK_SUMS once per sampler -- the sample bank, multi-sample work units, the chunk sums and the resolve under the light
    driver against the restatement's own sum."""
    n = 0
    for name, ms, g, integ, depth, flags, sampler, samples in E.multi_sample_cases():
        if name != scene:
            continue
        install(gpu, ms)
        cam = E.camera_for(g, sampler, E.SW, E.SH)
        if sampler == R.SAMPLER_ROW:
            cam.time0, cam.shutter = 0.25, 0.5                # (nothing moves: the draw is made, the time changes nothing but a Mirror's pdf)
        p = E.params(ms, E.SW, E.SH, integ, depth, flags=flags, seed=3 + n, sampler=sampler, samples=samples)
        ref, info, _ = compare(gpu, ms, cam, p, what=scene)
        assert np.isfinite(ref).all() and ref.max() > 0
        if integ != RUST2:
            assert info["reached"].min() > 0                  # both lights contribute
        n += 1
    assert n == 21


def test_multi_sample_sphere_field_through_the_tree(gpu):
    ms, g, p = E.field_multi_sample()
    install(gpu, ms)
    ref, info, res = compare(gpu, ms, LC.camera(g, E.SW, E.SH), p, what="field")
    assert info["reached"].min() > 0 and res["bvh as shipped"][1].node_tests > 0 and res["list"][1].node_tests == 0


# ---- 2. the light-build kernels with GEOM, static and MOVING, and instances under lights ------------------------------------------------------
@pytest.mark.parametrize("moving", [False, True])
def test_instances_under_lights(gpu, moving):
    """render_brute<MOVING, 9, GEOM> and render_bvh<MOVING, {global, LDS}, 9, GEOM> (moving) and their static twins: box instances as first
    hits, as occluders of shadow rays, and compared against the light's object code in shadow_geom_pick.  The same frames with
    RTW_FLAG_MIXED_MATERIAL set (no mixed object: the shim clears it) are the same frames, counters included.  Both renders run the same
    kernel.  Rays, segments, sphere, node and quad tests are compared on every variant.  The tree scheduler's phase_steps / phase_lanes depend on
    which wave takes which work unit from the shared queue, which the request does not define; they were equal over repeated launches of this
    frame, but -- as in test_flag_without_a_mixed_object_is_the_render_without_the_flag -- they are asserted on the list walk only, where one
    unit's steps do not depend on its neighbours."""
    ms, cam, ps = E.instance_cases(moving)
    install(gpu, ms, 0.0, 1.0)
    for p in ps:
        ref, info, res = compare(gpu, ms, cam, p, what=f"instances moving={moving}", build=(9, moving, True))
        E.check_instance_info(info, moving)
        assert np.isfinite(ref).all()
        assert res["list"][1].node_tests == 0
        for name, (_, st) in res.items():
            assert st.quad_tests > 0, name
            if name != "list":
                assert st.node_tests > 0, name
        q = R.RtwParams.from_buffer_copy(p)
        q.flags |= R.FLAG_MIXED_MATERIAL
        for name, (img, st) in variants(gpu, cam, q, build=(9, moving, True)).items():
            assert np.array_equal(img, res[name][0], equal_nan=True), (moving, p.integrator, name)
            assert counters(st)[:5] == counters(res[name][1])[:5], (moving, p.integrator, name)
            if name == "list":
                assert counters(st) == counters(res[name][1]), (moving, p.integrator)


# ---- 3. the light list up to its limit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16])
def test_light_list_up_to_the_limit(gpu, n):
    """n lights -- emissive spheres and quads, one object twice, a hidden light, a light that emits nothing, a sphere light with a velocity:
    the 16 rows of KArgs.lights, the pending-light bits of the flag word and `i < n` in light_step_bvh.  LIGHT_CAST under NO_RAND, LIGHT_BIASED
    under ROW through a shutter; segments == path queries + n * path hits."""
    ms, cam, ps = E.light_list_cases(n)
    install(gpu, ms, 0.0, 1.0)
    for p in ps:
        ref, info, res = compare(gpu, ms, cam, p, what=f"{n} lights")
        assert np.isfinite(ref).all()
        for name, (_, st) in res.items():
            assert st.segments == info["path_queries"] + n * info["path_hits"], name
        for name in TREE:
            assert res[name][1].node_tests > 0, name


# ---- 4. depth 0 and 1 ---------------------------------------------------------------------------------------------------------------------------
def test_depth_zero_and_one(gpu):
    """LIGHT_CAST, LIGHT_BIASED and RUST2 plus the flag at depth 0 and 1, list and tree, GEOM and sphere-only, both builds."""
    for name, ms, g, flags, has_quads in E.depth_cases():
        cam = LC.camera_no_rand(g, E.W, E.H)
        install(gpu, ms)
        bg = np.broadcast_to(ms.background, (E.H, E.W, 3))
        for p in E.depth_params(ms, flags):
            ref, info, res = compare(gpu, ms, cam, p, lds_geom=not has_quads, what=name)
            if p.depth == 0 and p.integrator != CAST:
                for v, (img, st) in res.items():
                    assert np.array_equal(img, bg) and st.segments == 0, (name, p.integrator, v)


# ---- 5. what nothing guards -------------------------------------------------------------------------------------------------------------------
def test_a_first_hit_that_is_a_lights_mid_point(gpu):
    """The shadow direction is 0 / 0.  The list walk first; then the tree, which hands such a ray to the list walk (wild_ray_query) -- with a
    field of 60 spheres also as shipped.  The tiny-light cases put NaN into the pixel, here and in the restatement."""
    for name, ms, cam, (i, j), P, li, want_nan in E.mid_point_cases():
        install(gpu, ms)
        for p in E.mid_point_params(ms):
            ref, info, res = compare(gpu, ms, cam, p, lds_geom=not ms.quads, what=name)
            assert bool(np.isnan(ref).any()) == want_nan and (not want_nan or np.isnan(ref[j, i]).any()), name
            if len(ms.spheres) > 48:
                assert res["bvh as shipped"][1].node_tests > 0, name


@pytest.mark.parametrize("weight", E.WEIGHTS)
def test_weights_rtw_ctx_set_lights_does_not_check(gpu, weight):
    """0, 1e30, NaN, inf and negative weights are accepted (status 0) and rendered as the restatement renders them."""
    ms, cam, p = E.weight_case(weight)
    gpu.set_scene(ms.scene)
    arr, n = R._light_array(ms.lights)
    assert R.lib().rtw_ctx_set_lights(gpu._h, arr, n, float(weight)) == R.RTW_OK
    ref, info, _ = compare(gpu, ms, cam, p, what=f"weight {weight}")
    assert E.lively(ref) and info["reached"].min() > 0
    assert bool(np.isfinite(ref).all()) == (weight in (0.0, 1e30, -100.0)), weight


def test_mixed_exponents_at_the_ends_a_lobe_from_behind_and_mixed_lights(gpu):
    ms, g = E.mixed_edge_scene()
    install(gpu, ms)
    cam = LC.camera_no_rand(g, E.W, E.H)
    for p in E.mixed_edge_params(ms):
        ref, info, _ = compare(gpu, ms, cam, p, what="mixed edges")
        assert info["mixed_hits"] > 0


def test_grazing_hits_on_a_light(gpu):
    ms, cam, ps = E.grazing_case()
    install(gpu, ms)
    for p in ps:
        ref, info, _ = compare(gpu, ms, cam, p, what="grazing")
        assert np.isfinite(ref).all() and E.lively(ref) and info["reached"][2] > 0


def test_a_pdf_equal_to_the_threshold_is_skipped(gpu):
    """LIGHT_BIASED skips a light when pdf <= 1 / (255 max e): on walls of MixedMaterial::new(0) the pdf of a dim light IS its threshold, bit
    for bit (tests/test_light_edges_cpu.py shows that equality is met and that `<` would give another frame)."""
    ms, cam, p = E.threshold_case()
    install(gpu, ms)
    ref, info, _ = compare(gpu, ms, cam, p, what="pdf == threshold")
    assert np.isfinite(ref).all() and E.lively(ref) and info["reached"][2] > 0
