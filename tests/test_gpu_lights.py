"""Rust2's light-biased integrators on the GPU (the light build of the render kernels): identities against the frozen CPU oracle, the
numpy restatement of tests/lights_common.py bit for bit under RTW_SAMPLER_NO_RAND, list walk == tree, row partition / multi-context, the
error paths, and the reference's own pipeline end to end.  Every pixel of every frame is compared."""
import numpy as np
import pytest

import rtw_amd as R
from tests import builds_common as B
from tests import lights_common as LC
from tests import oracle_binding as O

pytestmark = pytest.mark.gpu
F = np.float32
LIGHT = (R.INTEGRATOR_LIGHT_CAST, R.INTEGRATOR_LIGHT_BIASED)


# The kernels the enumerations through variants() declare and run (tests/test_render_builds_cpu.py holds the tables against the library),
# each where a test passes variants() its build: the light build (SPEC 9) without quads or instances -- test_restatement_sphere_only_scene
# here -- and with them -- test_gpu_light_edges.test_instances_under_lights --; the mixed build (SPEC 10) -- test_gpu_mixed's sphere-only
# and GEOM restatements --; the quaternion build (SPEC 11) -- test_gpu_quat_instances.test_bounce_for_bounce --; the placement build (SPEC
# 12) -- test_gpu_mesh_instances.test_bounce_for_bounce.
BUILDS = B.family(9, False) | B.family(9, True) | B.family(10, False) | B.family(10, True) | B.family(11, True) | B.family(12, True)


def variants(gpu, cam, p, lds_geom=False, build=None):
    """The frame through every closest-hit path: list walk, BVH request as shipped, tree forced with the nodes in LDS / in global memory
    (and, sphere-only scenes, the spheres in LDS or not).  {name: (image, stats)}
    build = (SPEC, MOVING, GEOM), the build the caller declares for its scene and request: every render is then asked which kernel it ran.
    The forced requests name theirs -- render_brute, render_bvh at NODES 1, 0, and 1 + v under RTW_OPT_LDS_GEOM = v --; with the knobs as
    shipped the request may walk the list, and a tree without quads or instances may or may not keep its spheres in LDS."""
    out = {}

    def render(name, *nodes):
        out[name] = gpu.render(cam, p)
        if build is not None:
            spec, moving, geom = build
            want = [B.tag(moving, n, spec, geom) for n in nodes]
            got = gpu.last_render_build()
            assert got in want and set(want) <= BUILDS, (name, got, want)

    p = R.RtwParams.from_buffer_copy(p)
    auto = (1,) if build is not None and build[2] else (1, 2)
    p.accel = R.ACCEL_BRUTE
    render("list", None)
    p.accel = R.ACCEL_BVH
    render("bvh as shipped", None, *auto)
    gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
    try:
        render("tree, lds nodes", *auto)
        if lds_geom:
            for v in (0, 1):
                gpu.set_option(R.OPT_LDS_GEOM, v)
                render(f"tree, lds geom {v}", 1 + v)
            gpu.set_option(R.OPT_LDS_GEOM, -1)
        p.flags |= R.FLAG_GLOBAL_NODES
        render("tree, global nodes", 0)
    finally:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
        gpu.set_option(R.OPT_LDS_GEOM, -1)
    return out


# ---- 4. identities against the frozen oracle -------------------------------------------------------------------------------------------
def test_identity_golden_scene_no_lights_and_weight_zero(gpu):
    _, g = LC.golden()
    w, h = 80, 60
    cam = LC.camera(g, w, h)
    for ls in (LC.LightScene(g["spheres"], g["quads"], [], g["background"]), LC.golden(weight=0.0)[0]):
        p = ls.params(w, h, R.INTEGRATOR_RUST2, 9, seed=7, sampler=R.SAMPLER_CENTRES, samples=9)
        ref, st_ref = O.render(cam, ls.scene, p, 16)
        assert ref.max() > 0
        gpu.set_scene(ls.scene)
        gpu.set_lights(ls.lights, ls.weight)
        p.integrator = R.INTEGRATOR_LIGHT_BIASED
        for name, (img, st) in variants(gpu, cam, p).items():
            assert np.array_equal(img, ref), (name, len(ls.lights), np.abs(img - ref).max())
            assert st.camera_rays == st_ref.camera_rays, name
            if not ls.lights:
                assert st.segments == st_ref.segments, name


def sphere_field(moving):
    base = R.Scene.generate(R.SCENE_C2)
    pods = [base._spheres[i] for i in range(base.n_spheres)]
    if moving:
        for i, s in enumerate(pods):
            if i % 3 == 1:
                s.velocity[1] = 0.3
    return R.Scene(pods, background=(0.6, 0.7, 0.9))


@pytest.mark.parametrize("moving", [False, True])
def test_identity_sphere_scene_through_the_tree(gpu, moving):
    from tests.test_oracle_golden import small_view
    _, cam, p = small_view(R.SCENE_C2, 96, 54, 9)
    scene = sphere_field(moving)
    p.integrator, p.sampler, p.samples, p.depth, p.gamma, p.seed = R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 9, 9, 1.0, 3
    ref, st_ref = O.render(cam, scene, p, 16)
    gpu.set_scene(scene, 0.0, 1.0)
    p.integrator = R.INTEGRATOR_LIGHT_BIASED
    for lights, weight in ((None, 100.0), ([(R.LIGHT_SPHERE, 1), (R.LIGHT_SPHERE, 5)], 0.0)):
        gpu.set_lights(lights, weight)
        res = variants(gpu, cam, p, lds_geom=True)
        assert res["tree, lds nodes"][1].node_tests > 0
        for name, (img, st) in res.items():
            assert np.array_equal(img, ref), (name, moving, lights, np.abs(img - ref).max())
            if lights is None:
                assert st.segments == st_ref.segments, name


# ---- 5. the restatement, bit for bit --------------------------------------------------------------------------------------------------
def occluded_scene():
    ls, g = LC.golden()
    blocker = {"origin": [-0.3, -0.3, 4.2], "u": [0.6, 0.0, 0.0], "v": [0.0, 0.6, 0.0], "material": "lambertian", "color": [0.5, 0.5, 0.5],
               "emitted": [0.0, 0.0, 0.0]}
    return LC.LightScene(g["spheres"], g["quads"] + [blocker], [ls.lights[0]], g["background"], weight=g["biased_weight"]), g


def emission_image_scene():
    _, g = LC.golden()
    rng = np.random.default_rng(2)
    albedo = rng.uniform(0.2, 1.0, (2, 4, 3)).astype(F)
    emission = rng.uniform(0.5, 6.0, (2, 2, 3)).astype(F)
    sp = [{"origin": [0.6, 0.4, 4.0], "radius": 0.35, "material": "lambertian", "color": [1, 1, 1], "emitted": [0.0, 0.0, 0.0], "tex": 0}]
    quads = [q for q in g["quads"] if q["name"] != "light quad"]
    return LC.LightScene(sp, quads, [(R.LIGHT_SPHERE, 0)], g["background"], textures=[albedo, emission], emission_images={0: 1},
                         weight=g["biased_weight"]), g


def compare_with_restatement(gpu, ls, g, w, h, configs):
    """Every frame of `configs` through every closest-hit path == the restatement bit for bit, with its segment count.  Returns, per
    config, the restatement's count of shadow queries per light that ended on another object."""
    cam = LC.camera_no_rand(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    blocked_all = []
    for integ, depth, seed in configs:
        p = ls.params(w, h, integ, depth, seed=seed)
        ref, seg, blocked = LC.render(ls, cam, p)
        blocked_all.append(blocked)
        assert np.isfinite(ref).all() and ref.max() > 0
        for name, (img, st) in variants(gpu, cam, p).items():
            same = (img == ref) | (np.isnan(img) & np.isnan(ref))
            print(f"integrator {integ} depth {depth} seed {seed} [{name}]: {int((~same).sum())} values differ, max |diff| {np.nanmax(np.abs(img - ref)):.3g}, "
                  f"segments {st.segments} / {seg}")
            assert same.all(), (integ, depth, seed, name)
            assert st.segments == seg and st.camera_rays == w * h, (name, st.segments, seg)
    return blocked_all


CONFIGS = [(R.INTEGRATOR_LIGHT_CAST, 10, 1), (R.INTEGRATOR_LIGHT_BIASED, 1, 1), (R.INTEGRATOR_LIGHT_BIASED, 2, 2),
           (R.INTEGRATOR_LIGHT_BIASED, 9, 1), (R.INTEGRATOR_LIGHT_BIASED, 9, 5)]


def test_restatement_golden_scene(gpu):
    ls, g = LC.golden()
    # the frame looks at both lights: some camera rays end ON a light (a hit point on the light itself)
    cam = LC.camera_no_rand(g, 40, 30)
    p1 = ls.params(40, 30, R.INTEGRATOR_RUST2, 1)
    first = [LC.closest(ls, *LC.camera_ray(cam, i, j), p1, j * 40 + i) for j in range(30) for i in range(40)]
    assert sum(1 for f in first if f is not None and f[0] in ls.light_obj) > 0
    compare_with_restatement(gpu, ls, g, 40, 30, CONFIGS)


def test_restatement_mirror_and_glass(gpu):
    ls, g = LC.mirror_glass_scene()
    compare_with_restatement(gpu, ls, g, 40, 30, [CONFIGS[0], CONFIGS[3], (R.INTEGRATOR_LIGHT_BIASED, 9, 8)])


def test_restatement_occluded_light(gpu):
    ls, g = occluded_scene()
    # the blocker hides the light quad from every surface point in front of it: every camera ray's first hit has z <= 4.2 or lies on the
    # walls beside it, and the restatement says how many shadow queries actually ended on another object than the light
    ls_open, _ = LC.golden()
    ls_open = LC.LightScene(g["spheres"], g["quads"], [ls_open.lights[0]], g["background"], weight=g["biased_weight"])
    cam = LC.camera_no_rand(g, 40, 30)
    p = ls.params(40, 30, R.INTEGRATOR_LIGHT_CAST, 10)
    _, _, open_blocked = LC.render(ls_open, cam, p)
    blocked = compare_with_restatement(gpu, ls, g, 40, 30, [CONFIGS[0], CONFIGS[3]])
    assert blocked[0][0] > open_blocked[0] and blocked[1][0] > 0, (blocked, open_blocked)
    # ... and geometrically: a first hit in front of the blocker's plane whose segment to the light's mid-point crosses that plane well inside
    # the blocker (|x|, |y| < 0.29 of its 0.3) must have its shadow query stopped by another object
    p1 = ls.params(40, 30, R.INTEGRATOR_RUST2, 1)
    n_front = 0
    for j in range(30):
        for i in range(40):
            o, d = LC.camera_ray(cam, i, j)
            h = LC.closest(ls, o, d, p1, j * 40 + i)
            if h is None or h[2][2] >= 4.19:
                continue
            pt, mid = h[2].astype(np.float64), ls.mids[0].astype(np.float64)
            c = pt + (mid - pt) * (4.2 - pt[2]) / (mid[2] - pt[2])
            if abs(c[0]) >= 0.29 or abs(c[1]) >= 0.29:
                continue
            sh = LC.closest(ls, h[2], LC.unit((ls.mids[0] - h[2]).astype(F)), p1, j * 40 + i)
            assert sh is not None and sh[0] != ls.light_obj[0], (i, j)
            n_front += 1
    assert n_front > 0


def test_restatement_emission_image_light(gpu):
    ls, g = emission_image_scene()
    compare_with_restatement(gpu, ls, g, 40, 30, [CONFIGS[0], CONFIGS[3]])


# ---- 5b. sphere-only scenes: the builds without quads, static and MOVING, with a light that is actually added -----------------------------
def sphere_only_scene(moving):
    """58 spheres over a large ground sphere, two of them emissive and the lights; no quads.  moving: every third sphere has a velocity (the
    lights stand still: a light's mid-point is its place at time 0)."""
    rng = np.random.default_rng(21)
    sp = [{"origin": [0.0, -101.0, 4.0], "radius": 100.0, "material": "lambertian", "color": [0.6, 0.6, 0.5], "emitted": [0, 0, 0]},
          {"origin": [-0.8, 0.6, 3.5], "radius": 0.25, "material": "lambertian", "color": [1, 1, 1], "emitted": [6.0, 5.0, 3.0]},
          {"origin": [1.0, 0.2, 4.5], "radius": 0.2, "material": "lambertian", "color": [1, 1, 1], "emitted": [2.0, 3.0, 6.0]}]
    for k in range(56):
        s = {"origin": [float(rng.uniform(-2.5, 2.5)), float(rng.uniform(-0.9, -0.3)), float(rng.uniform(2.0, 7.0))],
             "radius": float(rng.uniform(0.08, 0.25)), "material": ["lambertian", "mirror", "glass"][k % 3],
             "color": [float(x) for x in rng.uniform(0.3, 1.0, 3)], "emitted": [0.0, 0.0, 0.0]}
        if moving and k % 3 == 0:
            s["velocity"] = [0.0, float(rng.uniform(0.1, 0.5)), float(rng.uniform(-0.3, 0.3))]
        sp.append(s)
    return LC.LightScene(sp, [], [(R.LIGHT_SPHERE, 1), (R.LIGHT_SPHERE, 2)], (0.05, 0.06, 0.08), weight=100.0)


@pytest.mark.parametrize("moving", [False, True])
def test_restatement_sphere_only_scene(gpu, moving):
    """The kernels without the quad stage (list walk, tree with global / LDS nodes, spheres in LDS or not), static and MOVING, against the
    restatement with lights that pass the threshold -- NO_RAND (ray.time 0)."""
    ls = sphere_only_scene(moving)
    _, g = LC.golden()
    w, h = 32, 24
    cam = LC.camera_no_rand(g, w, h)
    gpu.set_scene(ls.scene, 0.0, 1.0)
    gpu.set_lights(ls.lights, ls.weight)
    for integ, depth, seed in ((R.INTEGRATOR_LIGHT_CAST, 10, 1), (R.INTEGRATOR_LIGHT_BIASED, 9, 4)):
        p = ls.params(w, h, integ, depth, seed=seed)
        ref, seg, _ = LC.render(ls, cam, p)
        p.integrator = R.INTEGRATOR_RUST2
        plain, _ = O.render(cam, ls.scene, p, 16)
        p.integrator = integ
        assert np.isfinite(ref).all() and not np.array_equal(ref, plain)          # the lights add something
        res = variants(gpu, cam, p, lds_geom=True, build=(9, moving, False))
        assert res["tree, lds nodes"][1].node_tests > 0
        for name, (img, st) in res.items():
            assert np.array_equal(img, ref), (moving, integ, name, int((img != ref).sum()))
            assert st.segments == seg, (moving, integ, name, st.segments, seg)


def test_shadow_rays_run_at_time_zero_whatever_the_paths_time(gpu):
    """RTW_SAMPLER_ROW with time0 = 0.4, shutter = 0.5: every path has its own ray.time in [0.4, 0.9), the spheres move, and the shadow rays
    still run at time 0 (where the restatement asks the oracle for them; a Mirror's pdf is then 0 by its exact time compare).  The tree covers
    [0, 1]; set for [0.4, 0.9] alone it does not cover the shadow rays' time and the request walks the list -- the same image."""
    ls = sphere_only_scene(True)
    _, g = LC.golden()
    w, h = 32, 24
    cam = LC.camera_no_rand(g, w, h)
    cam.time0, cam.shutter = 0.4, 0.5
    for integ, depth, seed in ((R.INTEGRATOR_LIGHT_CAST, 10, 2), (R.INTEGRATOR_LIGHT_BIASED, 9, 3)):
        p = ls.params(w, h, integ, depth, seed=seed, sampler=R.SAMPLER_ROW)
        ref, seg, _ = LC.render(ls, cam, p)
        # the restated camera draws of render_row are the oracle's: without lights the restatement is the oracle's RUST2 frame
        dark = LC.LightScene(ls.spheres, [], [], ls.background)
        if integ == R.INTEGRATOR_LIGHT_BIASED:
            q = R.RtwParams.from_buffer_copy(p)
            q.integrator = R.INTEGRATOR_RUST2
            assert np.array_equal(LC.render(dark, cam, p)[0], O.render(cam, dark.scene, q, 16)[0])
        still = R.RtwCamera.from_buffer_copy(cam)
        still.time0, still.shutter = 0.0, 0.0
        assert np.isfinite(ref).all() and not np.array_equal(ref, LC.render(ls, still, p)[0])       # the time matters in this scene
        for t0, t1, tree in ((0.0, 1.0, True), (0.4, 0.9, False)):
            gpu.set_scene(ls.scene, t0, t1)
            gpu.set_lights(ls.lights, ls.weight)
            res = variants(gpu, cam, p, lds_geom=True)
            assert (res["tree, lds nodes"][1].node_tests > 0) == tree
            for name, (img, st) in res.items():
                assert np.array_equal(img, ref), (integ, t0, name, int((img != ref).sum()))
                assert st.segments == seg, (integ, t0, name)


# ---- 6. list walk == tree, and the segment count -----------------------------------------------------------------------------------------
def test_brute_equals_bvh_with_a_sphere_field(gpu):
    ls0, g = LC.golden()
    sp = LC.sphere_field(g)
    ls = LC.LightScene(sp, g["quads"], ls0.lights, g["background"], weight=g["biased_weight"])
    w, h = 32, 24
    cam = LC.camera_no_rand(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    for integ in LIGHT:
        p = ls.params(w, h, integ, 9, seed=6)
        ref, seg, _ = LC.render(ls, cam, p)
        res = variants(gpu, cam, p)
        assert res["bvh as shipped"][1].node_tests > 0 and res["list"][1].node_tests == 0
        for name, (img, st) in res.items():
            assert np.array_equal(img, res["list"][0], equal_nan=True), (integ, name)
            assert st.segments == res["list"][1].segments == seg, (integ, name, st.segments, seg)
        assert np.array_equal(res["list"][0], ref, equal_nan=True), integ
        # at the reference's sampler too (no restatement: the two kernels against each other)
        p = ls.params(w, h, integ, 9, seed=6, sampler=R.SAMPLER_CENTRES, samples=9)
        res = variants(gpu, LC.camera(g, w, h), p)
        for name, (img, st) in res.items():
            assert np.array_equal(img, res["list"][0], equal_nan=True) and st.segments == res["list"][1].segments, (integ, name)


# ---- 7. row partition and several contexts ---------------------------------------------------------------------------------------------
def test_row_partition_and_two_contexts(gpu):
    ls, g = LC.golden()
    w, h = 64, 48
    cam = LC.camera(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    for integ in LIGHT:
        p = ls.params(w, h, integ, 9, seed=2, sampler=R.SAMPLER_CENTRES, samples=9, gamma=2.0)
        whole, st = gpu.render(cam, p)
        parts = []
        for k in range(3):
            q = R.RtwParams.from_buffer_copy(p)
            q.part_index, q.part_count = k, 3
            parts.append(gpu.render(cam, q)[0])
        rows = np.empty_like(whole)
        idx = [[r for r in range(h) if (r // 8) % 3 == k] for k in range(3)]
        for k in range(3):
            rows[idx[k]] = parts[k]
        assert np.array_equal(rows, whole, equal_nan=True), integ
        with R.MultiRenderer([0, 0]) as m:
            m.set_scene(ls.scene)
            m.set_lights(ls.lights, ls.weight)
            out = m.render(cam, p)
            img = out[0] if isinstance(out, tuple) else out
            assert np.array_equal(img, whole, equal_nan=True), integ


# ---- 8. error paths --------------------------------------------------------------------------------------------------------------------
def status_of(fn):
    try:
        fn()
    except R.RtwError as e:
        return e.status
    return 0


def test_set_lights_raw_argument_checks(gpu):
    """rtw_ctx_set_lights itself, through ctypes (the Python wrapper cannot form a NULL / n mismatch): on a real context."""
    import ctypes as C
    L = R.lib()
    one = (R.RtwLight * 1)(R.RtwLight(R.LIGHT_QUAD, 1))
    ls, g = LC.golden()
    with R.Renderer(0) as fresh:
        assert L.rtw_ctx_set_lights(fresh._h, one, 1, 100.0) == -6              # RTW_E_NO_SCENE before any scene
        assert L.rtw_ctx_set_lights(fresh._h, None, 0, 100.0) == -6
        fresh.set_scene(ls.scene)
        assert L.rtw_ctx_set_lights(fresh._h, None, 1, 100.0) == -1             # NULL with n = 1
        assert L.rtw_ctx_set_lights(fresh._h, one, 0, 100.0) == -1              # a list with n = 0
        assert L.rtw_ctx_set_lights(fresh._h, (R.RtwLight * 1)(R.RtwLight(2, 0)), 1, 100.0) == -1
        assert L.rtw_ctx_set_lights(fresh._h, (R.RtwLight * 17)(), 17, 100.0) == -1
        assert L.rtw_ctx_set_lights(fresh._h, one, 1, 100.0) == 0
        assert L.rtw_ctx_set_lights(fresh._h, None, 0, 100.0) == 0              # the legal clear
    with R.MultiRenderer([0, 0]) as m:
        m.set_scene(ls.scene)
        assert L.rtw_mgpu_set_lights(m._h, None, 1, 100.0) == -1
        assert L.rtw_mgpu_set_lights(m._h, one, 1, 100.0) == 0


def test_error_paths(gpu):
    ls, g = LC.golden()
    cam = LC.camera(g, 16, 12)
    p = ls.params(16, 12, R.INTEGRATOR_LIGHT_BIASED, 3)
    gpu.set_scene(ls.scene)
    assert status_of(lambda: gpu.set_lights([(R.LIGHT_SPHERE, 1)])) == -1          # index beyond the scene
    assert status_of(lambda: gpu.set_lights([(R.LIGHT_QUAD, 6)])) == -1
    assert status_of(lambda: gpu.set_lights([(2, 0)])) == -1
    assert status_of(lambda: gpu.set_lights([(R.LIGHT_QUAD, 0)] * 17)) == -1
    gpu.set_lights(ls.lights)
    p.integrator = 7
    assert status_of(lambda: gpu.render(cam, p)) == -1
    # a new scene clears the lights: the render is the no-light one
    gpu.set_scene(ls.scene)
    p.integrator = R.INTEGRATOR_LIGHT_BIASED
    a = gpu.render(cam, p)[0]
    gpu.set_lights(None)
    assert np.array_equal(a, gpu.render(cam, p)[0])
    # triangles, texture noise, a constant-density instance: RTW_E_UNSUPPORTED for both integrators
    gpu.set_triangles([R.Triangle.new((0, 0, 3), (1, 0, 0), (0, 1, 0))])
    for integ in LIGHT:
        p.integrator = integ
        assert status_of(lambda: gpu.render(cam, p)) == -5
    gpu.set_triangles(None)
    tex, entry = R.texture_from_color_noise((0.5, 0.5, 0.5), 2.0)
    noisy = R.Scene([R.Sphere.new_with_texture((0, 0, 3), 1.0, (1, 1, 1), None, 0)], textures=[tex], noise={0: entry})
    gpu.set_scene(noisy)
    for integ in LIGHT:
        p.integrator = integ
        assert status_of(lambda: gpu.render(cam, p)) == -5
    box = R.Instance.new_box((-1, -1, 2), (1, 1, 4), (1, 1, 1), None)
    box.const_density(0.5)
    gpu.set_scene(R.Scene.new([], [], [box]))
    for integ in LIGHT:
        p.integrator = integ
        assert status_of(lambda: gpu.render(cam, p)) == -5
    p.integrator = R.INTEGRATOR_RUST2
    gpu.render(cam, p)


# ---- 9. end to end: the reference's own pipeline -----------------------------------------------------------------------------------------
def test_end_to_end_reference_pipeline(gpu):
    ls, g = LC.golden()
    w, h = g["width"], g["height"]
    cam = LC.camera(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    p = ls.params(w, h, R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"], seed=1, sampler=R.SAMPLER_CENTRES, samples=g["samples"],
                  gamma=g["gamma"], mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
    lit, st = gpu.render(cam, p)
    p.integrator = R.INTEGRATOR_RUST2
    plain, st0 = gpu.render(cam, p)
    assert np.isfinite(lit).all()
    u8 = R.quantize_u8_rust2(lit)
    out = gpu.bilateral_filter(u8, 3)
    out = out[0] if isinstance(out, tuple) else out
    assert out.shape == u8.shape and out.dtype == np.uint8
    mean_lit, mean_plain = float(u8.mean()), float(R.quantize_u8_rust2(plain).mean())
    # by how much, from the restatement at a reduced size (linear radiance, several seeds): the ratio of the two integrators' mean radiance
    rw, rh = 40, 30
    rcam = LC.camera_no_rand(g, rw, rh)
    ratios = []
    for seed in range(1, 7):
        pr = ls.params(rw, rh, R.INTEGRATOR_LIGHT_BIASED, 9, seed=seed)
        a, _, _ = LC.render(ls, rcam, pr)
        pr.integrator = R.INTEGRATOR_RUST2
        b, _ = O.render(rcam, ls.scene, pr, 16)
        ratios.append(float(a.mean()) / max(float(b.mean()), 1e-12))
    lin = float(lit.astype(np.float64).__pow__(g["gamma"]).mean()) / max(float(plain.astype(np.float64).__pow__(g["gamma"]).mean()), 1e-12)
    lo, hi = min(ratios), max(ratios)
    print(f"mean of the 8-bit frame: light-biased {mean_lit:.2f}, ray_color {mean_plain:.2f}; linear ratio {lin:.3f}; "
          f"restatement's ratio over seeds {lo:.3f} .. {hi:.3f}; segments {st.segments} vs {st0.segments}; {st.kernel_ms:.2f} ms vs {st0.kernel_ms:.2f} ms")
    assert mean_lit > mean_plain
    assert lo <= lin <= hi, (lin, ratios)
