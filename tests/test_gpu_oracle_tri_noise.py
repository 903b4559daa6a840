"""The triangle build (SPEC 8) and the noise build (SPEC 7) of the render kernels against the CPU oracle, bit for bit (rtw_oracle_render_ex:
the oracle's own restatement of Rust2's Triangle and of PerlinNoise), bounce for bounce: metal, glass, textured (both texel rules) and
emissive triangles, a triangle that ties a quad, noise seen after a bounce, on moving spheres and on an instance member; every build each
scene can reach.  Textured spheres are compared under RTW_ORACLE_FLAG_DEVICE_UV (the device's atan2 / acos sequences), which makes the texel
choice the device's: nothing is left to a tolerance.

Which build runs is argued from render_need (rtw_host.cpp), as in test_every_build_of_the_traversal_kernel: triangles select
SPEC 8 with GEOM for every integrator, sampler and flag, and noise in use selects SPEC 7 (with GEOM when the scene has quads or
instances, without otherwise); a scene with a moving sphere runs the MOVING half.  Within a build: RTW_ACCEL_BRUTE is the list walk;
RTW_ACCEL_BVH with RTW_OPT_LIST_WALK_MAX = 0 (so that the sphere count does not send the request to the list walk) is render_bvh, whose node
argument is 0 under RTW_FLAG_GLOBAL_NODES (f32 nodes in global memory), else 1 (f16 nodes in LDS), or 2 (LDS nodes plus the sphere geometry in
LDS: RTW_OPT_LDS_GEOM = 1, the spheres-only builds; the GEOM builds have no such variant)."""
import numpy as np
import pytest

import rtw_amd as R
from tests import builds_common as B
from tests import oracle_binding as O
from tests.test_gpu_perlin import noised_c5
from tests.test_gpu_triangles import CONFIGS, mixed_scene, params, view

pytestmark = pytest.mark.gpu

f32 = np.float32
THREADS = 16
NOISE_CONFIGS = [c for c in CONFIGS if c[0] != R.INTEGRATOR_RUST2] + [(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, R.FLAG_CHUNK_SUMS)]   # Rust2 has no noise


def exact(img, ref):
    """Bit for bit; NaN (which a scale of 0 produces) must be NaN on both sides -- its payload is the hardware's, not the arithmetic's."""
    a, b = np.isnan(img), np.isnan(ref)
    return np.array_equal(a, b) and np.array_equal(np.where(a, 0, img).view(np.uint32), np.where(b, 0, ref).view(np.uint32))


def where(img, ref):
    bad = ~((img.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(img) & np.isnan(ref))).all(axis=2)
    return f"{int(bad.sum())} pixels differ, first {np.argwhere(bad)[:3].tolist()}"


# the builds: (name, accel, flags added, RTW_OPT_LDS_GEOM, NODES of render_bvh or None for render_brute)
LIST = ("list walk", R.ACCEL_BRUTE, 0, -1, None)
NODES0 = ("tree, global nodes", R.ACCEL_BVH, R.FLAG_GLOBAL_NODES, -1, 0)
NODES1 = ("tree, LDS nodes", R.ACCEL_BVH, 0, 0, 1)
NODES2 = ("tree, LDS nodes + LDS spheres", R.ACCEL_BVH, 0, 1, 2)

# the kernels these tests declare and run (tests/test_render_builds_cpu.py holds the tables against the library): the noise build without
# and with quads / instances, and the triangle build
BUILDS = B.family(7, False) | B.family(7, True) | B.family(8, True)


def against_oracle(gpu, scene, cam, p, builds, spec, moving, geom, list_quad_tests=True):
    """Render `scene` through each of `builds` and compare every image and segment count with the oracle's; the list walk's quad_tests too.
    Every render ran render_brute / render_bvh<moving, NODES of the build, spec, geom>."""
    ref, st_ref = O.render(cam, scene, p, THREADS, device_uv=True)
    gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
    gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
    flags = p.flags
    try:
        for name, accel, extra, lds_geom, nodes in builds:
            gpu.set_option(R.OPT_LDS_GEOM, lds_geom)
            p.accel, p.flags = accel, flags | extra
            img, st = gpu.render(cam, p)
            assert B.tag(moving, nodes, spec, geom) in BUILDS
            B.ran(gpu, B.tag(moving, nodes, spec, geom), name)
            assert exact(img, ref), (name, where(img, ref))
            assert st.segments == st_ref.segments, (name, st.segments, st_ref.segments)
            if accel == R.ACCEL_BRUTE and list_quad_tests:
                assert st.quad_tests == st_ref.quad_tests, (name, st.quad_tests, st_ref.quad_tests)
            if accel == R.ACCEL_BVH:
                assert st.node_tests > 0, name
    finally:
        p.flags = flags
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
        gpu.set_option(R.OPT_LDS_GEOM, -1)
    return ref, st_ref


# ---- triangles: the six kernels of the triangle build (MOVING x {list walk, tree / global nodes, tree / LDS nodes}) --------------------
TIE_QUAD = ((-1.5, 1.2, 3.0), (1.2, 0.0, 0.0), (0.0, 1.0, 0.0))       # a wall facing the camera, above everything else


def tri_scene(moving):
    """mixed_scene (metal, glass and textured icosphere faces; spheres, quads, a rotated box and a medium) with, in front of its triangle list:
    a big textured wall (texture 0, which has an emission image: Rust2's rule under RUST2, the quad rule otherwise), an emissive triangle, a
    textured metal triangle, and a triangle built from the origin and edges of one more quad -- the same plane, so it ties the quad at
    equal t and must lose to it.  moving: every third small sphere moves (the MOVING half of the build)."""
    extra = [R.Triangle.new((-4.0, 0.05, -3.0), (3.0, 0.0, 0.0), (0.0, 2.5, 0.0), R.SCATTER_M, (1, 1, 1), tex_index=0),
             R.Triangle.new((2.5, 0.3, -2.0), (1.0, 0.0, 0.0), (0.0, 1.5, 0.0), R.SCATTER_M, (0.9, 0.9, 0.9), emitted=(3.0, 2.0, 1.0)),
             R.Triangle.new(TIE_QUAD[0], TIE_QUAD[1], TIE_QUAD[2], R.SCATTER_M, (0.1, 0.9, 0.1), emitted=(0.0, 2.0, 0.0)),
             R.Triangle.new((0.5, 0.05, 2.0), (1.2, 0.0, 0.0), (0.3, 1.4, 0.0), R.METALLIC_M, (0.9, 0.8, 0.7), tex_index=0)]
    scene = mixed_scene(extra)
    quads = list(scene._quads)[:scene.n_quads] + [R.Quad.new(*TIE_QUAD, R.SCATTER_M, (0.9, 0.2, 0.6)).pod]
    scene._install_geom(quads, list(scene._instances)[:scene.n_instances], list(scene._inst_spheres)[:scene.pod.n_inst_spheres],
                        list(scene._inst_quads)[:scene.pod.n_inst_quads])
    if moving:
        for i in range(1, scene.n_spheres, 3):
            scene._spheres[i].velocity[1] = 3.0
    cam = view()
    if moving:
        cam.shutter = 1.0 / 30.0
    return scene, cam


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("integ,samp,flags", CONFIGS)
def test_triangle_build_against_the_oracle(gpu, moving, integ, samp, flags):
    scene, cam = tri_scene(moving)
    ref, st = against_oracle(gpu, scene, cam, params(integ, samp, flags), (LIST, NODES0, NODES1), 8, moving, True)
    assert st.segments > 0 and np.isfinite(ref).mean() > 0.99


@pytest.mark.parametrize("what", ["degenerate_first", "far", "nan_vertex"])
def test_triangle_fallback_scenes_against_the_oracle(gpu, what):
    if what == "degenerate_first":
        extra = [R.Triangle.new((0.5, 0.5, 0.5), (1, 1, 1), (2, 2, 2), R.SCATTER_M, (1, 0, 0))]
    elif what == "far":
        extra = [R.Triangle.new((1e30, 0, 0), (1, 0, 0), (0, 1, 0), R.SCATTER_M, (1, 0, 0))]
    else:
        extra = [R.Triangle.new((np.nan, 0, 0), (1, 0, 0), (0, 1, 0), R.SCATTER_M, (1, 0, 0))]
    scene, cam = mixed_scene(extra), view()
    for integ, samp, flags in CONFIGS[:4]:
        p = params(integ, samp, flags, spp=4)
        ref, st_ref = O.render(cam, scene, p, THREADS)
        gpu.set_scene(scene)
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        try:
            for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):            # both walk the triangle list here (triangle_bvh_validate: list_walk)
                p.accel = accel
                img, st = gpu.render(cam, p)
                assert exact(img, ref), (what, integ, accel, where(img, ref))
                assert st.segments == st_ref.segments and st.quad_tests == st_ref.quad_tests, (what, integ, accel)
        finally:
            gpu.set_option(R.OPT_LIST_WALK_MAX, 48)


def test_triangle_partitions_against_the_oracle(gpu):
    scene, cam = tri_scene(True)
    p = params(R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, 0, 72, 56, 4)
    p.row_block, p.part_index, p.part_count = 8, 1, 3
    part_ref, st_part = O.render(cam, scene, p, THREADS)
    assert part_ref.shape[0] == R.lib().rtw_part_rows(56, 8, 1, 3) < 56
    gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
    for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
        p.accel = accel
        img, st = gpu.render(cam, p)
        assert exact(img, part_ref) and st.segments == st_part.segments and st.rows == st_part.rows, accel
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    ref, st_ref = O.render(cam, scene, p, THREADS)
    with R.MultiRenderer([0, 0, 0]) as m:                       # rtw_mgpu: three contexts on GPU 0, rows dealt in blocks of 8
        m.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
        for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
            p.accel = accel
            img, tot, _ = m.render(cam, p)
            assert exact(img, ref) and tot.segments == st_ref.segments, accel


# ---- noise: the fourteen kernels of the noise build ---------------------------------------------------------------------------------
def noise_field(moving, geom):
    """130 spheres in the shape of test_every_build_of_the_traversal_kernel's (geometry small enough for LDS): an image-textured ground with
    noise, textured small spheres with noise (every fourth of them on a texture with scale 0: p / 0 is inf or NaN), every third moving
    when `moving`.  geom: plus a noised textured quad and a rotated, translated box whose member sphere and walls carry noise (local points)."""
    rng = np.random.default_rng(31 + 2 * moving + geom)
    ground = rng.uniform(0.1, 0.9, size=(6, 9, 3)).astype(f32)
    small = rng.uniform(0.2, 1.0, size=(3, 5, 3)).astype(f32)
    mats = [R.SCATTER_M, R.METALLIC_M, R.GLASS_M, R.FUZZY3_M]
    spheres = [R.Sphere.new_with_texture((0, -1000, 0), 1000.0, None, R.SCATTER_M, 0)]
    for i in range(129):
        c = (float(rng.uniform(-5, 5)), float(rng.uniform(0.15, 1.0)), float(rng.uniform(-6, 1)))
        vel = (0.0, float(rng.uniform(0.0, 6.0)), 0.0) if (moving and i % 3 == 0) else None
        r = float(rng.uniform(0.1, 0.3))
        if i % 2 == 0:
            spheres.append(R.Sphere.new_with_texture(c, r, tuple(rng.uniform(0.5, 1.0, 3)), mats[i % 4], 2 if i % 8 == 0 else 1, velocity=vel))
        else:
            spheres.append(R.Sphere.with_albedo(c, r, tuple(rng.uniform(0.3, 0.9, 3)), mats[i % 4], velocity=vel))
    textures = [ground, small, np.full((1, 1, 3), 0.8, f32)]
    noise = {0: (R.PerlinNoise(5), 0.7), 1: (R.PerlinNoise(6), 0.15), 2: (R.PerlinNoise(7), 0.0)}
    quads, instances = (), ()
    if geom:
        quads = [R.Quad.new((-3.0, 0.02, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), R.SCATTER_M, tex_index=1)]
        member = R.Sphere.new_with_texture((0.5, 0.5, 0.5), 0.35, (1.0, 1.0, 1.0), R.SCATTER_M, 1)
        walls = [R.Quad.new((0, 0, 1), (1, 0, 0), (0, 1, 0), R.SCATTER_M, tex_index=0),
                 R.Quad.new((1, 0, 0), (0, 0, 1), (0, 1, 0), R.SCATTER_M, tex_index=1)]
        box = R.Instance.new([member], walls)
        box.rotate((0.0, 0.6, 0.2)); box.translate((1.5, 0.1, -1.0))
        instances = [box]
    scene = R.Scene(spheres, textures=textures, quads=quads, instances=instances, noise=noise)
    vp = R.Viewport.new_from_res(64, 48, 9, 6, 1.0, vfov=45.0, origin=(0.0, 1.6, 6.0), direction=(0.0, -0.2, -1.0), lens_radius=0.03)
    if moving:
        vp.shutter_speed, vp.fps = 1.0 / 30.0, 30.0
    return scene, vp.camera()


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("geom", [False, True])
@pytest.mark.parametrize("integ,samp,flags", NOISE_CONFIGS)
def test_noise_build_against_the_oracle(gpu, moving, geom, integ, samp, flags):
    scene, cam = noise_field(moving, geom)
    builds = (LIST, NODES0, NODES1) if geom else (LIST, NODES0, NODES1, NODES2)
    ref, st = against_oracle(gpu, scene, cam, params(integ, samp, flags), builds, 7, moving, geom)
    if integ in (R.INTEGRATOR_GRADIENT, R.INTEGRATOR_BG_COLOR):     # (NORMAL and FLAG read no texture)
        assert np.isnan(ref).any(axis=2).sum() > 0 and np.isfinite(ref).all(axis=2).mean() > 0.5     # the scale-0 texture is in view


def test_noised_c5_against_the_oracle(gpu):
    _, noised, cam, p = noised_c5()
    p.gamma = 1.0
    assert any(noised._spheres[i].velocity[1] != 0 for i in range(noised.n_spheres)) and noised.n_quads == noised.n_instances == 0
    ref, st = against_oracle(gpu, noised, cam, p, (LIST, NODES0, NODES1), 7, True, False)
    assert st.nan_pixels > 0 and np.isfinite(ref).all(axis=2).mean() > 0.1


def test_noise_seen_after_a_metal_bounce(gpu):
    """Noised textured spheres behind the camera, seen only in a mirror sphere that fills the view: the noise of the second hit."""
    tex = np.random.default_rng(8).uniform(0.2, 1.0, size=(4, 8, 3)).astype(f32)
    spheres = [R.Sphere.with_albedo((0.0, 0.0, -4.0), 3.0, (0.95, 0.95, 0.95), R.METALLIC_M)]
    rng = np.random.default_rng(9)
    for k in range(60):
        c = (float(rng.uniform(-4, 4)), float(rng.uniform(-3, 3)), float(rng.uniform(3.0, 6.0)))
        spheres.append(R.Sphere.new_with_texture(c, 0.5, (1.0, 1.0, 1.0), R.SCATTER_M, 0))
    scene = R.Scene(spheres, textures=[tex], background=(0.2, 0.3, 0.4), noise={0: (R.PerlinNoise(12), 0.25)})
    vp = R.Viewport.new_from_res(64, 48, 9, 4, 1.0, vfov=50.0, origin=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0))
    cam = vp.camera()
    plain = R.Scene(spheres, textures=[tex], background=(0.2, 0.3, 0.4))
    for integ in (R.INTEGRATOR_GRADIENT, R.INTEGRATOR_BG_COLOR):
        p = params(integ, R.SAMPLER_ROW, 0)
        ref, _ = against_oracle(gpu, scene, cam, p, (LIST, NODES0, NODES1, NODES2), 7, False, False)
        without, _ = O.render(cam, plain, p, THREADS, device_uv=True)
        assert not np.array_equal(ref, without)                    # the noise reaches the image
