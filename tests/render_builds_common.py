"""Scenes, cases and oracle frames of tests/test_gpu_render_builds.py (the GPU side) and tests/test_render_builds_cpu.py (the conditions on
these inputs, checked with the oracle alone).

The scene is test_every_build_of_the_traversal_kernel's: a textured ground and 129 small spheres of four materials, small enough for the
sphere geometry to fit in LDS and large enough to be given to the tree; every third small sphere moves when `moving`.  Here every eighth
small sphere also emits and the background is not black, so that the terms of RTW_INTEGRATOR_BG_COLOR and _RUST2 reach pixels.  geom: plus
a floor quad in front of the field, a wall quad inside it (spheres stand in front of parts of it), a rotated and translated box, and a
constant-density box (the oracle's Instance::collision_normal draws the medium's distance whatever the integrator, so every integrator gets
it)."""
import numpy as np

import rtw_amd as R
from tests import builds_common as B
from tests import oracle_binding as O

WIDTH, HEIGHT, SPP, DEPTH = 112, 64, 4, 8          # 4 spp: a square count, for the stratified and centres samplers
THREADS = 16
BACKGROUND = (0.25, 0.35, 0.6)

# (name, SPEC, integrator, sampler, flags)
SPHERE_CONFIGS = [("demo", 4, R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, 0),
                  ("rust2", 5, R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 0),
                  ("serial", 6, R.INTEGRATOR_GRADIENT, R.SAMPLER_STRATIFIED, 0)]
GEOM_CONFIGS = [("common", 2, R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, 0)] + SPHERE_CONFIGS + [
    ("generic-normal", 0, R.INTEGRATOR_NORMAL, R.SAMPLER_ROW, 0),
    ("generic-chunk-sums", 0, R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, R.FLAG_CHUNK_SUMS),
    ("generic-cpp", 0, R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, R.FLAG_CPP)]
CONFIGS = {False: SPHERE_CONFIGS, True: GEOM_CONFIGS}
# nodes: None the list walk; 0 the tree under RTW_FLAG_GLOBAL_NODES; 1 RTW_OPT_LDS_GEOM 0; 2 RTW_OPT_LDS_GEOM 1 (no GEOM build has it)
PATHS = {False: (None, 0, 1, 2), True: (None, 0, 1)}


def cases():
    """[(id, declared tag, geom, moving, config, nodes)]"""
    out = []
    for geom in (False, True):
        for cfg in CONFIGS[geom]:
            for moving in (False, True):
                for nodes in PATHS[geom]:
                    tag = B.tag(moving, nodes, cfg[1], geom)
                    out.append((f"{tag}-{cfg[0]}", tag, geom, moving, cfg, nodes))
    return out


CASES = cases()

_scenes, _frames = {}, {}


def scene_and_camera(geom, moving):
    """(Scene, RtwCamera, Viewport) -- built once, never changed."""
    key = (bool(geom), bool(moving))
    if key in _scenes:
        return _scenes[key]
    rng = np.random.default_rng(5 + 2 * moving + 1)                              # the textured scenes of test_every_build_of_the_traversal_kernel
    tex = rng.uniform(0.1, 0.9, size=(4, 6, 3)).astype(np.float32)
    mats = [R.SCATTER_M, R.METALLIC_M, R.GLASS_M, R.FUZZY3_M]
    spheres = [R.Sphere.new_with_texture((0, -1000, 0), 1000.0, None, R.SCATTER_M, 0)]
    for i in range(129):
        c = (float(rng.uniform(-5, 5)), float(rng.uniform(0.15, 1.0)), float(rng.uniform(-6, 1)))
        vel = (0.0, float(rng.uniform(0.0, 6.0)), 0.0) if (moving and i % 3 == 0) else None
        s = R.Sphere.with_albedo(c, float(rng.uniform(0.1, 0.3)), tuple(rng.uniform(0.3, 0.9, 3)), mats[i % 4], velocity=vel)
        if i % 8 == 4:                                                           # (a diffuse one: 4 % 4 == 0)
            for k, e in enumerate((4.0, 3.0, 2.0)):
                s.pod.emitted[k] = e
        spheres.append(s)
    quads, instances = (), ()
    if geom:
        quads = [R.Quad.new((-1.6, 0.02, 2.0), (2.6, 0.0, 0.0), (0.0, 0.0, 2.2), R.SCATTER_M, (0.8, 0.3, 0.3)),
                 R.Quad.new((-2.5, 0.0, -3.0), (5.0, 0.0, 0.0), (0.0, 2.4, 0.0), R.METALLIC_M, (0.9, 0.9, 0.7), emitted=(0.3, 0.3, 0.5))]
        box = R.Instance.new_box((0, 0, 0), (1.2, 1.2, 1.2), (0.9, 0.8, 0.4), R.SCATTER_M)
        box.rotate((0.0, 0.5, 0.1)); box.translate((1.8, 0.0, 2.2))
        smoke = R.Instance.new_box((0, 0, 0), (1.2, 1.2, 1.2), (0.2, 0.2, 0.2), R.SCATTER_M)
        smoke.translate((-3.4, 0.0, 2.0)); smoke.const_density(0.8)
        instances = [box, smoke]
    scene = R.Scene(spheres, textures=[tex], background=BACKGROUND, quads=quads, instances=instances)
    vp = R.Viewport.new_from_res(WIDTH, HEIGHT, SPP, DEPTH, 1.0, vfov=45.0, origin=(0.0, 1.6, 6.0), direction=(0.0, -0.2, -1.0), lens_radius=0.03)
    if moving:
        vp.shutter_speed, vp.fps = 1.0 / 30.0, 30.0
    _scenes[key] = (scene, vp.camera(), vp)
    return _scenes[key]


def view(geom, moving, cfg):
    """(Scene, RtwCamera) of a case.  RTW_SAMPLER_CENTRES reads Rust2's camera (left_top and full-viewport deltas: camera2_new), the other
    samplers the Viewport's; both look at the field from the same place.  CENTRES and STRATIFIED trace every ray at time 0 (Ray::new): their
    MOVING kernels run with the spheres where they start."""
    scene, cam, _ = scene_and_camera(geom, moving)
    if cfg[3] == R.SAMPLER_CENTRES:
        cam2 = R.camera2_new(WIDTH / HEIGHT, (0.0, 1.6, 6.0), (0.0, 1.0, 0.0), (0.0, -0.2, -1.0), 45.0, 0.03)
        cam2.time0, cam2.shutter = cam.time0, cam.shutter
        cam = cam2
    return scene, cam


def params(geom, moving, cfg):
    _, _, vp = scene_and_camera(geom, moving)
    p = vp.params(cfg[2], cfg[3])
    p.gamma, p.flags = 1.0, cfg[4]
    return p


def oracle_frame(geom, moving, cfg):
    """The oracle's frame with the device's texel choice (RTW_ORACLE_FLAG_DEVICE_UV) and its counters: one per (scene, configuration),
    computed once and shared."""
    key = (bool(geom), bool(moving), cfg[0])
    if key not in _frames:
        scene, cam = view(geom, moving, cfg)
        ref, st = O.render(cam, scene, params(geom, moving, cfg), threads=THREADS, device_uv=True)
        ref.setflags(write=False)
        _frames[key] = (ref, st)
    return _frames[key]
