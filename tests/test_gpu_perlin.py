"""Perlin noise of image textures on the GPU (the noise build, SPEC 7): the device's noise against the host's, the noise multiplier at
the right point for spheres, quads and instance members, invariance of the image under the closest-hit strategy and the device split,
the reference's noise_test scene, and the error paths."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.test_oracle_golden import small_view
from tests.test_perlin_cpu import point_set

pytestmark = pytest.mark.gpu

F = np.float32
SCALE = 0.5


def test_device_noise_equals_host_noise_bitwise(gpu):
    perlin = R.PerlinNoise(77)
    pts = point_set(seed=11)
    for depth in range(0, 8):
        host = perlin.noise(pts) if depth == 0 else perlin.turb(pts, depth)
        dev = gpu.perlin_eval(perlin, pts, depth)
        assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), (depth, np.flatnonzero(host.view(np.uint32) != dev.view(np.uint32))[:5])


# ---- the ratio tests: one white-textured Lambert object, NO_RAND sampler, depth 2, gamma 1 -----------------------------------------------
# A lit pixel is albedo * sky(scatter direction); the noise multiplies the albedo (1 without noise) and draws no random number, so the
# noised image is the plain one times noise(p / scale) at the pixel's hit point p.
ROT_Y = 0.4
TRANS = np.array([5.3, 0.0, 0.0])


def rot_y(v, b):        # Vec3::rotated((0, b, 0)) (vec3.rs:161-181 with a = c = 0): a proper rotation about y
    v = np.asarray(v, np.float64)
    return np.array([v[0] * np.cos(b) + v[2] * np.sin(b), v[1], -v[0] * np.sin(b) + v[2] * np.cos(b)])


def to_local(w):
    return rot_y(np.asarray(w, np.float64) - TRANS, -ROT_Y)


def camera_rays(v):
    cam = v.cam
    o = np.array(cam.origin, F)
    p00, du, dv = np.array(cam.pixel00, F), np.array(cam.delta_u, F), np.array(cam.delta_v, F)
    rays = {}
    for j in range(v.height):
        for i in range(v.width):
            rays[(j, i)] = (o.astype(np.float64), ((p00 + du * F(i)) + dv * F(j)).astype(np.float64))
    return rays


SPHERE_C, SPHERE_R = np.array([0.0, 0.0, -1.5]), 0.5
QUAD_O, QUAD_U, QUAD_V = np.array([-1.0, -0.6, -1.5]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 1.2, 0.0])


def hit_sphere(o, d):
    oc = o - SPHERE_C
    a, b, c = d @ d, oc @ d, oc @ oc - SPHERE_R * SPHERE_R
    disc = b * b - a * c
    if disc < 1e-3 * a:                                   # (keep off the silhouette)
        return None
    return o + d * ((-b - np.sqrt(disc)) / a)


def hit_quad(o, d):
    n = np.cross(QUAD_U, QUAD_V)
    t = (n @ QUAD_O - n @ o) / (n @ d)
    p = o + d * t
    w = n / (n @ n)
    planar = p - QUAD_O
    alfa, beta = w @ np.cross(planar, QUAD_V), w @ np.cross(QUAD_U, planar)
    return p if 0.02 < alfa < 0.98 and 0.02 < beta < 0.98 else None


def build_ratio_scene(kind, noise):
    img = np.ones((1, 1, 3), F)
    nz = {0: noise} if noise else None
    if kind == "sphere":
        return R.Scene([R.Sphere.new_with_texture(tuple(SPHERE_C), SPHERE_R, (1.0, 1.0, 1.0), R.SCATTER_M, 0)], textures=[img], noise=nz)
    if kind == "quad":
        return R.Scene((), textures=[img], quads=[R.Quad.new(tuple(QUAD_O), tuple(QUAD_U), tuple(QUAD_V), R.SCATTER_M, tex_index=0)], noise=nz)
    # the same object as a member of an instance rotated about y and translated far along x, so that its LOCAL points are far from the world ones
    if kind == "inst_sphere":
        member = R.Sphere.new_with_texture(tuple(float(x) for x in to_local(SPHERE_C)), SPHERE_R, (1.0, 1.0, 1.0), R.SCATTER_M, 0)
        inst = R.Instance.new([member], [])
    else:
        lo, lu, lv = to_local(QUAD_O), rot_y(QUAD_U, -ROT_Y), rot_y(QUAD_V, -ROT_Y)
        inst = R.Instance.new([], [R.Quad.new(tuple(lo), tuple(lu), tuple(lv), R.SCATTER_M, tex_index=0)])
    inst.translate(tuple(TRANS))
    inst.rotate((0.0, ROT_Y, 0.0))
    return R.Scene((), textures=[img], instances=[inst], noise=nz)


@pytest.mark.parametrize("kind", ["sphere", "quad", "inst_sphere", "inst_quad"])
def test_noise_multiplies_the_albedo_at_the_hit_point(gpu, kind):
    perlin = R.PerlinNoise(2024)
    v = R.Viewport.new_from_res(48, 27, 1, 2, 1.0)
    p = v.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_NO_RAND, R.ACCEL_BRUTE)
    cam = v.camera()
    gpu.set_scene(build_ratio_scene(kind, None))
    plain, st_plain = gpu.render(cam, p)
    plain = plain.copy()
    gpu.set_scene(build_ratio_scene(kind, (perlin, SCALE)))
    noised, st_noised = gpu.render(cam, p)
    assert st_noised.segments == st_plain.segments        # noise draws no random number
    hit = hit_sphere if "sphere" in kind else hit_quad
    world, local, pix = [], [], []
    for (j, i), (o, d) in camera_rays(v).items():
        w = hit(o, d)
        if w is None:
            continue
        world.append(w); local.append(to_local(w)); pix.append((j, i))
    assert len(pix) > 50
    js, is_ = np.array(pix).T
    a, b = plain[js, is_], noised[js, is_]
    assert np.all(a > 0.0)                                 # every such pixel is lit: sky through a white albedo
    at = lambda pts: perlin.noise((np.array(pts) / SCALE).astype(F)).astype(np.float64)
    n_world, n_local = at(world), at(local)
    n_true = n_local if kind.startswith("inst") else n_world
    err = np.abs(b - a * n_true[:, None]).max(axis=1)
    assert np.all(err <= 1e-4 * a.max(axis=1) + 1e-6), (kind, err.max())
    if kind.startswith("inst"):                          # ... and NOT the noise at the world point
        err_w = np.abs(b - a * n_world[:, None]).max(axis=1)
        assert np.mean(err_w <= 1e-4 * a.max(axis=1) + 1e-6) < 0.1, kind


# ---- invariance on a noised C5 frame ----------------------------------------------------------------------------------------------------
def noised_c5():
    scene, cam, p = small_view(R.SCENE_C5, 64, 36, 4)
    t = list(scene._textures)[0]
    ground = np.array(scene._texels[t.texel_offset:t.texel_offset + t.row * t.col], F).reshape(t.col, t.row, 3)
    spheres = list(scene._spheres)[:scene.n_spheres]
    for s in spheres:                                      # the big Lambert sphere reads a second texture, with scale 0: p / 0 -> inf / NaN
        if s.radius == 1.0 and s.center[0] < -3.0:
            s.tex = 1
    textures = [ground, np.full((1, 1, 3), 0.9, F)]
    perlin = R.PerlinNoise(5)
    plain = R.Scene(spheres, textures=textures)
    noised = R.Scene(spheres, textures=textures, noise={0: (perlin, 0.7), 1: (R.PerlinNoise(6), 0.0)})
    return plain, noised, cam, p


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_noised_c5_invariance(gpu):
    plain, noised, cam, p = noised_c5()
    t0, t1 = cam.time0, cam.time0 + cam.shutter
    gpu.set_scene(plain, t0, t1)
    ref, st_ref = gpu.render(cam, p)
    ref = ref.copy()
    gpu.set_scene(noised, t0, t1)
    gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
    p.accel = R.ACCEL_BVH
    bvh, st_bvh = gpu.render(cam, p)
    bvh = bvh.copy()
    assert st_bvh.node_tests > 0
    p.accel = R.ACCEL_BRUTE
    brute, st_brute = gpu.render(cam, p)
    brute = brute.copy()
    assert same(bvh, brute)
    assert st_bvh.segments == st_brute.segments == st_ref.segments
    assert st_bvh.nan_pixels == st_brute.nan_pixels == int(np.isnan(bvh).any(axis=2).sum()) > 0
    assert not same(bvh, ref)
    fin = ~np.isnan(bvh).any(axis=2)
    assert fin.sum() > 0.1 * fin.size
    # clearing the noise, or a fresh scene, gives the plain image back bit for bit
    gpu.set_texture_noise()
    cleared, _ = gpu.render(cam, p)
    assert same(cleared, ref)
    gpu.set_scene(noised, t0, t1)
    assert same(gpu.render(cam, p)[0], brute)
    assert R.lib().rtw_ctx_set_scene(gpu._h, C.byref(noised.pod), t0, t1) == 0      # the C call alone: set_scene clears the noise
    assert same(gpu.render(cam, p)[0], ref)
    gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    # two contexts on one GPU through rtw_mgpu: the same image as one context
    p.accel = R.ACCEL_BVH
    with R.MultiRenderer([0, 0]) as m:
        m.set_scene(noised, t0, t1)
        m.set_option(R.OPT_LIST_WALK_MAX, 0)
        multi, tot, _ = m.render(cam, p)
    assert same(multi, bvh) and tot.segments == st_bvh.segments


# ---- the reference's noise_test (Rust/src/viewport/texture_test.rs:143-214), built here ---------------------------------------------
def test_reference_noise_test_scene(gpu):
    img, entry = R.texture_from_color_noise((1.0, 1.0, 1.0), 0.01, seed=31)
    spheres = [R.Sphere.new((-1.0, 0.0, -1.0), 0.5, (0.8, 0.8, 0.8), R.METALLIC_M),
               R.Sphere.new((1.0, 0.0, -1.0), 0.5, (0.8, 0.6, 0.2), R.METALLIC_M),
               R.Sphere.new_with_texture((0.0, -100.5, -1.0), 100.0, (1.0, 1.0, 1.0), R.SCATTER_M, 0),
               R.Sphere.new((0.0, 0.0, -1.0), 0.5, (0.8, 0.8, 0.0), R.SCATTER_M)]
    scene = R.Scene(spheres, textures=[img], noise={0: entry})
    v = R.Viewport.new_from_res(400, 225, 100, 10, 2.0)
    v.maxt = 1e3                                            # ray_color_d (main.rs:17-46)
    cam = v.camera()
    gpu.set_scene(scene)
    out = {}
    for accel, walk_max in ((R.ACCEL_BVH, 0), (R.ACCEL_BRUTE, 48)):
        gpu.set_option(R.OPT_LIST_WALK_MAX, walk_max)
        im, st = gpu.render(cam, v.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_STRATIFIED, accel))
        out[accel] = (im.copy(), st)
    gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    (a, sa), (b, sb) = out[R.ACCEL_BVH], out[R.ACCEL_BRUTE]
    assert a.shape == (225, 400, 3) and sa.node_tests > 0 and sb.node_tests == 0
    assert same(a, b) and sa.segments == sb.segments
    # a negative mean under gamma 2 is NaN, in the reference too
    assert sa.nan_pixels == int(np.isnan(a).any(axis=2).sum())
    assert np.isfinite(a).any()
    # the one-shot Viewport path passes the noise on as well
    assert same(v.render(R.INTEGRATOR_GRADIENT, scene), a)


# ---- error paths ------------------------------------------------------------------------------------------------------------------------
def test_noise_error_paths(rtw):
    L = R.lib()
    perlin = R.PerlinNoise(1)
    per = (R.RtwTextureNoise * 1)(R.RtwTextureNoise(0, 1.0))
    with R.Renderer(0) as r:
        assert L.rtw_ctx_set_texture_noise(r._h, C.byref(perlin.pod), 1, per, 1) == -6           # RTW_E_NO_SCENE
        scene = build_ratio_scene("sphere", (perlin, SCALE))
        r.set_scene(scene)
        v = R.Viewport.new_from_res(16, 9, 4, 2, 1.0)
        with pytest.raises(R.RtwError) as e:
            r.render(v.camera(), v.params(R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, R.ACCEL_BRUTE))
        assert e.value.status == -5                                                               # RTW_E_UNSUPPORTED
        r.render(v.camera(), v.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, R.ACCEL_BRUTE))      # (the others render)
        per2 = (R.RtwTextureNoise * 2)(R.RtwTextureNoise(0, 1.0), R.RtwTextureNoise(-1, 1.0))
        assert L.rtw_ctx_set_texture_noise(r._h, C.byref(perlin.pod), 1, per2, 2) == -1          # n_textures != the scene's
        bad = (R.RtwTextureNoise * 1)(R.RtwTextureNoise(1, 1.0))
        assert L.rtw_ctx_set_texture_noise(r._h, C.byref(perlin.pod), 1, bad, 1) == -1           # table index out of range
        assert L.rtw_ctx_set_texture_noise(r._h, None, 0, None, 1) == -1
        assert L.rtw_ctx_set_texture_noise(r._h, None, 0, None, 0) == 0                           # NULL / 0: cleared
        r.render(v.camera(), v.params(R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, R.ACCEL_BRUTE))     # no noise: Rust2 renders again
