"""The surface buffers (rtw_ctx_scene_surface, rtw_ctx_surface_map, rtw_pixel_rays; include/rtw.h "surface buffers"):
t, idx and normal are scene_hits' bits on scenes with all four groups, placed meshes and quaternion instances; RTW_ACCEL_BVH equals
RTW_ACCEL_BRUTE in albedo, emitted and material under every fall-back; the record is pinned to the CPU oracle through renders whose
frame IS emitted + albedo of the first hit; surface_map against depth_map and against scene_surface over pixel_rays; misses, a skipped
medium, NULL outputs and the refusals."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import oracle_binding as O
from tests import quat_common as QC
from tests.test_gpu_scene_hits import MAXT, MINT, geom_rays, geom_scene

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("t", "idx", "normal", "albedo", "emitted", "material")


def same(a, b):
    """The same bits, or NaN on both sides (a NaN ray's t)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def assert_hits(gpu, rays, mint, maxt, accel, integrator=R.INTEGRATOR_BG_COLOR, time=0.0):
    s = gpu.scene_surface(rays, mint, maxt, integrator, time=time, accel=accel)
    t, idx, nrm, _ = gpu.scene_hits(rays, mint, maxt, time=time, accel=accel, normals=True)
    assert same(s["t"], t) and same(s["idx"], idx) and same(s["normal"], nrm)
    miss = s["idx"] < 0
    assert not s["albedo"][miss].any() and not s["emitted"][miss].any() and not s["material"][miss].any()
    return s


# ---- 1. t, idx, normal are scene_hits' ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_four_groups_agree_with_scene_hits(gpu, accel):
    scene = geom_scene()
    gpu.set_scene(scene)
    s = assert_hits(gpu, geom_rays(), MINT, MAXT, accel)
    ns, nq, ni = scene.n_spheres, scene.n_quads, scene.n_instances
    idx = s["idx"]
    groups = [np.sum((idx >= 0) & (idx < ns)), np.sum((idx >= ns) & (idx < ns + nq)), np.sum((idx >= ns + nq) & (idx < ns + nq + ni)),
              np.sum(idx >= ns + nq + ni), np.sum(idx < 0)]
    assert min(groups) > 20, groups
    # the record of each group, from what the scene was made of (tests/test_gpu_scene_hits.py geom_scene)
    assert (s["albedo"][(idx >= 0) & (idx < ns)] == F(0.5) * F(0.5)).all()              # the spheres' tex_color * col_mod
    assert (s["material"][idx == 1] == np.array(R.METALLIC_M, F)).all() and (s["material"][idx == 2] == np.array(R.GLASS_M, F)).all()
    assert (s["albedo"][idx == ns + nq] == F(0.7)).all()                                # the box
    assert (s["albedo"][idx == ns + nq + 1] == F(0.5) * F(0.5)).all()                   # the pair of spheres
    assert (s["albedo"][idx >= ns + nq + ni] == F(1.0)).all() and not s["emitted"].any()


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_placed_meshes_agree_with_scene_hits(gpu, accel):
    ms = MI.MeshScene(MI.standard_mesh(), MI.standard_placements(), background=(1.0, 1.0, 1.0))
    ms.install(gpu)
    try:
        s = assert_hits(gpu, MI.standard_rays(), MI.MINT, MI.MAXT, accel, R.INTEGRATOR_RUST2)
        hit = s["idx"] >= 0
        assert 0.25 < hit.mean() < 0.75
        colours = {tuple(np.asarray(t["color"], F) * F(1.0)) for t in ms.T.tris}
        assert {tuple(c) for c in s["albedo"][hit]} <= colours and len({tuple(c) for c in s["albedo"][hit]}) > 10
    finally:
        gpu.set_scene(geom_scene())


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_quaternion_instances_agree_with_scene_hits(gpu, accel):
    g = QC.golden()
    qs = QC.fixture_scene(g)
    qs.install(gpu)
    try:
        o, d = QC.depth_rays(QC.camera(g, 48, 36), 48, 36)
        s = assert_hits(gpu, np.concatenate([o, d], 1).astype(F), g["mint"], g["maxt"], accel, R.INTEGRATOR_RUST2)
        box = s["idx"] == 0
        assert 50 < box.sum() < len(box)
        assert (s["albedo"][box] == (np.asarray(g["color"], F) * F(1.0))).all() and (s["emitted"][box] == np.asarray(g["emitted"], F)).all()
    finally:
        gpu.set_scene(geom_scene())


# ---- 2. RTW_ACCEL_BVH equals RTW_ACCEL_BRUTE under every fall-back ---------------------------------------------------------------------------
@pytest.mark.parametrize("list_walk_max", [0, 48])
def test_bvh_equals_brute_under_the_sphere_fallbacks(gpu, list_walk_max):
    rng = np.random.default_rng(8)
    tex = [rng.random((5, 7, 3)).astype(F)]
    sp = [R.Sphere.new_with_texture((float(x), float(y), -6.0), 0.45, (0.9, 0.8, 0.7), R.SCATTER_M, 0) if (x + y) % 2 else
          R.Sphere.new((float(x), float(y), -6.0), 0.45, (0.1 * (x + 5), 0.5, 0.3), R.METALLIC_M) for x in range(-3, 4) for y in range(-3, 3)]
    scene = R.Scene(sp, textures=tex)
    assert scene.n_spheres == 42                                  # at most the default of 48: the tree at 0, the list at the default
    rays = np.concatenate([np.zeros((3000, 3)), rng.uniform((-4.0, -4.0, -6.0), (4.0, 3.0, -6.0), (3000, 3))], 1).astype(F)
    gpu.set_scene(scene)
    gpu.set_option(R.OPT_LIST_WALK_MAX, list_walk_max)
    try:
        for integrator in (R.INTEGRATOR_BG_COLOR, R.INTEGRATOR_RUST2):
            a = assert_hits(gpu, rays, MINT, MAXT, R.ACCEL_BRUTE, integrator)
            b = assert_hits(gpu, rays, MINT, MAXT, R.ACCEL_BVH, integrator)
            assert all(same(a[k], b[k]) for k in KEYS), integrator
            assert (b["stats"].node_tests > 0) == (list_walk_max == 0) and a["stats"].node_tests == 0
            assert len(np.unique(a["albedo"], axis=0)) > 25 and 500 < (a["idx"] >= 0).sum() < 2900
    finally:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)


@pytest.mark.parametrize("mesh_list_max", [0, 4294967295])
def test_bvh_equals_brute_under_the_mesh_fallbacks(gpu, mesh_list_max):
    ms = MI.MeshScene(MI.standard_mesh(), MI.standard_placements())
    ms.install(gpu)
    gpu.set_option(R.OPT_MESH_LIST_MAX, mesh_list_max)
    try:
        rays = MI.standard_rays()
        a = assert_hits(gpu, rays, MI.MINT, MI.MAXT, R.ACCEL_BRUTE, R.INTEGRATOR_RUST2)
        b = assert_hits(gpu, rays, MI.MINT, MI.MAXT, R.ACCEL_BVH, R.INTEGRATOR_RUST2)
        assert all(same(a[k], b[k]) for k in KEYS)
    finally:
        gpu.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)
        gpu.set_scene(geom_scene())


# ---- 3. the record against the oracle --------------------------------------------------------------------------------------------------------
# One convex object, a mirror-like material, background 1 1 1, RTW_SAMPLER_NO_RAND, depth 2, gamma 1.  The ray scattered off a convex body
# meets nothing else, so under RTW_INTEGRATOR_BG_COLOR (oracle/rtw_oracle.c ray_color_bg_iter: L = emitted * 1, thr = 1 * col_mod, then the
# miss adds background * thr) and under RTW_INTEGRATOR_RUST2 (ray_color_rust2_iter: the same with emmited and multiplied) the frame is
# emitted + albedo of the first hit exactly (x * 1 and 0 + x are exact), and the background where nothing is hit.  Metallicness 1: no
# cosine pdf is formed, so no path is poisoned.
W, H = 40, 30


def texture(seed, h=6, w=9):
    return np.random.default_rng(seed).random((h, w, 3)).astype(F)


def convex_scenes():
    white = (1.0, 1.0, 1.0)
    box = R.Instance.new_box((-0.6, -0.5, -0.4), (0.6, 0.5, 0.4), (0.7, 0.4, 0.2), R.METALLIC_M)
    box.rotate((0.0, 0.5, 0.0))        # about one axis: under a compound turn the oracle's mirror ray off one face meets the box again
    box.translate((0.1, 0.0, -3.0))
    vtx, faces = R.mesh_icosphere(1, centre=(0.0, 0.0, -3.0), radius=0.9)
    return {
        "textured sphere": (R.Scene([R.Sphere.new_with_texture((0.0, 0.0, -3.0), 1.0, (0.9, 0.8, 0.7), R.METALLIC_M, 0)], textures=[texture(1)],
                                    background=white), (R.INTEGRATOR_BG_COLOR,)),
        "textured quad": (R.Scene([], textures=[texture(2)], background=white,
                                  quads=[R.Quad.new((-1.0, -0.8, -3.0), (2.0, 0.3, -0.5), (0.1, 1.6, 0.2), R.METALLIC_M, emitted=(0.1, 0.2, 0.3), tex_index=0)]),
                          (R.INTEGRATOR_BG_COLOR,)),
        "box instance": (R.Scene([], background=white, instances=[box]), (R.INTEGRATOR_BG_COLOR,)),
        "rust2 sphere with emit_tex": (R.Scene([R.Sphere.new_with_texture((0.0, 0.0, -3.0), 1.0, white, R.METALLIC_M, 0)],
                                               textures=[texture(3), texture(4, 5, 8)], emission_images={0: 1}, background=white),
                                       (R.INTEGRATOR_RUST2,)),
        "textured triangle": (R.Scene([], textures=[texture(5), texture(6, 4, 4)], emission_images={0: 1}, background=white,
                                      triangles=[R.Triangle.new((-1.2, -0.9, -3.0), (2.4, 0.2, -0.4), (0.3, 1.9, 0.1), R.METALLIC_M,
                                                                emitted=(0.05, 0.0, 0.1), tex_index=0)]),
                              (R.INTEGRATOR_BG_COLOR, R.INTEGRATOR_RUST2)),
        "convex mesh": (R.Scene([], background=white, triangles=R.Triangle.from_mesh(vtx, faces, R.METALLIC_M, (0.3, 0.6, 0.9), (0.0, 0.1, 0.0))),
                        (R.INTEGRATOR_BG_COLOR, R.INTEGRATOR_RUST2)),
    }


CASES = [(name, integ) for name, (_, integs) in convex_scenes().items() for integ in integs]


@pytest.mark.parametrize("name,integrator", CASES, ids=[f"{n}-{i}" for n, i in CASES])
def test_albedo_plus_emitted_is_the_oracle_frame(gpu, name, integrator):
    scene = convex_scenes()[name][0]
    vp = R.Viewport.new_from_res(W, H, 1, 2, 1.0, vfov=50.0, origin=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0))
    cam = vp.camera()
    p = vp.params(integrator, R.SAMPLER_NO_RAND, R.ACCEL_BRUTE)
    p.mint, p.maxt = MINT, MAXT
    frame, _ = O.render(cam, scene, p, device_uv=True)
    gpu.set_scene(scene)
    try:
        rays = R.pixel_rays(cam, W, H, (0.0, 0.0))
        for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
            s = gpu.scene_surface(rays, MINT, MAXT, integrator, accel=accel)
            hit = (s["idx"] >= 0).reshape(H, W)
            assert 60 < hit.sum() < W * H - 60, hit.sum()
            got = (s["albedo"] + s["emitted"]).reshape(H, W, 3)
            assert same(got[hit], frame[hit]), name
            assert (frame[~hit] == 1.0).all() and not got[~hit].any()
            assert len(np.unique(s["albedo"][s["idx"] >= 0], axis=0)) > (1 if "textured" in name or "emit_tex" in name else 0)
            m = surface_map_of(gpu, cam, integrator, accel)
            assert all(same(m[k].reshape(s[k].shape), s[k]) for k in KEYS[1:])
    finally:
        gpu.set_scene(geom_scene())


def surface_map_of(gpu, cam, integrator, accel, offset=(0.0, 0.0)):
    m = gpu.surface_map(cam, W, H, MINT, MAXT, integrator, R.RAYS_PIXEL, offset, accel=accel)
    m["t"] = m["depth"]
    return m


def test_a_placed_convex_mesh_is_the_oracle_frame_of_the_same_triangles(gpu):
    """A placement at the origin with the identity quaternion moves nothing (o - 0 and the identity turn are exact): the placed mesh's
    record, formed in the placement's frame, is the oracle's of the same triangles in world space."""
    vtx, faces = R.mesh_icosphere(1, centre=(0.0, 0.0, -3.0), radius=0.9)
    tris = R.Triangle.from_mesh(vtx, faces, R.METALLIC_M, (0.3, 0.6, 0.9), (0.0, 0.1, 0.0))
    scene = R.Scene([], background=(1.0, 1.0, 1.0), triangles=tris)
    vp = R.Viewport.new_from_res(W, H, 1, 2, 1.0, vfov=50.0, origin=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0))
    p = vp.params(R.INTEGRATOR_RUST2, R.SAMPLER_NO_RAND, R.ACCEL_BRUTE)
    p.mint, p.maxt = MINT, MAXT
    frame, _ = O.render(vp.camera(), scene, p)
    gpu.set_scene(scene)
    gpu.set_mesh_instances([([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])])
    try:
        s = gpu.scene_surface(R.pixel_rays(vp.camera(), W, H), MINT, MAXT, R.INTEGRATOR_RUST2)
        hit = (s["idx"] >= 0).reshape(H, W)
        assert 60 < hit.sum() < W * H - 60 and (s["idx"][s["idx"] >= 0] == 0).all()          # the placement's index
        assert same((s["albedo"] + s["emitted"]).reshape(H, W, 3)[hit], frame[hit])
    finally:
        gpu.set_scene(geom_scene())


# ---- 4. surface_map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_surface_map_with_depth_rays_is_depth_map(gpu, accel):
    gpu.set_scene(geom_scene())
    cam = R.camera2_new(48 / 36, (0.0, 0.3, 1.5), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), 70.0, 0.0)
    depth, ids, nrm, _ = gpu.depth_map(cam, 48, 36, MINT, MAXT, accel=accel, ids=True, normals=True)
    m = gpu.surface_map(cam, 48, 36, MINT, MAXT, R.INTEGRATOR_BG_COLOR, R.RAYS_DEPTH_MAP, (0.3, 0.9), accel=accel)      # (the offset is not read)
    assert same(m["depth"], depth) and same(m["idx"], ids) and same(m["normal"], nrm)
    assert 100 < (ids < 0).sum() < ids.size - 100 and (m["depth"][ids < 0] == F(MAXT) * F(1.6)).all()
    s = gpu.scene_surface(R.depth_rays(cam, 48, 36), MINT, MAXT, accel=accel)
    assert all(same(m[k].reshape(s[k].shape), s[k]) for k in KEYS[1:])


@pytest.mark.parametrize("offset", [(0.0, 0.0), (0.5, 0.5), (0.25, 0.875)])
def test_surface_map_with_pixel_rays_is_scene_surface_over_pixel_rays(gpu, offset):
    gpu.set_scene(geom_scene())
    vp = R.Viewport.new_from_res(W, H, 1, 2, 1.0, vfov=75.0, origin=(0.0, 0.3, 1.5), direction=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0))
    cam = vp.camera()
    rays = R.pixel_rays(cam, W, H, offset)
    # rtw_pixel_rays is the rule as written, in f32
    o, p00, du, dv = (np.array(list(v), F) for v in (cam.origin, cam.pixel00, cam.delta_u, cam.delta_v))
    j, i = np.mgrid[0:H, 0:W]
    want = (p00 + du * (i[..., None].astype(F) + F(offset[0]))) + dv * (j[..., None].astype(F) + F(offset[1]))
    assert same(rays[:, 3:], want.reshape(-1, 3).astype(F)) and (rays[:, :3] == o).all()
    for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
        s = gpu.scene_surface(rays, MINT, MAXT, accel=accel)
        m = surface_map_of(gpu, cam, R.INTEGRATOR_BG_COLOR, accel, offset)
        hit = s["idx"] >= 0
        assert 100 < hit.sum() < hit.size - 100
        assert all(same(m[k].reshape(s[k].shape), s[k]) for k in KEYS[1:])
        assert same(m["depth"].reshape(-1)[hit], s["t"][hit]) and (m["depth"].reshape(-1)[~hit] == F(MAXT) * F(1.6)).all()
    if offset == (0.0, 0.0):                                      # RTW_SAMPLER_NO_RAND's ray: the NORMAL integrator's frame shows the same normals
        p = vp.params(R.INTEGRATOR_NORMAL, R.SAMPLER_NO_RAND, R.ACCEL_BRUTE)
        p.mint, p.maxt = MINT, MAXT
        frame = gpu.render(cam, p)[0]
        n = m["normal"]
        hit = m["idx"] >= 0
        assert same(frame[hit], ((n + F(1.0)) * F(0.5)).astype(F)[hit])


# ---- 5. the rest -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_a_constant_density_box_in_front_of_a_wall_reports_the_wall(gpu, accel):
    wall = R.Quad.new((-3.0, -3.0, -6.0), (6.0, 0.0, 0.0), (0.0, 6.0, 0.0), R.SCATTER_M, color=(0.2, 0.4, 0.6), emitted=(0.0, 0.5, 0.0))
    fog = R.Instance.new_box((-2.0, -2.0, -0.5), (2.0, 2.0, 0.5), (1.0, 1.0, 1.0), R.SCATTER_M)
    fog.translate((0.0, 0.0, -3.0))
    fog.const_density(0.7)
    gpu.set_scene(R.Scene([], quads=[wall], instances=[fog]))
    rng = np.random.default_rng(3)
    rays = np.concatenate([np.zeros((512, 3)), rng.uniform((-0.6, -0.6, -3.0), (0.6, 0.6, -3.0), (512, 3))], 1).astype(F)
    s = assert_hits(gpu, rays, MINT, MAXT, accel)
    assert (s["idx"] == 0).all() and (s["albedo"] == np.array([0.2, 0.4, 0.6], F)).all() and (s["emitted"] == np.array([0.0, 0.5, 0.0], F)).all()
    assert (s["material"] == np.array(R.SCATTER_M, F)).all()
    gpu.set_scene(geom_scene())


def test_null_outputs_and_refusals(gpu):
    scene = geom_scene()
    gpu.set_scene(scene)
    rays = geom_rays(257)
    n = len(rays)
    full = gpu.scene_surface(rays, MINT, MAXT)
    t, idx, alb = np.empty(n, F), np.empty(n, np.int32), np.full((n, 3), 7.0, F)
    call = R.lib().rtw_ctx_scene_surface
    args = lambda **k: [k.get("h", gpu._h), k.get("rays", rays.ctypes.data), k.get("n", n), 0.0, MINT, MAXT, k.get("accel", R.ACCEL_BVH),
                        k.get("integrator", R.INTEGRATOR_BG_COLOR), k.get("t", t.ctypes.data), k.get("idx", idx.ctypes.data), None,
                        k.get("albedo", alb.ctypes.data), None, None, None]
    assert call(*args()) == 0                                     # normal, emitted, material and stats NULL
    assert same(t, full["t"]) and same(idx, full["idx"]) and same(alb, full["albedo"])
    alb[:] = 7.0
    for bad in (dict(h=None), dict(rays=None), dict(n=0), dict(accel=2), dict(t=None), dict(idx=None), dict(albedo=None), dict(integrator=7)):
        assert call(*args(**bad)) == -1, bad
        assert (alb == 7.0).all()
    # surface_map: depth_map's refusals, albedo, integrator, ray rule
    vp = R.Viewport.new_from_res(8, 6, 1, 2, 1.0)
    cam = vp.camera()
    d, ai = np.empty((6, 8), F), np.full((6, 8, 3), 7.0, F)
    mcall = R.lib().rtw_ctx_surface_map
    margs = lambda **k: [k.get("h", gpu._h), k.get("cam", C.byref(cam)), k.get("w", 8), k.get("hgt", 6), k.get("rule", R.RAYS_PIXEL), None, 0.0, MINT, MAXT,
                         k.get("accel", R.ACCEL_BVH), k.get("integrator", R.INTEGRATOR_RUST2), k.get("d", d.ctypes.data), None, None,
                         k.get("albedo", ai.ctypes.data), None, None, None]
    assert mcall(*margs()) == 0                                   # a NULL offset is 0 0
    assert same(ai, gpu.surface_map(cam, 8, 6, MINT, MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, (0.0, 0.0))["albedo"])
    ai[:] = 7.0
    for bad in (dict(h=None), dict(cam=None), dict(w=0), dict(hgt=0), dict(w=65536, hgt=65536), dict(rule=2), dict(accel=2), dict(integrator=7),
                dict(d=None), dict(albedo=None)):
        assert mcall(*margs(**bad)) == -1, bad
        assert (ai == 7.0).all()
    assert R.lib().rtw_pixel_rays(None, 8, 6, None, d.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert R.lib().rtw_pixel_rays(C.byref(cam), 0, 6, None, d.ctypes.data_as(C.POINTER(C.c_float))) == -1
    with R.Renderer(0) as other:                                  # before any scene
        with pytest.raises(R.RtwError):
            other.scene_surface(rays, MINT, MAXT)


def test_active_texture_noise_is_refused(gpu):
    perlin = R.PerlinNoise(3)
    tex, entry = R.texture_from_color_noise((0.8, 0.6, 0.4), 0.5, perlin)
    scene = R.Scene([R.Sphere.new_with_texture((0.0, 0.0, -3.0), 1.0, (1.0, 1.0, 1.0), R.SCATTER_M, 0)], textures=[tex], noise={0: entry})
    gpu.set_scene(scene)
    try:
        rays = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.0, -1.0], F), (64, 1))
        t, idx, _ = gpu.scene_hits(rays, MINT, MAXT)              # the plain query answers
        assert (idx == 0).all()
        n = len(rays)
        out = [np.full(n, 7.0, F), np.full(n, 7, np.int32), np.full((n, 3), 7.0, F), np.full((n, 3), 7.0, F), np.full((n, 3), 7.0, F), np.full((n, 3), 7.0, F)]
        rc = R.lib().rtw_ctx_scene_surface(gpu._h, rays.ctypes.data, n, 0.0, MINT, MAXT, R.ACCEL_BVH, R.INTEGRATOR_BG_COLOR,
                                           *(a.ctypes.data for a in out), None)
        assert rc == -1 and all((a == 7).all() for a in out)
    finally:
        gpu.set_scene(geom_scene())
