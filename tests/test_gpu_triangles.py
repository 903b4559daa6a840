"""Rust2 triangles on the MI355X: device queries == host == numpy, tree == list (queries and renders, every integrator and sampler, the
fallback scenes), the reference's triangle_test scene as a known answer, RNG-free images against numpy, contexts and error paths."""
import numpy as np
import pytest

import rtw_amd as R
from tests.test_triangles_cpu import adversarial_rays, pods, random_mesh, reference_triangle_test, same, tri_hits_np, tri_new

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    if R.device_count() == 0:
        pytest.fail("no GPU")
    with R.Renderer(0) as r:
        yield r


def tri_scene_only(triangles, background=(0.0, 0.0, 0.0), spheres=()):
    return R.Scene(list(spheres), background=background, triangles=triangles)


# ---- queries ---------------------------------------------------------------------------------------------------------------------
def test_device_list_walk_equals_host_and_numpy(gpu):
    rng = np.random.default_rng(11)
    O, U, V = random_mesh(rng, 80)
    rays = np.concatenate([np.concatenate([rng.uniform(-8, 8, (20000, 3)), rng.normal(size=(20000, 3))], 1).astype(f32),
                           adversarial_rays(rng, O, U, V, 20000)])
    gpu.set_scene(tri_scene_only(pods(O, U, V)))
    t_np, i_np = tri_hits_np(O, U, V, rays, 1e-3, 1e4)
    t_h, i_h = R.triangle_hits(pods(O, U, V), rays, 1e-3, 1e4)
    t_d, i_d, st = gpu.triangle_hits(rays, 1e-3, 1e4, R.ACCEL_BRUTE)
    assert np.array_equal(i_d, i_h) and np.array_equal(i_h, i_np)
    assert same(t_d, t_h) and same(t_h, t_np)
    assert st.quad_tests == len(rays) * 80 and st.node_tests == 0


def test_device_tree_equals_list_on_200k_mesh(gpu):
    vtx, faces = R.mesh_terrain(317, seed=2)
    mesh = R.Triangle.from_mesh(vtx, faces)
    assert len(mesh) > 200000
    rng = np.random.default_rng(12)
    n = 1 << 20
    src = rng.uniform(-12, 12, (n, 3)).astype(f32)
    src[:, 1] = rng.uniform(-3, 8, n)
    tgt = vtx[rng.integers(0, len(vtx), n)]                                    # aimed at vertices: shared edges and corners
    tgt[: n // 2] += rng.normal(scale=0.05, size=(n // 2, 3)).astype(f32)
    rays = np.concatenate([src, tgt - src], 1).astype(f32)
    O = vtx[faces[:, 0]]
    adv = adversarial_rays(rng, O, vtx[faces[:, 1]] - O, vtx[faces[:, 2]] - O, 1 << 17)
    rays = np.concatenate([rays, adv])
    gpu.set_scene(tri_scene_only(mesh))
    for mint, maxt in ((1e-3, 1e4), (0.5, 3.0), (-1e3, 1e3)):
        t_l, i_l, st_l = gpu.triangle_hits(rays, mint, maxt, R.ACCEL_BRUTE)
        t_b, i_b, st_b = gpu.triangle_hits(rays, mint, maxt, R.ACCEL_BVH)
        assert np.array_equal(i_b, i_l), (mint, maxt, int((i_b != i_l).sum()))
        assert same(t_b, t_l)
        assert st_b.node_tests > 0 and st_b.quad_tests * 50 < st_l.quad_tests       # the tree prunes
        assert (i_l >= 0).sum() > n // 4


# ---- renders: tree == list -------------------------------------------------------------------------------------------------------
def mixed_scene(extra=(), mesh_level=2, background=(0.7, 0.8, 1.0)):
    rng = np.random.default_rng(5)
    spheres = [R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5))]
    for k in range(60):
        c = (float(rng.uniform(-6, 6)), 0.2, float(rng.uniform(-6, 6)))
        mat = [R.SCATTER_M, R.METALLIC_M, R.GLASS_M, R.FUZZY3_M][k % 4]
        spheres.append(R.Sphere.new(c, 0.2, tuple(float(x) for x in rng.uniform(0.2, 0.9, 3)), mat))
    quads = [R.Quad.new((-2, 0.01, -2), (1.5, 0, 0), (0, 0, 1.5), R.SCATTER_M, (0.8, 0.3, 0.3)),
             R.Quad.new((-1, 3, -1), (2, 0, 0), (0, 0, 2), R.SCATTER_M, (1, 1, 1), emitted=(4, 4, 4))]
    box = R.Instance.new_box((0, 0, 0), (1, 1, 1), (0.9, 0.9, 0.9), R.SCATTER_M)
    box.rotate((0.0, 0.4, 0.1)); box.translate((2.0, 0.0, 1.0))
    smoke = R.Instance.new_box((0, 0, 0), (1.2, 1.2, 1.2), (0.2, 0.2, 0.2), R.SCATTER_M)
    smoke.translate((-3.0, 0.0, 2.0)); smoke.const_density(0.8)
    vtx, faces = R.mesh_icosphere(mesh_level, (0.0, 1.0, 0.0), 1.0)
    tris = list(R.Triangle.from_mesh(vtx, faces, mat=R.SCATTER_M, color=(0.3, 0.7, 0.4)))
    tris[3] = R.Triangle.new(tris[3].pod.origin, tris[3].pod.u, tris[3].pod.v, R.METALLIC_M, (0.9, 0.9, 0.9))
    tris[5] = R.Triangle.new(tris[5].pod.origin, tris[5].pod.u, tris[5].pod.v, R.GLASS_M, (1, 1, 1))
    tris[7] = R.Triangle.new(tris[7].pod.origin, tris[7].pod.u, tris[7].pod.v, R.SCATTER_M, (1, 1, 1), tex_index=0)
    vt, ft = R.mesh_terrain(24, 10.0, 0.4, 3, (0.0, 0.02, 0.0))
    tris += list(R.Triangle.from_mesh(vt, ft, mat=R.SCATTER_M, color=(0.6, 0.5, 0.3)))
    tris = list(extra) + tris
    tex = np.random.default_rng(1).random((3, 4, 3)).astype(f32)
    emit = np.random.default_rng(2).random((2, 2, 3)).astype(f32)
    return R.Scene(spheres, textures=[tex, emit], background=background, quads=quads, instances=[box, smoke],
                   emission_images={0: 1}, triangles=tris)


def view(w=64, h=48):
    vp = R.Viewport.new_from_res(w, h, 1, 4, 1.0, vfov=40.0, origin=(6.0, 3.0, 8.0), direction=(-6.0, -2.2, -8.0), vup=(0.0, 1.0, 0.0))
    return vp.camera()


CONFIGS = [(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, 0), (R.INTEGRATOR_GRADIENT, R.SAMPLER_STRATIFIED, 0),
           (R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, 0), (R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 0),
           (R.INTEGRATOR_NORMAL, R.SAMPLER_NO_RAND, 0), (R.INTEGRATOR_FLAG, R.SAMPLER_ROW, 0),
           (R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, R.FLAG_CPP), (R.INTEGRATOR_RUST2, R.SAMPLER_ROW, R.FLAG_CHUNK_SUMS)]


def params(integ, samp, flags, w=64, h=48, spp=9, depth=6):
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = w, h, spp, depth, 1.0
    p.mint, p.maxt = 0.001, 1e4
    p.integrator, p.sampler, p.flags, p.seed = integ, samp, flags, 77
    return p


def tree_vs_list(r, cam, p, expect_tree=True):
    p.accel = R.ACCEL_BRUTE
    a, sa = r.render(cam, p)
    p.accel = R.ACCEL_BVH
    b, sb = r.render(cam, p)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"max |diff| {np.nanmax(np.abs(a - b))}"
    assert sa.segments == sb.segments
    if expect_tree:
        assert sb.quad_tests < sa.quad_tests
    return a, sa, sb


@pytest.mark.parametrize("integ,samp,flags", CONFIGS)
def test_render_tree_equals_list(gpu, integ, samp, flags):
    gpu.set_scene(mixed_scene())
    a, sa, sb = tree_vs_list(gpu, view(), params(integ, samp, flags))
    assert sa.segments > 0 and np.isfinite(a).mean() > 0.99


@pytest.mark.parametrize("what", ["degenerate_first", "far", "nan_vertex"])
def test_render_fallback_scenes_tree_equals_list(gpu, what):
    if what == "degenerate_first":
        extra = [R.Triangle.new((0.5, 0.5, 0.5), (1, 1, 1), (2, 2, 2), R.SCATTER_M, (1, 0, 0))]
    elif what == "far":
        extra = [R.Triangle.new((1e30, 0, 0), (1, 0, 0), (0, 1, 0), R.SCATTER_M, (1, 0, 0))]
    else:
        extra = [R.Triangle.new((np.nan, 0, 0), (1, 0, 0), (0, 1, 0), R.SCATTER_M, (1, 0, 0))]
    rc, _, _, walk = R.triangle_bvh_validate(mixed_scene(extra).triangles)
    assert rc == 0 and walk == 1                                   # the list walk answers these scenes
    gpu.set_scene(mixed_scene(extra))
    for integ, samp, flags in CONFIGS[:4]:
        tree_vs_list(gpu, view(), params(integ, samp, flags, spp=4), expect_tree=False)


def test_render_wild_rays_and_ranges(gpu):
    gpu.set_scene(mixed_scene())
    for mint, maxt in ((0.001, np.inf), (np.nan, 1e4), (0.001, 3e12)):
        p = params(R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, 0, spp=4)
        p.mint, p.maxt = mint, maxt
        tree_vs_list(gpu, view(), p, expect_tree=False)


# ---- the reference's own scene ---------------------------------------------------------------------------------------------------
def test_reference_triangle_test_scene(gpu):
    scene, cam, p, want, hit = reference_triangle_test()             # (the numpy known answer, shared with the oracle's test)
    gpu.set_scene(scene)
    for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
        p.accel = accel
        img, st = gpu.render(cam, p)
        assert np.array_equal(img[:, :, 0], want) and np.array_equal(img[:, :, 1], want) and np.array_equal(img[:, :, 2], want)
    assert 0.05 < (hit >= 0).mean() < 0.5


# ---- RNG-free images against numpy ------------------------------------------------------------------------------------------------
def test_normal_and_flag_images_against_numpy(gpu):
    vtx, faces = R.mesh_icosphere(2, (0.0, 0.0, -3.0), 1.0)
    mesh = R.Triangle.from_mesh(vtx, faces, mat=R.SCATTER_M, color=(0.4, 0.6, 0.8))
    O = vtx[faces[:, 0]]; U = vtx[faces[:, 1]] - O; V = vtx[faces[:, 2]] - O
    W, H = 48, 40
    vp = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=60.0, origin=(0.2, 0.1, 0.0), direction=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0))
    cam = vp.camera()
    gpu.set_scene(R.Scene([], triangles=mesh))
    i = np.arange(W, dtype=f32)[None, :]
    j = np.arange(H, dtype=f32)[:, None]
    p00, du, dv = (np.array(x, f32) for x in (cam.pixel00, cam.delta_u, cam.delta_v))
    d = (p00 + du * i[..., None]) + dv * j[..., None]
    o = np.broadcast_to(np.array(cam.origin, f32), d.shape)
    rays = np.concatenate([o, d], -1).reshape(-1, 6)
    _, hit = tri_hits_np(O, U, V, rays, 0.001, 1e4)
    N, _, _ = tri_new(O, U, V)
    ud = d.reshape(-1, 3) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).reshape(-1, 1)
    # NORMAL (C++/src/tests.cpp:76-97): 0.5 * (normal + 1) on a hit, the sky gradient otherwise -- through the library's own shading, so
    # compare the pixels the numpy coverage says are hits against the normal rule and the misses against the image of an empty scene
    p = params(R.INTEGRATOR_NORMAL, R.SAMPLER_NO_RAND, 0, W, H, 1, 1)
    for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
        p.accel = accel
        img, _ = gpu.render(cam, p)
        h = hit.reshape(H, W)
        nrm = N[np.maximum(h, 0)]
        want = (nrm + f32(1.0)) * f32(0.5)                          # (normal + 1) * 0.5 (tests.cpp:91)
        assert (h >= 0).sum() > 100
        assert np.array_equal(img[h >= 0], want[h >= 0])
    empty = R.Scene([R.Sphere.new((0, -1e6, 0), 1.0)])
    with R.Renderer(0) as r2:
        r2.set_scene(empty)
        sky, _ = r2.render(cam, p)
    assert np.array_equal(img[hit.reshape(H, W) < 0], sky[hit.reshape(H, W) < 0])
    # FLAG: blue on a miss, and a lambertian hit ends the path with yellow (Rust/src/viewport/glass_tests.rs:8-54)
    p = params(R.INTEGRATOR_FLAG, R.SAMPLER_NO_RAND, 0, W, H, 1, 4)
    img_b, _ = gpu.render(cam, p)
    p.accel = R.ACCEL_BVH
    img_t, _ = gpu.render(cam, p)
    assert np.array_equal(img_b, img_t)
    assert np.array_equal(img_b[hit.reshape(H, W) < 0], np.broadcast_to(np.array([0, 0, 1], f32), img_b[hit.reshape(H, W) < 0].shape))
    hits = img_b[hit.reshape(H, W) >= 0]
    assert np.array_equal(hits, np.broadcast_to(np.array([1, 1, 0], f32), hits.shape))


# ---- contexts --------------------------------------------------------------------------------------------------------------------
def test_multi_context_equals_single(gpu):
    scene = mixed_scene()
    cam = view(72, 56)
    p = params(R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, 0, 72, 56, 4)
    p.accel = R.ACCEL_BVH
    gpu.set_scene(scene)
    one, _ = gpu.render(cam, p)
    for n in (1, 3, 5):
        with R.MultiRenderer([0] * n) as m:
            m.set_scene(scene)
            img, tot, _ = m.render(cam, p)
            assert np.array_equal(img.view(np.uint32), one.view(np.uint32)), n


def test_set_scene_clears_triangles_and_clearing_is_neutral(gpu):
    base = R.Scene.generate(R.SCENE_C1)
    cam, p = R.default_view(R.SCENE_C1)
    p.width, p.height, p.samples = 64, 36, 4
    gpu.set_scene(base)
    before, st0 = gpu.render(cam, p)
    vtx, faces = R.mesh_icosphere(2, tuple(cam.origin), 50.0)             # a dome around the camera: it replaces the sky
    mesh = R.Triangle.from_mesh(vtx, faces, mat=R.SCATTER_M, color=(0.3, 0.7, 0.4))
    gpu.set_triangles(mesh)
    with_tris, st1 = gpu.render(cam, p)
    assert st1.quad_tests > 0 and not np.array_equal(before, with_tris)
    gpu.set_triangles(None)
    after, st2 = gpu.render(cam, p)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32)) and st2.quad_tests == 0
    gpu.set_triangles(mesh)
    gpu.set_scene(base)                                             # set_scene clears them
    again, st3 = gpu.render(cam, p)
    assert np.array_equal(before.view(np.uint32), again.view(np.uint32)) and st3.quad_tests == 0
    with pytest.raises(R.RtwError) as e:
        gpu.triangle_hits(np.zeros((1, 6), f32), 0.0, 1.0)
    assert e.value.status == -6


def test_noise_with_triangles_is_unsupported(gpu):
    tex = np.ones((2, 2, 3), f32)
    perlin = R.PerlinNoise(3)
    s = R.Scene([R.Sphere.new_with_texture((0, 0, -2), 0.5, (1, 1, 1), R.SCATTER_M, 0)], textures=[tex], noise={0: (perlin, 1.0)},
                triangles=[R.Triangle.new((0, 0, -3), (1, 0, 0), (0, 1, 0))])
    with pytest.raises(R.RtwError) as e:
        gpu.set_scene(s)
    assert e.value.status == -5
    s2 = R.Scene([R.Sphere.new_with_texture((0, 0, -2), 0.5, (1, 1, 1), R.SCATTER_M, 0)], textures=[tex], noise={0: (perlin, 1.0)})
    gpu.set_scene(s2)
    with pytest.raises(R.RtwError) as e:
        gpu.set_triangles([R.Triangle.new((0, 0, -3), (1, 0, 0), (0, 1, 0))])
    assert e.value.status == -5
    gpu.set_scene(R.Scene([R.Sphere.new((0, 0, -2), 0.5)], textures=[tex]))
    with pytest.raises(R.RtwError):
        gpu.set_triangles([R.Triangle.new((0, 0, -3), (1, 0, 0), (0, 1, 0), tex_index=1)])   # a texture the scene does not have
