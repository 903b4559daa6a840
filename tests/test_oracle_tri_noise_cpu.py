"""The oracle's triangles, texture noise and device-UV flag on the host (no GPU): rtw_oracle_triangle_hits / rtw_oracle_perlin_eval against the
numpy restatements and the library's host forms bit for bit, the reference's triangle_test scene as a known answer, rtw_oracle_render_ex
neutral without extras, RTW_ORACLE_FLAG_DEVICE_UV moving exactly the predicted texels, and the oracle standing apart from the product."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests.test_gpu_triangles import params
from tests.test_oracle_golden import small_view
from tests.test_perlin_cpu import point_set, ref_noise, ref_turb
from tests.test_triangles_cpu import adversarial_rays, pods, random_mesh, reference_triangle_test, same, tri_hits_np, tri_new

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


# ---- triangles ----------------------------------------------------------------------------------------------------------------------
def odd_mesh(rng):
    """A random mesh with a degenerate triangle (u x v == 0: NaN derived fields), one beyond 2^40 and one with a NaN vertex among them."""
    O_, U, V = random_mesh(rng, 60)
    V[5] = U[5] * f32(2)
    O_[17] = f32(1e30)
    O_[29, 1] = np.nan
    return O_, U, V


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("odd", [False, True])
def test_oracle_triangle_hits_match_numpy_and_host(seed, odd):
    rng = np.random.default_rng(100 + seed)
    O_, U, V = odd_mesh(rng) if odd else random_mesh(rng, 60)
    rays = np.concatenate([np.concatenate([rng.uniform(-8, 8, (3000, 3)), rng.normal(size=(3000, 3))], 1).astype(f32),
                           adversarial_rays(rng, O_, U, V, 3000)])
    for mint, maxt in ((1e-3, 1e4), (0.5, 3.0), (-1e3, 1e3), (np.nan, 1e4), (1e-3, np.inf)):
        t_np, i_np = tri_hits_np(O_, U, V, rays, mint, maxt)
        t_h, i_h = R.triangle_hits(pods(O_, U, V), rays, mint, maxt)
        t_o, i_o = O.triangle_hits(pods(O_, U, V), rays, mint, maxt)
        assert np.array_equal(i_o, i_np) and np.array_equal(i_o, i_h), (mint, maxt)
        assert same(t_o, t_np) and same(t_o, t_h), (mint, maxt)
    assert (i_o >= 0).sum() > 1000
    if odd:
        assert (i_o == 5).any()                                     # the degenerate triangle's NaN hit wins where it comes first


def test_oracle_derived_fields_match_the_pod():
    rng = np.random.default_rng(4)
    O_, U, V = odd_mesh(rng)
    O_, U, V = np.concatenate([O_, random_mesh(rng, 300, 100.0, 5.0)[0]]), np.concatenate([U, random_mesh(rng, 300, 100.0, 5.0)[1]]), \
        np.concatenate([V, random_mesh(rng, 300, 100.0, 5.0)[2]])
    tris = [R.Triangle.new(O_[i], U[i], V[i]) for i in range(len(O_))]
    got = O.triangle_derived(tris)
    want = np.array([list(t.pod.normal) + [t.pod.d] + list(t.pod.w) for t in tris], f32)
    assert bits_equal(got, want) or np.array_equal(got, want, equal_nan=True)
    N, D, W = tri_new(O_, U, V)
    assert same(got, np.concatenate([N, D[:, None], W], 1))
    # the oracle reads origin / u / v only: a pod whose derived fields are wrong (TriangleArray leaves them 0) hits the same
    arr = pods(O_, U, V)
    assert bits_equal(O.triangle_derived(arr)[~np.isnan(got).any(axis=1)], got[~np.isnan(got).any(axis=1)])


# ---- Perlin noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 77, 2024])
def test_oracle_perlin_matches_numpy_and_host(seed):
    perlin = R.PerlinNoise(seed)
    pts = point_set(seed=seed + 1)
    cells = np.array([[2.0 ** 31, 0.5, -0.5], [-(2.0 ** 31), 2.0 ** 63, 1.25], [2.0 ** 63, -(2.0 ** 63), 3.0], [np.inf, np.nan, -np.inf],
                      [-(2.0 ** 31) - 256.0, 2.0 ** 31 + 128.0, 7.0]], f32)
    pts = np.concatenate([pts, cells])
    ranvec, perm = perlin.ranvec, perlin.perm
    for depth in range(0, 6):
        oracle = O.perlin_eval(perlin, pts, depth)
        host = perlin.noise(pts) if depth == 0 else perlin.turb(pts, depth)
        want = ref_noise(ranvec, perm, pts) if depth == 0 else ref_turb(ranvec, perm, pts, depth)
        assert bits_equal(oracle, host), depth
        assert bits_equal(oracle, want), depth
    assert np.isnan(O.perlin_eval(perlin, cells[3:4])).all()


# ---- the reference's triangle_test ----------------------------------------------------------------------------------------------------
def test_reference_triangle_test_scene_on_the_oracle():
    scene, cam, p, want, hit = reference_triangle_test()
    img, st = O.render(cam, scene, p, threads=os.cpu_count() or 1)
    for k in range(3):
        assert np.array_equal(img[:, :, k], want)
    n_rays = p.width * p.height * p.samples
    assert st.camera_rays == n_rays and st.quad_tests == st.segments
    assert st.segments == n_rays + int((hit >= 0).sum())                  # a hit scatters once more (depth 2), a miss ends the path


# ---- neutrality -------------------------------------------------------------------------------------------------------------------------
def render_ex(cam, scene, p, x):
    out = np.empty((p.height, p.width, 3), f32)
    st = R.RtwStats()
    rc = O.lib().rtw_oracle_render_ex(C.byref(cam), C.byref(scene.pod), C.byref(x) if x is not None else None, C.byref(p),
                                      out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st), 4)
    assert rc == 0, rc
    return out, st


def same_stats(a, b):
    return (a.camera_rays, a.segments, a.sphere_tests, a.quad_tests, a.nan_pixels, a.rows) == \
        (b.camera_rays, b.segments, b.sphere_tests, b.quad_tests, b.nan_pixels, b.rows)


@pytest.mark.parametrize("which", [R.SCENE_C1, R.SCENE_C5, R.SCENE_QUAD_TEST, R.SCENE_PRESENTATION])
def test_render_ex_without_extras_is_render(which):
    if which in (R.SCENE_QUAD_TEST, R.SCENE_PRESENTATION):
        scene = R.Scene.generate_geom(which)
        cam, p = R.default_view(which)
        p.width, p.height, p.samples = 48, 27, 3
    else:
        scene, cam, p = small_view(which, 48, 27, 3)
    p.gamma = 1.0
    ref, st_ref = O.render(cam, scene, p, threads=4)
    for x in (None, O.Extras()):
        img, st = render_ex(cam, scene, p, x)
        assert bits_equal(img, ref) and same_stats(st, st_ref), which


def test_noise_tables_without_noise_in_use_give_the_plain_image():
    scene, cam, p = small_view(R.SCENE_C5, 48, 27, 3)
    p.gamma = 1.0
    ref, st_ref = O.render(cam, scene, p, threads=4)
    perlin = R.PerlinNoise(9)
    tables = (R.RtwPerlin * 1)(perlin.pod)
    # every texture's entry says "no noise"
    per = (R.RtwTextureNoise * scene.n_textures)(*[R.RtwTextureNoise(-1, 0.5) for _ in range(scene.n_textures)])
    x = O.Extras()
    x.perlin, x.n_perlin = C.cast(tables, C.POINTER(R.RtwPerlin)), 1
    x.tex_noise, x.n_tex_noise = C.cast(per, C.POINTER(R.RtwTextureNoise)), scene.n_textures
    img, st = render_ex(cam, scene, p, x)
    assert bits_equal(img, ref) and same_stats(st, st_ref)
    # a second texture that nothing uses carries the noise (through the Scene and the binding)
    t = list(scene._textures)[0]
    ground = np.array(scene._texels[t.texel_offset:t.texel_offset + t.row * t.col], f32).reshape(t.col, t.row, 3)
    spheres = list(scene._spheres)[:scene.n_spheres]
    unused = R.Scene(spheres, textures=[ground, np.full((2, 2, 3), 0.5, f32)], noise={1: (perlin, 0.3)})
    img, st = O.render(cam, unused, p, threads=4)
    assert bits_equal(img, ref) and same_stats(st, st_ref)
    # ... and on the ground it changes the image, not the path
    used = R.Scene(spheres, textures=[ground], noise={0: (perlin, 0.3)})
    img, st = O.render(cam, used, p, threads=4)
    assert not bits_equal(img, ref) and same_stats(st, st_ref)


def test_render_ex_argument_checks():
    scene, cam, p = small_view(R.SCENE_C5, 16, 9, 1)
    out = np.empty((9, 16, 3), f32)
    L = O.lib()
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    tri = (R.RtwTriangle * 1)(R.Triangle.new((0, 0, -3), (1, 0, 0), (0, 1, 0), tex_index=scene.n_textures).pod)
    x = O.Extras()
    x.triangles, x.n_triangles = C.cast(tri, C.POINTER(R.RtwTriangle)), 1
    assert L.rtw_oracle_render_ex(C.byref(cam), C.byref(scene.pod), C.byref(x), C.byref(p), fp, None, 1) == -1   # texture out of range
    per = (R.RtwTextureNoise * 1)(R.RtwTextureNoise(1, 1.0))
    tables = (R.RtwPerlin * 1)(R.PerlinNoise(1).pod)
    x = O.Extras()
    x.perlin, x.n_perlin = C.cast(tables, C.POINTER(R.RtwPerlin)), 1
    x.tex_noise, x.n_tex_noise = C.cast(per, C.POINTER(R.RtwTextureNoise)), 1
    assert L.rtw_oracle_render_ex(C.byref(cam), C.byref(scene.pod), C.byref(x), C.byref(p), fp, None, 1) == -1   # table index out of range
    per[0].perlin = 0
    assert L.rtw_oracle_render_ex(C.byref(cam), C.byref(scene.pod), C.byref(x), C.byref(p), fp, None, 1) == 0


# ---- RTW_ORACLE_FLAG_DEVICE_UV -------------------------------------------------------------------------------------------------------
def uv_scene():
    """One image-textured sphere filling the view, a texture 1 texel wide and 2^20 tall: v picks among a million rows, so the last-bit
    differences between libm's acosf and the device's sequence move some hits across a row edge.  Nothing else can be hit (a
    Lambert or mirror scatter leaves the convex sphere), so every difference is the first hit's."""
    rng = np.random.default_rng(3)
    tex = rng.uniform(0.05, 0.95, size=(1 << 20, 1, 3)).astype(f32)
    s = R.Sphere.new_with_texture((0.0, 0.0, -2.0), 1.2, None, R.SCATTER_M, 0)
    for k in range(3):
        s.pod.col_mod[k] = 1.0
    return R.Scene([s], textures=[tex], background=(0.7, 0.8, 1.0)), tex


@pytest.mark.parametrize("integrator", [R.INTEGRATOR_GRADIENT, R.INTEGRATOR_RUST2])
def test_device_uv_flag_moves_only_the_predicted_texels(integrator):
    scene, tex = uv_scene()
    W, H = 64, 48
    vp = R.Viewport.new_from_res(W, H, 1, 2, 1.0, vfov=70.0, origin=(0.0, 0.0, 0.0))
    cam = vp.camera()
    p = vp.params(integrator, R.SAMPLER_NO_RAND, R.ACCEL_BRUTE)
    plain, st_plain = O.render(cam, scene, p, threads=4)
    dev, st_dev = O.render(cam, scene, p, threads=4, device_uv=True)
    assert same_stats(st_dev, st_plain)
    # the first hit of every pixel (the camera ray of SAMPLER_NO_RAND, viewport.rs:498-503) and its texel under both UV sequences
    o = np.array(cam.origin, f32)
    p00, du, dv = (np.array(x, f32) for x in (cam.pixel00, cam.delta_u, cam.delta_v))
    normals, pix = [], []
    for j in range(H):
        for i in range(W):
            d = (p00 + du * f32(i)) + dv * f32(j)
            rec, _ = O.trace_ray(o, d, 0.0, scene, p, pixel=j * W + i)
            if rec and rec[0].hit and rec[0].sphere == 0:
                normals.append(list(rec[0].normal)); pix.append((j, i))
    nrm = np.ascontiguousarray(normals, f32)
    uv = {}
    for plain_seq in (0, 1):
        out = np.empty((len(nrm), 4), f32)
        O.lib().rtw_oracle_sphere_uv(nrm.ctypes.data_as(C.POINTER(C.c_float)), len(nrm), plain_seq, out.ctypes.data_as(C.POINTER(C.c_float)))
        uv[plain_seq] = out
    rows, cols = tex.shape[0], tex.shape[1]
    if integrator == R.INTEGRATOR_RUST2:
        idx = {k: np.array([O.lib().rtw_oracle_rust2_texel_index(float(u), float(v), cols, rows, 0) for u, v in uv[k][:, 2:4]]) for k in uv}
    else:                                                     # Rust/ rule: (floor(u * (row - 1)), floor(v * (col - 1))), one column here
        idx = {k: np.floor(uv[k][:, 3] * f32(rows - 1)).astype(np.int64) for k in uv}
    moved = np.zeros((H, W), bool)
    for (j, i), a, b in zip(pix, idx[0], idx[1]):
        moved[j, i] = a != b
    differ = (plain.view(np.uint32) != dev.view(np.uint32)).any(axis=2)
    assert len(pix) > 0.5 * W * H
    assert moved.sum() >= 3, int(moved.sum())
    assert np.array_equal(differ, moved), (int(differ.sum()), int(moved.sum()))


def test_the_tie_and_the_walls_are_in_view():
    from tests.test_gpu_oracle_tri_noise import tri_scene
    """The triangle scene of tests/test_gpu_oracle_tri_noise.py exercises what it claims: the tie triangle, nudged one ulp towards the camera so that it wins, changes the image,
    and so do the textured wall's texels and the emissive triangle's emission."""
    scene, cam = tri_scene(False)
    p = params(R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, 0, spp=4)
    ref, _ = O.render(cam, scene, p, 4)
    tri = scene.triangles
    for k, edit in ((2, "nudge"), (0, "texture"), (1, "emission")):
        saved = R.RtwTriangle.from_buffer_copy(tri[k])
        if edit == "nudge":
            tri[k].origin[2] = float(np.nextafter(f32(tri[k].origin[2]), f32(np.inf)))   # (the plane z = 3 faces the camera at z = 8)
        elif edit == "texture":
            tri[k].tex = -1
        else:
            tri[k].emitted[0] = 0.0
        img, _ = O.render(cam, scene, p, 4)
        tri[k] = saved
        assert not np.array_equal(img, ref), edit


# ---- the oracle stands apart -------------------------------------------------------------------------------------------------------
def test_oracle_includes_nothing_of_the_product():
    src = open(os.path.join(ROOT, "oracle", "rtw_oracle.c")).read()
    includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', src, re.M)
    assert "rtw_oracle.h" in includes
    for inc in includes:
        assert "csrc" not in inc and not inc.startswith("rtw_") or inc == "rtw_oracle.h", inc
        assert os.path.basename(inc) not in os.listdir(os.path.join(ROOT, "raytracing-in-a-weekend_amd", "csrc")), inc
    hdr = open(os.path.join(ROOT, "include", "rtw_oracle.h")).read()
    assert re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', hdr, re.M) == ["rtw.h"]
