"""One context, reused: after a big scene, a small one, partitions, options, triangles, lights, noise, a refused scene, queries and filters,
every answer equals, bit for bit, the answer of a context created for that call alone.

The module's context `ctx` is this file's own (not the session renderer): its buffer history is what the tests below give it, in file order.
Each test also stands alone -- run by itself it starts from the first render only."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import lights_common as LC
from tests import oracle_binding as O
from tests.test_gpu_perlin import SCALE, build_ratio_scene
from tests.test_oracle_golden import small_view

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID = -1


def c2_view(w, h, samples):
    scene, cam, p = small_view(R.SCENE_C2, w, h, samples)
    p.gamma, p.accel = 1.0, R.ACCEL_BVH
    return scene, cam, p


def c1_view(accel):
    scene = R.Scene.generate(R.SCENE_C1)
    cam, p = R.default_view(R.SCENE_C1)
    p.width, p.height, p.samples, p.gamma, p.accel = 64, 36, 4, 1.0, accel
    return scene, cam, p


def render(r, view):
    scene, cam, p = view
    r.set_scene(scene)
    return r.render(cam, p)[0]


def fresh(step):
    """step(r) on a context created for it and closed after it."""
    with R.Renderer(0) as r:
        return step(r)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check(ctx, step, what):
    """The step on the context with a history and on a fresh one: every array of the answer equal on the bits."""
    got, want = step(ctx), fresh(step)
    if isinstance(got, np.ndarray):
        got, want = (got,), (want,)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (what, k)
    return got if len(got) > 1 else got[0]


def assemble(parts, height, row_block):
    """The compact rows of each partition at their image rows."""
    full = np.empty((height,) + parts[0].shape[1:], F)
    n_blocks = (height + row_block - 1) // row_block
    for k, img in enumerate(parts):
        r = 0
        for b in range(k, n_blocks, len(parts)):
            rows = min(row_block, height - b * row_block)
            full[b * row_block:b * row_block + rows] = img[r:r + rows]
            r += rows
        assert r == len(img)
    return full


@pytest.fixture(scope="module")
def first():
    """Step 1's view and its image on a fresh context (485 spheres: the tree kernel with f16 nodes in LDS)."""
    view = c2_view(160, 90, 8)
    return view, fresh(lambda r: render(r, view))


@pytest.fixture(scope="module")
def ctx(first):
    """The context with a history; it has rendered step 1 before any test sees it."""
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    view, want = first
    with R.Renderer(0) as r:
        assert same(render(r, view), want)
        yield r


def test_first_render_equals_the_oracle(ctx, first):
    (scene, cam, p), want = first
    ref, st_ref = O.render(cam, scene, p)
    img, st = ctx.render(cam, p)
    assert st.node_tests > 0 and st.segments == st_ref.segments
    assert same(img, ref) and same(want, ref)


def test_scenes_frames_partitions_and_options(ctx, first):
    # 2. a smaller scene and a smaller frame: every retained buffer is larger than needed
    for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
        check(ctx, lambda r: render(r, c1_view(accel)), f"C1 64 x 36, accel {accel}")

    # 3. a bigger frame again, as three partitions of 8-row blocks (120 rows = 15 blocks) ...
    big = c2_view(200, 120, 4)
    whole = fresh(lambda r: render(r, big))

    def partitions(r):
        scene, cam, p = big
        r.set_scene(scene)
        q = R.RtwParams.from_buffer_copy(p)
        q.row_block, q.part_count = 8, 3
        parts = []
        for k in range(3):
            q.part_index = k
            parts.append(r.render(cam, q)[0].copy())
        return assemble(parts, 120, 8)
    assert same(check(ctx, partitions, "three partitions"), whole)
    # ... and two contexts of one GPU into a pageable host frame (pinned staging, scattered on the host), growing and shrinking
    with R.MultiRenderer([0, 0]) as m:
        for view in (c2_view(96, 54, 4), big, c1_view(R.ACCEL_BVH)):
            scene, cam, p = view
            m.set_scene(scene)
            img, tot, _ = m.render(cam, p, out=np.full((p.height, p.width, 3), -1.0, F))
            assert tot.rows == p.height
            assert same(img, fresh(lambda r: render(r, view))), (p.width, p.height)

    # 4. a sample bank too small for the frame (bands of one tile row: 25 tiles x 16 samples x 64 x 12 B = 0.29 MiB of 0.5 MiB), then the
    #    default again: the bank of the whole frame (4.4 MiB) is larger than any this context has had
    banked = c2_view(200, 120, 16)
    want = fresh(lambda r: render(r, banked))
    for gb in (0.0005, 48.0):
        def bank(r):
            r.set_option(R.OPT_SAMPLE_BANK_GB, gb)
            return render(r, banked)
        assert same(check(ctx, bank, f"sample bank of {gb} GB"), want)

    # 5. the cost order of the tiles under one scene: built, regrown for more tiles, rebuilt in place for fewer, reused as it is
    sizes = ((160, 90), (200, 120), (160, 90), (160, 90))

    def ordered(r, mode=2):
        r.set_option(R.OPT_TILE_ORDER, mode)
        r.set_scene(big[0])
        out = []
        for w, h in sizes:
            _, cam, p = c2_view(w, h, 4)
            out.append(r.render(cam, p)[0].copy())
        r.set_option(R.OPT_TILE_ORDER, 0)
        return tuple(out)
    raster = fresh(lambda r: ordered(r, 0))
    for img, want in zip(check(ctx, ordered, "tile order 2"), raster):
        assert same(img, want)
    assert same(render(ctx, first[0]), first[1])


def test_triangles_lights_noise_and_a_refused_scene(ctx, first):
    view, image = first
    scene, cam, p = view

    # 6. triangles on and off: a 20-triangle dome around the camera replaces the sky; without it the image is step 1's
    vtx, faces = R.mesh_icosphere(0, tuple(cam.origin), 50.0)
    dome = R.Triangle.from_mesh(vtx, faces, mat=R.SCATTER_M, color=(0.3, 0.7, 0.4))

    def with_dome(r):
        r.set_scene(scene)
        r.set_triangles(dome)
        return r.render(cam, p)[0]
    assert not same(check(ctx, with_dome, "C2 under a dome of triangles"), image)
    ctx.set_triangles(None)
    assert same(ctx.render(cam, p)[0], image)

    # 7. lights on and off
    ls, g = LC.golden()
    lcam = LC.camera(g, 40, 30)
    lp = ls.params(40, 30, R.INTEGRATOR_LIGHT_BIASED, 9, seed=3, sampler=R.SAMPLER_ROW, samples=4)

    def lit(r):
        r.set_scene(ls.scene)
        r.set_lights(ls.lights, ls.weight)
        return r.render(lcam, lp)[0]

    def unlit(r):
        r.set_scene(ls.scene)
        return r.render(lcam, lp)[0]
    assert not same(check(ctx, lit, "the light scene, light-biased"), fresh(unlit))
    bp = R.RtwParams.from_buffer_copy(p)
    bp.integrator = R.INTEGRATOR_LIGHT_BIASED

    def c2_light_biased(r):                                # (set_scene clears the lights)
        r.set_scene(scene)
        return r.render(cam, bp)[0]
    check(ctx, c2_light_biased, "C2 light-biased after a scene with lights")

    # 8. texture noise on and off: one white-textured sphere
    v = R.Viewport.new_from_res(48, 27, 1, 2, 1.0)
    np_, ncam = v.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_NO_RAND, R.ACCEL_BRUTE), v.camera()
    plain = fresh(lambda r: render(r, (build_ratio_scene("sphere", None), ncam, np_)))
    noised = check(ctx, lambda r: render(r, (build_ratio_scene("sphere", (R.PerlinNoise(2024), SCALE)), ncam, np_)), "noised sphere")
    assert not same(noised, plain)
    ctx.set_texture_noise()
    assert same(ctx.render(ncam, np_)[0], plain)

    # 9. a refused set_scene keeps the old scene
    bad = R.Scene([R.Sphere.new_with_texture((0.0, 0.0, -1.5), 0.5, (1.0, 1.0, 1.0), R.SCATTER_M, 0)])      # texture 0 of none
    with pytest.raises(R.RtwError) as e:
        ctx.set_scene(bad)
    assert e.value.status == E_INVALID
    assert same(ctx.render(ncam, np_)[0], plain)
    assert same(render(ctx, view), image)


def test_queries_and_filters_between_renders(ctx, first):
    import torch
    view, image = first
    scene, cam, p = view
    L = R.lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(21)
    origin = np.array(list(cam.origin), F)
    rays = np.concatenate([np.broadcast_to(origin, (64, 3)), rng.normal(0.0, 4.0, (64, 3)).astype(F) - origin], 1).astype(F)
    dcam = R.camera2_new(32 / 18, tuple(origin), (0.0, 1.0, 0.0), tuple(-origin), 40.0, 0.0)
    MINT, MAXT = 0.001, 1000.0

    # 10. scene_hits over 64 rays and a 32 x 18 depth map with ids and normals: staged through host arrays, and straight into device tensors
    def queries(r):
        r.set_scene(scene)
        t, idx, nrm, _ = r.scene_hits(rays, MINT, MAXT, normals=True)
        depth, ids, normals, _ = r.depth_map(dcam, 32, 18, MINT, MAXT, ids=True, normals=True)
        d_rays = torch.from_numpy(rays).to(dev)
        d_t, d_i, d_n = (torch.full((64,), -7.5, device=dev), torch.full((64,), -77, dtype=torch.int32, device=dev),
                         torch.full((64, 3), -7.5, device=dev))
        d_d, d_ids, d_nrm = (torch.full((18, 32), -7.5, device=dev), torch.full((18, 32), -77, dtype=torch.int32, device=dev),
                             torch.full((18, 32, 3), -7.5, device=dev))
        torch.cuda.synchronize()
        st = R.RtwStats()
        assert L.rtw_ctx_scene_hits(r._h, d_rays.data_ptr(), 64, 0.0, MINT, MAXT, R.ACCEL_BVH, d_t.data_ptr(), d_i.data_ptr(), d_n.data_ptr(),
                                    C.byref(st)) == R.RTW_OK
        assert L.rtw_ctx_depth_map(r._h, C.byref(dcam), 32, 18, 0.0, MINT, MAXT, R.ACCEL_BVH, d_d.data_ptr(), d_ids.data_ptr(), d_nrm.data_ptr(),
                                   C.byref(st)) == R.RTW_OK
        direct = tuple(x.cpu().numpy() for x in (d_t, d_i, d_n, d_d, d_ids, d_nrm))
        staged = (t, idx, nrm, depth, ids, normals)
        for a, b in zip(staged, direct):
            assert same(a, b)
        return staged
    t, idx, *_ = check(ctx, queries, "scene queries")
    assert 0 < int((idx >= 0).sum()) < 64
    assert same(ctx.render(cam, p)[0], image)

    # 11. the filter's scratch growing, shrinking and growing again at another size (u8 host frames: img, terms, table, out)
    frames = [np.random.default_rng(k).integers(0, 256, (h, w, 3), dtype=np.uint8) for k, (w, h) in enumerate(((48, 32), (16, 8), (48, 32)))]
    for frame, size in zip(frames, (3, 2, 5)):
        check(ctx, lambda r: r.bilateral_filter(frame, size)[0], f"bilateral filter of {frame.shape}, size {size}")
    f32 = (frames[0].astype(F) / F(255.0))                       # a host f32 frame: staged, then quantised on the device
    check(ctx, lambda r: r.bilateral_filter(f32, 4, R.PROXIMITY_EDGES)[0], "bilateral filter of an f32 frame")
    assert same(ctx.render(cam, p)[0], image)


def test_destroy_then_create(ctx, first):
    # 12. close the context with the history, create and close a second on the same device, render step 1 on a third
    view, image = first
    ctx.close()
    R.Renderer(0).close()
    assert same(fresh(lambda r: render(r, view)), image)
