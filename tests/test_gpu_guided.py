"""The guided filter on the GPU (rtw_ctx_guided_filter): the device's bytes against the host path's, byte for byte -- the CPU test's cases,
both sides of the kernel's two LDS thresholds, the largest size, every combination of guide terms under every LDS layout, buffers in device
memory, the anchors to rtw_ctx_bilateral_filter, a light-biased render filtered with its own depth map, and the context's life around it."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.guided_common import FORMATS, GUIDE_SETS, PROXIMITIES, SHAPES, SIGMA_DEPTH, SIGMA_NORMAL, SIZES, as_f32_frame, case_image, guides, pick
from tests.test_bilateral_cpu import F, random_image, smooth_image

pytestmark = pytest.mark.gpu

ALL = dict(sigma_depth=SIGMA_DEPTH, sigma_normal=SIGMA_NORMAL, same_object=True)


def big_guides(h, w, seed):
    """Guides for an image of any size: a depth ramp with steps, two normal planes with noise, four objects and -1 misses."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    depth = (2.0 + 3.0 * ((x * 4) // w % 2) + 0.01 * y + rng.normal(0, 0.02, (h, w))).astype(F)
    n = np.where(((x + y) % 64 < 32)[..., None], np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, 0.8])) + rng.normal(0, 0.05, (h, w, 3))
    normal = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    ids = ((x * 2) // w + 2 * ((y * 2) // h)).astype(np.int32)
    ids[rng.random((h, w)) < 0.03] = -1
    return depth, normal, ids


def check_device_equals_host(gpu, img, size, prox=R.PROXIMITY_SQUARE, avg=0.0, **kw):
    host, sh = R.guided_filter(img, size, proximity=prox, avg_gradient=avg, **kw)
    dev, sd = gpu.guided_filter(img, size, proximity=prox, avg_gradient=avg, **kw)
    assert np.float32(sd.avg_gradient).view(np.uint32) == np.float32(sh.avg_gradient).view(np.uint32), (sd.avg_gradient, sh.avg_gradient)
    assert sd.taps == sh.taps and sd.spatial == sh.spatial
    bad = np.argwhere(dev != host)
    assert len(bad) == 0, (img.shape, size, prox, sorted(k for k, v in kw.items() if v is not None), len(bad), bad[:5].tolist())
    return dev, sd


# ---- 1. the CPU test's cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prox", PROXIMITIES, ids=["square", "edges"])
@pytest.mark.parametrize("size", SIZES)
def test_device_equals_host_on_the_cpu_cases(gpu, size, prox):
    for h, w in SHAPES:
        img = case_image(h, w)
        for fmt in FORMATS:
            src = img if fmt == R.PIXELS_U8 else as_f32_frame(img)
            for gset in GUIDE_SETS:
                check_device_equals_host(gpu, src, size, prox, **pick(gset, *guides(h, w)))


# ---- 2. / 3. the LDS thresholds and the largest size -----------------------------------------------------------------------------------
# The kernel keeps the packed-pixel tile ((32 + 2 s) x (16 + 2 s) dwords) in LDS, the guide planes (one tile per component: 5 with all three
# guides) behind it while tile + planes <= GUIDE_LDS_MAX, else the guides are read from global memory; and the weight table (1 KiB per
# distinct dx^2 + dy^2 of the window) as well while everything in LDS stays <= TABLE_LDS_MAX (csrc/rtw_filter.hip: GUIDED_GUIDE_LDS_MAX,
# GUIDED_TABLE_LDS_MAX, guided_layout).
GUIDE_LDS_MAX = 80 * 1024
TABLE_LDS_MAX = 80 * 1024


def layout(size, edges, planes=5):
    """(table in LDS, guides in LDS) of the kernel for a window of `size` with `planes` guide components."""
    tile = (32 + 2 * size) * (16 + 2 * size) * 4
    offs = [(dx, dy) for dx in range(-size, size) for dy in range(-size, size) if not edges or abs(dx) + abs(dy) < size]
    table = 1024 * max(1, len({dx * dx + dy * dy for dx, dy in offs}))
    guide_lds = tile * (1 + planes) <= GUIDE_LDS_MAX
    return table + tile * (1 + (planes if guide_lds else 0)) <= TABLE_LDS_MAX, guide_lds


@pytest.mark.parametrize("size,table_lds,guide_lds", [(8, True, True), (9, False, True), (17, False, True), (18, False, False)])
def test_both_sides_of_the_lds_thresholds(gpu, size, table_lds, guide_lds):
    """Square, all three guides.  Table: in LDS at size 8, in global memory at 9.  Guides: in LDS at size 17, in global memory at 18."""
    assert layout(size, False) == (table_lds, guide_lds)
    h, w = 50, 75                                         # two workgroups each way, ragged
    img = smooth_image(h, w, 60 + size)
    check_device_equals_host(gpu, img, size, **dict(zip(("depth", "normal", "ids"), big_guides(h, w, size))), **ALL)


def test_depth_alone_keeps_table_and_guide_in_lds_longer(gpu):
    """One plane instead of five moves the guides' threshold: at size 18 a depth-only Edges call keeps its plane in LDS, the full call nothing."""
    assert layout(18, True, planes=1) == (False, True) and layout(18, False) == (False, False)
    h, w = 50, 75
    depth, _, _ = big_guides(h, w, 3)
    check_device_equals_host(gpu, smooth_image(h, w, 61), 18, R.PROXIMITY_EDGES, depth=depth, sigma_depth=SIGMA_DEPTH)


@pytest.mark.parametrize("prox", PROXIMITIES, ids=["square", "edges"])
def test_size_64_on_40x24(gpu, prox):
    h, w = 24, 40
    assert layout(R.BILATERAL_MAX_SIZE, prox == R.PROXIMITY_EDGES) == (False, False)
    check_device_equals_host(gpu, random_image(h, w, 62), R.BILATERAL_MAX_SIZE, prox,
                             **dict(zip(("depth", "normal", "ids"), big_guides(h, w, 4))), **ALL)


# ---- 4. every template instance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [0, 1, 2, 3, 4], ids=["by-size", "table+guides", "guides", "table", "neither"])
def test_every_combination_of_terms_under_every_layout(gpu, lay):
    """The kernel is a template on (table in LDS, guides in LDS, depth, normal, ids): RTW_OPT_GUIDED_LAYOUT asks for each placement, the
    eight combinations of terms select the rest.  The layout never changes a byte."""
    h, w = 37, 70
    img = case_image(h, w)
    depth, normal, ids = guides(h, w)
    gpu.set_option(R.OPT_GUIDED_LAYOUT, lay)
    try:
        for d in (False, True):
            for n in (False, True):
                for i in (False, True):
                    check_device_equals_host(gpu, img, 4, depth=depth if d else None, normal=normal if n else None, ids=ids if i else None,
                                             sigma_depth=SIGMA_DEPTH if d else 0.0, sigma_normal=SIGMA_NORMAL if n else 0.0, same_object=i)
    finally:
        gpu.set_option(R.OPT_GUIDED_LAYOUT, 0)
    with pytest.raises(R.RtwError):
        gpu.set_option(R.OPT_GUIDED_LAYOUT, 5)


# ---- 5. device pointers ----------------------------------------------------------------------------------------------------------------
def test_device_pointers_for_image_guides_and_out(gpu):
    import torch
    h, w = 90, 130
    img = smooth_image(h, w, 63)
    depth, normal, ids = big_guides(h, w, 5)
    host, _ = R.guided_filter(img, 6, depth=depth, normal=normal, ids=ids, proximity=R.PROXIMITY_EDGES, **ALL)
    t = {k: torch.from_numpy(a).to("cuda:0") for k, a in (("img", img), ("depth", depth), ("normal", normal), ("ids", ids))}
    t_out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    # each buffer on the device alone, then all of them
    for on_dev in (["img"], ["depth"], ["normal"], ["ids"], ["out"], ["img", "depth", "normal", "ids", "out"]):
        src = t["img"].data_ptr() if "img" in on_dev else img
        kw = dict(depth=t["depth"].data_ptr() if "depth" in on_dev else depth, normal=t["normal"].data_ptr() if "normal" in on_dev else normal,
                  ids=t["ids"].data_ptr() if "ids" in on_dev else ids)
        if "img" in on_dev:
            kw.update(shape=(h, w), in_format=R.PIXELS_U8)
        if "out" in on_dev:
            t_out.zero_()
            torch.cuda.synchronize()
            o, _ = gpu.guided_filter(src, 6, proximity=R.PROXIMITY_EDGES, out=t_out.data_ptr(), **kw, **ALL)
            assert o == t_out.data_ptr()
            got = t_out.cpu().numpy()
        else:
            got, _ = gpu.guided_filter(src, 6, proximity=R.PROXIMITY_EDGES, **kw, **ALL)
        assert np.array_equal(got, host), on_dev
    # an f32 frame on the device
    frame = torch.from_numpy(as_f32_frame(img)).to("cuda:0")
    torch.cuda.synchronize()
    got, _ = gpu.guided_filter(frame.data_ptr(), 6, proximity=R.PROXIMITY_EDGES, shape=(h, w), in_format=R.PIXELS_F32_RUST2,
                               depth=t["depth"].data_ptr(), normal=t["normal"].data_ptr(), ids=t["ids"].data_ptr(), **ALL)
    assert np.array_equal(got, host)


# ---- 6. anchors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prox", PROXIMITIES, ids=["square", "edges"])
def test_terms_off_equals_the_bilateral_filter_on_the_device(gpu, prox):
    for (h, w), size in (((37, 70), 3), ((50, 75), 10), ((60, 90), 24)):
        img = smooth_image(h, w, 64)
        plain, sp = gpu.bilateral_filter(img, size, prox)
        depth, normal, ids = big_guides(h, w, 6)
        for kw in (dict(), dict(depth=depth, normal=normal, ids=ids)):
            out, st = gpu.guided_filter(img, size, proximity=prox, **kw)
            assert np.array_equal(out, plain) and st.taps == sp.taps and st.avg_gradient == sp.avg_gradient
        const = dict(depth=np.full((h, w), 3.25, F), normal=np.tile(np.array([0.6, 0.0, 0.8], F), (h, w, 1)), ids=np.full((h, w), 5, np.int32))
        assert np.array_equal(gpu.guided_filter(img, size, proximity=prox, **const, **ALL)[0], plain)


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
def test_light_biased_render_filtered_with_its_depth_map(gpu):
    from tests import lights_common as LC
    ls, g = LC.golden()
    w, h = 80, 60
    cam = LC.camera(g, w, h)
    p = ls.params(w, h, R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"], seed=1, sampler=R.SAMPLER_CENTRES, samples=4, gamma=g["gamma"],
                  mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    frame, _ = gpu.render(cam, p)
    depth, ids, normals, _ = gpu.depth_map(cam, w, h, g["mint"], g["maxt"], ids=True, normals=True)
    assert len(np.unique(ids)) > 2 and np.isfinite(depth).all()
    dev, sd = gpu.guided_filter(frame, 10, depth=depth, normal=normals, ids=ids, sigma_depth=0.2, sigma_normal=0.3, same_object=True)
    host, sh = R.guided_filter(frame, 10, depth=depth, normal=normals, ids=ids, sigma_depth=0.2, sigma_normal=0.3, same_object=True)
    assert np.array_equal(dev, host) and np.float32(sd.avg_gradient).view(np.uint32) == np.float32(sh.avg_gradient).view(np.uint32)
    assert dev.any() and not np.array_equal(dev, gpu.bilateral_filter(frame, 10)[0])
    after, _ = gpu.render(cam, p)
    assert np.array_equal(after, frame)                                        # the scene is left alone


# ---- 8. the context's life -------------------------------------------------------------------------------------------------------------
def test_context_renders_filters_and_is_destroyed_after_guided_calls():
    from tests.test_oracle_golden import rust2_view
    scene, cam, p = rust2_view(96, 54, 4, 5)
    img = smooth_image(54, 96, 65)
    depth, normal, ids = big_guides(54, 96, 7)
    outs = []
    for _ in range(2):                                     # a second context after the first is destroyed
        with R.Renderer(0) as r:
            r.set_scene(scene)
            before, sb = r.render(cam, p)
            a, _ = r.guided_filter(img, 10, depth=depth, normal=normal, ids=ids, **ALL)
            big = smooth_image(120, 200, 66)                # the scratch regrows
            r.guided_filter(big, 20, **dict(zip(("depth", "normal", "ids"), big_guides(120, 200, 8))), **ALL)
            plain, _ = r.bilateral_filter(img, 10)
            b, _ = r.guided_filter(img, 10, depth=depth, normal=normal, ids=ids, **ALL)
            after, sa = r.render(cam, p)
            assert np.array_equal(before, after) and sa.segments == sb.segments
            assert np.array_equal(a, b) and np.array_equal(plain, R.bilateral_filter(img, 10)[0])
            outs.append(a)
    assert np.array_equal(*outs) and np.array_equal(outs[0], R.guided_filter(img, 10, depth=depth, normal=normal, ids=ids, **ALL)[0])


def test_error_paths_device(gpu):
    img = random_image(8, 8, 1)
    out = np.empty_like(img)
    depth, normal, ids = np.ones((8, 8), F), np.ones((8, 8, 3), F), np.ones((8, 8), np.int32)
    ip, op = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    dp, np_, xp = (C.c_void_p(a.ctypes.data) for a in (depth, normal, ids))
    call = R.lib().rtw_ctx_guided_filter

    def prm(sd=0.0, sn=0.0, same=0, size=2):
        return C.byref(R.RtwGuidedFilter(R.RtwBilateral(size, R.PROXIMITY_SQUARE, R.PIXELS_U8, 0.0), sd, sn, same))

    assert call(gpu._h, ip, 8, 8, dp, np_, xp, prm(1.0, 1.0, 1), op, None) == 0
    assert call(gpu._h, ip, 8, 8, None, None, None, prm(), op, None) == 0
    assert call(None, ip, 8, 8, dp, np_, xp, prm(), op, None) == -1
    assert call(gpu._h, None, 8, 8, dp, np_, xp, prm(), op, None) == -1
    assert call(gpu._h, ip, 8, 8, dp, np_, xp, None, op, None) == -1
    assert call(gpu._h, ip, 8, 8, dp, np_, xp, prm(), None, None) == -1
    assert call(gpu._h, ip, 2, 8, dp, np_, xp, prm(), op, None) == -1
    assert call(gpu._h, ip, 8, 8, dp, np_, xp, prm(size=R.BILATERAL_MAX_SIZE + 1), op, None) == -1
    for v in (-1.0, float("nan"), float("inf"), 1e-30):
        assert call(gpu._h, ip, 8, 8, dp, np_, xp, prm(sd=v), op, None) == -1
        assert call(gpu._h, ip, 8, 8, dp, np_, xp, prm(sn=v), op, None) == -1
    assert call(gpu._h, ip, 8, 8, None, np_, xp, prm(sd=1.0), op, None) == -1
    assert call(gpu._h, ip, 8, 8, dp, None, xp, prm(sn=1.0), op, None) == -1
    assert call(gpu._h, ip, 8, 8, dp, np_, None, prm(same=1), op, None) == -1
    assert call(gpu._h, ip, 8, 8, dp, np_, xp, prm(same=2), op, None) == -1
    with pytest.raises(ValueError):
        gpu.guided_filter(12345, 3)                           # a pointer without shape / format
    check_device_equals_host(gpu, img, 2, depth=depth, sigma_depth=1.0)     # the context still works
