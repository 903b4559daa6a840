"""The post-process kernels (csrc/rtw_filter.hip) at their value, size and sum-order edges, on the GPU, exactly: bilateral_quantize_kernel
against a numpy restatement of Rust2's rounding at every tie and special value; bilateral_gradient_sum_kernel against the serial Python sum at
every n % 4 and around its 2048-term chunks; guided_filter_kernel with NaN, infinite, overflowing and denormal-scaled guides through both of
its load paths; both filter kernels on frames around and below their 32 x 16 workgroup.  The cases and references are
filter_edges_common.py's; test_filter_edges_cpu.py proves that they discriminate."""
import numpy as np
import pytest

import rtw_amd as R
from tests import filter_edges_common as E
from tests.guided_common import mismatch
from tests.test_bilateral_cpu import F

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- A. quantisation at its ties and specials ----------------------------------------------------------------------------------------
def test_quantise_kernel_on_a_staged_frame(gpu):
    frame = E.quantize_frame()
    out, st = gpu.bilateral_filter(frame, **E.READ_OUT)
    E.check_read_out(out, E.ref_quantize_rust2(frame))
    assert st.avg_gradient == 1.0 and st.taps == E.QUANT_H * E.QUANT_W


def test_quantise_kernel_on_a_frame_in_device_memory(gpu):
    import torch
    frame = E.quantize_frame()
    h, w = frame.shape[:2]
    t = torch.from_numpy(frame.copy()).to("cuda:0")
    torch.cuda.synchronize()
    out, _ = gpu.bilateral_filter(t.data_ptr(), shape=(h, w), in_format=R.PIXELS_F32_RUST2, **E.READ_OUT)
    E.check_read_out(out, E.ref_quantize_rust2(frame))
    assert np.array_equal(E.bits(t.cpu().numpy()), E.bits(frame))                            # the frame is read, not rewritten


def test_quantise_kernel_through_the_guided_filter(gpu):
    frame = E.quantize_frame()
    out, _ = gpu.guided_filter(frame, **E.READ_OUT)
    E.check_read_out(out, E.ref_quantize_rust2(frame))


# ---- B. the gradient sum at vector, chunk and tail boundaries ------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.TERM_COUNTS)
def test_gradient_sum_on_thin_frames(gpu, n):
    """3 x (n + 2) and (n + 2) x 3: n terms, and filter grids of up to 193 x 1 and 1 x 385 workgroups over a frame three pixels thick."""
    for o in E.ORIENTATIONS:
        img = E.thin_frame(n, o)
        dev, sd = gpu.bilateral_filter(img, 3)
        host, sh = R.bilateral_filter(img, 3)
        assert same_bits(sd.avg_gradient, E.thin_avg(n, o)), (n, o, sd.avg_gradient, E.thin_avg(n, o))
        assert sd.taps == sh.taps and sd.spatial == sh.spatial
        assert mismatch(dev, host) is None, (n, o, mismatch(dev, host))
        if n <= E.REF_BYTES_MAX_N:
            ref, taps = E.thin_bytes(n, o)
            assert sd.taps == taps and mismatch(dev, ref) is None, (n, o, mismatch(dev, ref))
        g, sg = gpu.guided_filter(img, 3)                                                     # the same pass in front of the other kernel
        assert same_bits(sg.avg_gradient, sd.avg_gradient) and np.array_equal(g, dev)


@pytest.mark.parametrize("n,last,value", list(E.single_term_cases()), ids=E.SINGLE_TERM_IDS)
def test_single_term_known_answer(gpu, n, last, value):
    img, want = E.single_term_frame(n, last, value)
    _, st = gpu.bilateral_filter(img, 1)
    assert same_bits(st.avg_gradient, want), (n, last, st.avg_gradient, want)


# ---- C. the guided filter with non-finite and extreme guides, on both load paths ------------------------------------------------------
@pytest.mark.parametrize("h,w", E.GUIDED_SHAPES, ids=[f"{w}x{h}" for h, w in E.GUIDED_SHAPES])
@pytest.mark.parametrize("name", list(E.GUIDED_CASES))
def test_guided_edge_values_under_both_layouts(gpu, name, h, w):
    img = E.guided_image(h, w)
    kw = E.guided_case(name, h, w)
    try:
        for size in E.GUIDED_SIZES:
            for prox in E.PROXIMITIES:
                ref = E.guided_ref(name, h, w, size, prox)
                host, _ = R.guided_filter(img, size, proximity=prox, avg_gradient=E.GUIDED_AVG, **kw)
                for where, lay in E.GUIDED_LAYOUTS.items():
                    gpu.set_option(R.OPT_GUIDED_LAYOUT, lay)
                    dev, st = gpu.guided_filter(img, size, proximity=prox, avg_gradient=E.GUIDED_AVG, **kw)
                    assert st.avg_gradient == F(E.GUIDED_AVG)
                    assert mismatch(dev, host) is None, (where, size, prox, mismatch(dev, host))
                    assert mismatch(dev, ref) is None, (where, size, prox, mismatch(dev, ref))
                    dead = E.dead_centres(kw)
                    if dead is not None:
                        assert not dev[dead].any()
                    assert dev.any() != (name in E.BLACK_CASES)
    finally:
        gpu.set_option(R.OPT_GUIDED_LAYOUT, 0)


def whole_window_in(mask, size):
    """Pixels whose half-open clipped window (x - min(x, s) .. x + min(w - x - 1, s), rows likewise) is non-empty and lies inside `mask`."""
    h, w = mask.shape
    out = np.zeros_like(mask)
    for y in range(h):
        for x in range(w):
            win = mask[y - min(y, size):y + min(h - y - 1, size), x - min(x, size):x + min(w - x - 1, size)]
            out[y, x] = win.size > 0 and win.all()
    return out


def test_scene_hits_planes_guide_the_filter_in_device_memory(gpu):
    """Render -> scene_hits of the depth rays -> guided filter, with t (+inf on the sky), the normals and the indices as they come, in device
    memory: the host form's bytes on the copied-back planes.  A sky pixel's depth is +inf, so with the depth term on every tap of its window
    is dropped (inf - inf) or weighs +0 (dz^2 = inf): sky comes out 0 0 0 -- the documented behaviour of a non-finite depth."""
    import torch
    from tests.test_oracle_golden import rust2_view
    w, h = 48, 27
    scene, cam, p = rust2_view(w, h, 4, 5)
    gpu.set_scene(scene)
    frame, _ = gpu.render(cam, p)
    t, idx, nrm, _ = gpu.scene_hits(R.depth_rays(cam, w, h), p.mint, p.maxt, normals=True)
    sky = np.isinf(t).reshape(h, w)
    assert np.array_equal(sky, idx.reshape(h, w) < 0) and (t[np.isinf(t)] > 0).all() and sky.any() and not sky.all()
    inside = whole_window_in(sky, 3)
    assert inside.any()
    planes = dict(depth=t.reshape(h, w), normal=nrm.reshape(h, w, 3), ids=idx.reshape(h, w))
    dev_t = {k: torch.from_numpy(a).to("cuda:0") for k, a in planes.items()}
    d_frame = torch.from_numpy(frame).to("cuda:0")
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in dev_t.items()}
    try:
        for terms in (dict(sigma_depth=0.5), dict(sigma_depth=0.5, sigma_normal=0.3, same_object=True), dict(sigma_normal=0.3, same_object=True)):
            host, sh = R.guided_filter(frame, 3, **planes, **terms)
            for lay in E.GUIDED_LAYOUTS.values():
                gpu.set_option(R.OPT_GUIDED_LAYOUT, lay)
                dev, sd = gpu.guided_filter(d_frame.data_ptr(), 3, shape=(h, w), in_format=R.PIXELS_F32_RUST2, **ptrs, **terms)
                assert same_bits(sd.avg_gradient, sh.avg_gradient) and mismatch(dev, host) is None, (terms, lay, mismatch(dev, host))
                if "sigma_depth" in terms:
                    assert not dev[sky].any() and not dev[inside].any() and dev[~sky].any()
                else:
                    assert dev[inside].any()                                                  # without the depth term the sky is filtered like anything
    finally:
        gpu.set_option(R.OPT_GUIDED_LAYOUT, 0)
    for k, a in planes.items():                                                               # the planes are read, not rewritten
        assert np.array_equal(dev_t[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32)), k


# ---- D. frame geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", E.GEOMETRY_SHAPES, ids=[f"{w}x{h}" for h, w in E.GEOMETRY_SHAPES])
def test_small_geometries(gpu, h, w):
    img = E.geometry_image(h, w)
    gk = E.geometry_guides(h, w)
    for size in E.GEOMETRY_SIZES:
        for prox in E.PROXIMITIES:
            host, sh = R.bilateral_filter(img, size, prox)
            dev, sd = gpu.bilateral_filter(img, size, prox)
            assert same_bits(sd.avg_gradient, sh.avg_gradient) and sd.taps == sh.taps and sd.spatial == sh.spatial
            assert mismatch(dev, host) is None, ("bilateral", size, prox, mismatch(dev, host))
            host, sh = R.guided_filter(img, size, proximity=prox, **gk)
            dev, sd = gpu.guided_filter(img, size, proximity=prox, **gk)
            assert same_bits(sd.avg_gradient, sh.avg_gradient) and sd.taps == sh.taps
            assert mismatch(dev, host) is None, ("guided", size, prox, mismatch(dev, host))


@pytest.mark.parametrize("avg", E.AVG_EXTREMES)
def test_given_avg_gradient_extremes(gpu, avg):
    img = E.geometry_image(17, 33)
    for prox in E.PROXIMITIES:
        host, sh = R.bilateral_filter(img, 3, prox, avg_gradient=avg)
        dev, sd = gpu.bilateral_filter(img, 3, prox, avg_gradient=avg)
        assert same_bits(sd.avg_gradient, sh.avg_gradient) and same_bits(sd.avg_gradient, F(avg))
        assert mismatch(dev, host) is None, (prox, mismatch(dev, host))
        assert dev.any() == (avg != 1e-30)
        g, _ = gpu.guided_filter(img, 3, proximity=prox, avg_gradient=avg)
        assert np.array_equal(g, dev)
