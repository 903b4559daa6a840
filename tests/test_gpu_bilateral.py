"""Rust2's bilateral post-process on the GPU (rtw_ctx_bilateral_filter): the device's bytes and range term against the host path's, bit for
bit -- the CPU test's cases, the reference's own 800x600 / size 10 setting, Edges, a table too large for LDS, the f32 frame path, frames
in device memory, a Rust2 render filtered on the device -- plus the renders around a filter call and the error paths."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.test_bilateral_cpu import PROXIMITIES, SIZES, image_cases, random_image, smooth_image

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def check_device_equals_host(gpu, img, size, prox, avg=0.0):
    host, sh = R.bilateral_filter(img, size, prox, avg_gradient=avg)
    dev, sd = gpu.bilateral_filter(img, size, prox, avg_gradient=avg)
    assert same_bits(sd.avg_gradient, sh.avg_gradient), (sd.avg_gradient, sh.avg_gradient)
    assert sd.taps == sh.taps and sd.spatial == sh.spatial
    bad = np.argwhere(dev != host)
    assert len(bad) == 0, (img.shape, size, prox, len(bad), bad[:5].tolist())
    return dev, sd


@pytest.mark.parametrize("prox", PROXIMITIES)
@pytest.mark.parametrize("size", SIZES)
def test_device_equals_host_small_cases(gpu, size, prox):
    for _, img in image_cases():
        check_device_equals_host(gpu, img, size, prox)


def test_reference_setting_800x600_square_10(gpu):
    img = smooth_image(600, 800, 31)
    _, st = check_device_equals_host(gpu, img, 10, R.PROXIMITY_SQUARE)
    assert st.avg_gradient > 0 and st.spatial == 20.0


def test_640x360_edges_10(gpu):
    check_device_equals_host(gpu, random_image(360, 640, 32), 10, R.PROXIMITY_EDGES)


@pytest.mark.parametrize("prox", PROXIMITIES)
def test_table_beyond_lds(gpu, prox):
    """size 24: the weight table no longer fits beside the tile in LDS and is read from global memory."""
    check_device_equals_host(gpu, smooth_image(130, 170, 33), 24, prox)
    check_device_equals_host(gpu, random_image(70, 90, 34), R.BILATERAL_MAX_SIZE, prox)


def test_given_avg_gradient_skips_the_pass(gpu):
    img = smooth_image(90, 160, 35)
    for avg in (0.02, 0.5):
        _, st = check_device_equals_host(gpu, img, 5, R.PROXIMITY_SQUARE, avg)
        assert st.avg_gradient == np.float32(avg) and st.gradient_ms == 0.0


def test_known_answers_on_device(gpu):
    assert not gpu.bilateral_filter(np.full((40, 50, 3), 99, np.uint8), 4)[0].any()          # uniform: all zero
    assert not gpu.bilateral_filter(random_image(40, 50, 2), 0)[0].any()                     # size 0: all zero
    img = np.zeros((3, 3, 3), np.uint8)
    img[:, 2] = 255
    assert not gpu.bilateral_filter(img, 1)[0].any()                                           # the x + size column is never taken


def test_f32_frame_equals_quantise_then_u8(gpu):
    rng = np.random.default_rng(40)
    frame = rng.uniform(-0.05, 1.1, (120, 200, 3)).astype(np.float32)
    frame[7, 9] = (np.nan, np.inf, -np.inf)
    for prox in PROXIMITIES:
        a, sa = gpu.bilateral_filter(frame, 6, prox)
        b, sb = R.bilateral_filter(R.quantize_u8_rust2(frame), 6, prox)
        assert np.array_equal(a, b) and same_bits(sa.avg_gradient, sb.avg_gradient)


def test_device_pointers_in_and_out(gpu):
    import torch
    img = smooth_image(200, 300, 41)
    frame = (img.astype(np.float32) + 0.3) / np.float32(255.99)
    host, sh = R.bilateral_filter(img, 7, R.PROXIMITY_EDGES)
    for src, fmt in ((img, R.PIXELS_U8), (frame, R.PIXELS_F32_RUST2)):
        t_in = torch.from_numpy(src).to("cuda:0")
        t_out = torch.zeros((200, 300, 3), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        o, sd = gpu.bilateral_filter(t_in.data_ptr(), 7, R.PROXIMITY_EDGES, shape=(200, 300), in_format=fmt, out=t_out.data_ptr())
        assert o == t_out.data_ptr()
        assert np.array_equal(t_out.cpu().numpy(), host) and same_bits(sd.avg_gradient, sh.avg_gradient), fmt
        # device in, host out; host in, device out
        h_out, _ = gpu.bilateral_filter(t_in.data_ptr(), 7, R.PROXIMITY_EDGES, shape=(200, 300), in_format=fmt)
        assert np.array_equal(h_out, host)
        t_out.zero_()
        torch.cuda.synchronize()
        gpu.bilateral_filter(src, 7, R.PROXIMITY_EDGES, out=t_out.data_ptr())
        assert np.array_equal(t_out.cpu().numpy(), host)


def test_rust2_render_filtered_on_device(gpu):
    """render_rows_async -> bilateral_filter (postprocessing.rs:444-447) without a host round trip: the f32 frame stays on the device."""
    import torch
    from tests.test_oracle_golden import rust2_view
    scene, cam, p = rust2_view(160, 90, 9, 6)
    assert p.integrator == R.INTEGRATOR_RUST2 and p.sampler == R.SAMPLER_CENTRES
    gpu.set_scene(scene)
    frame_host, _ = gpu.render(cam, p)
    t = torch.zeros((90, 160, 3), dtype=torch.float32, device="cuda:0")
    t_out = torch.zeros((90, 160, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.render(cam, p, out=t.data_ptr())
    for size, prox in ((10, R.PROXIMITY_SQUARE), (4, R.PROXIMITY_EDGES)):
        _, sd = gpu.bilateral_filter(t.data_ptr(), size, prox, shape=(90, 160), in_format=R.PIXELS_F32_RUST2, out=t_out.data_ptr())
        ref, sh = R.bilateral_filter(R.quantize_u8_rust2(frame_host), size, prox)
        assert np.array_equal(t_out.cpu().numpy(), ref) and same_bits(sd.avg_gradient, sh.avg_gradient)
        assert ref.any()


def test_renders_unchanged_around_a_filter(gpu):
    from tests.test_oracle_golden import rust2_view
    scene, cam, p = rust2_view(96, 54, 4, 5)
    gpu.set_scene(scene)
    before, sb = gpu.render(cam, p)
    gpu.bilateral_filter(smooth_image(300, 400, 42), 10)
    gpu.bilateral_filter(random_image(100, 100, 43), 24, R.PROXIMITY_EDGES)
    after, sa = gpu.render(cam, p)
    assert np.array_equal(before, after) and sa.segments == sb.segments


def test_back_to_back_sizes_rebuild_the_table(gpu):
    img = smooth_image(150, 220, 44)
    outs = {}
    for size, prox in ((10, R.PROXIMITY_SQUARE), (3, R.PROXIMITY_SQUARE), (24, R.PROXIMITY_EDGES), (1, R.PROXIMITY_SQUARE),
                       (10, R.PROXIMITY_EDGES), (10, R.PROXIMITY_SQUARE)):
        out, _ = check_device_equals_host(gpu, img, size, prox)
        outs.setdefault((size, prox), []).append(out)
    assert np.array_equal(*outs[(10, R.PROXIMITY_SQUARE)])
    assert not np.array_equal(outs[(10, R.PROXIMITY_SQUARE)][0], outs[(3, R.PROXIMITY_SQUARE)][0])
    # and a different frame size on the same context (buffers regrow)
    check_device_equals_host(gpu, random_image(41, 23, 45), 10, R.PROXIMITY_SQUARE)
    check_device_equals_host(gpu, smooth_image(400, 500, 46), 10, R.PROXIMITY_EDGES)


def test_error_paths_device(gpu):
    img = random_image(8, 8, 1)
    out = np.empty_like(img)
    ip, op = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    L = R.lib()
    ok = R.RtwBilateral(2, R.PROXIMITY_SQUARE, R.PIXELS_U8, 0.0)
    assert L.rtw_ctx_bilateral_filter(gpu._h, ip, 8, 8, C.byref(ok), op, None) == 0
    assert L.rtw_ctx_bilateral_filter(None, ip, 8, 8, C.byref(ok), op, None) == -1
    assert L.rtw_ctx_bilateral_filter(gpu._h, None, 8, 8, C.byref(ok), op, None) == -1
    assert L.rtw_ctx_bilateral_filter(gpu._h, ip, 8, 8, None, op, None) == -1
    assert L.rtw_ctx_bilateral_filter(gpu._h, ip, 8, 8, C.byref(ok), None, None) == -1
    assert L.rtw_ctx_bilateral_filter(gpu._h, ip, 2, 8, C.byref(ok), op, None) == -1
    assert L.rtw_ctx_bilateral_filter(gpu._h, ip, 8, 2, C.byref(ok), op, None) == -1
    assert L.rtw_ctx_bilateral_filter(gpu._h, ip, 65536, 3, C.byref(ok), op, None) == -1
    bad = [R.RtwBilateral(2, 2, R.PIXELS_U8, 0.0), R.RtwBilateral(2, R.PROXIMITY_SQUARE, 2, 0.0),
           R.RtwBilateral(R.BILATERAL_MAX_SIZE + 1, R.PROXIMITY_SQUARE, R.PIXELS_U8, 0.0)]
    bad += [R.RtwBilateral(2, R.PROXIMITY_SQUARE, R.PIXELS_U8, v) for v in (-1.0, float("nan"), float("inf"))]
    for prm in bad:
        assert L.rtw_ctx_bilateral_filter(gpu._h, ip, 8, 8, C.byref(prm), op, None) == -1
    with pytest.raises(ValueError):
        gpu.bilateral_filter(12345, 3)                        # a pointer without shape / format
    # the context still works
    check_device_equals_host(gpu, img, 2, R.PROXIMITY_SQUARE)
