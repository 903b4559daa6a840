"""Scene ray queries, the parts that need no GPU: rtw_depth_rays against an f32 numpy restatement of Rust2's Viewport::depth_map ray
(Rust2/src/viewport.rs:77-80, then :63), and the argument checks of the three calls."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R

F = np.float32
E_INVALID = -1


def camera():
    """Off-axis, with a vup that is neither the default nor perpendicular to the view direction."""
    return R.camera2_new(1.7, (1.25, -0.5, 3.0), (0.3, 1.0, -0.2), (-0.4, 0.15, -1.0), 47.0, 0.0)


def restated_rays(cam, width, height):
    """unit(left_top + delta_x * (i as f32 / width as f32) + delta_y * (j as f32 / height as f32)): explicit f32 operations, each product a
    vector times a scalar, the sums left to right, unit(a) = a / sqrt(a . a)."""
    lt = np.array(list(cam.pixel00), F)
    dx = np.array(list(cam.delta_u), F)
    dy = np.array(list(cam.delta_v), F)
    o = np.array(list(cam.origin), F)
    out = np.empty((height * width, 6), F)
    for j in range(height):
        fy = F(F(j) / F(height))
        for i in range(width):
            fx = F(F(i) / F(width))
            a = ((lt + (dx * fx).astype(F)).astype(F) + (dy * fy).astype(F)).astype(F)
            l2 = F(F(F(a[0] * a[0]) + F(a[1] * a[1])) + F(a[2] * a[2]))
            out[j * width + i, :3] = o
            out[j * width + i, 3:] = (a / F(np.sqrt(l2))).astype(F)
    return out


@pytest.mark.parametrize("width,height", [(1, 1), (3, 2), (33, 17), (64, 64)])
def test_depth_rays_equal_the_f32_restatement(width, height):
    cam = camera()
    got = R.depth_rays(cam, width, height)
    assert got.shape == (width * height, 6) and got.dtype == np.float32
    want = restated_rays(cam, width, height)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # directions are unit length and differ from pixel to pixel (the camera is not degenerate)
    assert np.allclose(np.linalg.norm(got[:, 3:].astype(np.float64), axis=1), 1.0, atol=1e-6)
    if width * height > 1:
        assert len(np.unique(got[:, 3:], axis=0)) == width * height


def test_depth_rays_argument_errors():
    L = R.lib()
    cam = camera()
    buf = np.zeros((4, 6), F)
    p = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rtw_depth_rays(C.byref(cam), 0, 2, p) == E_INVALID
    assert L.rtw_depth_rays(C.byref(cam), 2, 0, p) == E_INVALID
    assert L.rtw_depth_rays(None, 2, 2, p) == E_INVALID
    assert L.rtw_depth_rays(C.byref(cam), 2, 2, None) == E_INVALID
    assert not buf.any()
    assert L.rtw_depth_rays(C.byref(cam), 2, 2, p) == R.RTW_OK
    with pytest.raises(R.RtwError):
        R.depth_rays(cam, 0, 3)


def test_null_context_is_invalid_without_a_device():
    L = R.lib()
    cam = camera()
    rays = np.zeros((2, 6), F)
    t = np.zeros(2, F)
    idx = np.zeros(2, np.int32)
    st = R.RtwStats()
    assert L.rtw_ctx_scene_hits(None, rays.ctypes.data, 2, 0.0, 0.001, 100.0, R.ACCEL_BVH, t.ctypes.data, idx.ctypes.data, None,
                                C.byref(st)) == E_INVALID
    assert L.rtw_ctx_depth_map(None, C.byref(cam), 2, 1, 0.0, 0.001, 100.0, R.ACCEL_BVH, t.ctypes.data, None, None, C.byref(st)) == E_INVALID
