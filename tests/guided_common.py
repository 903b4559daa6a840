"""Shared by the guided-filter tests (test_guided_cpu.py, test_gpu_guided.py): an independent numpy restatement of the definition in
include/rtw.h (every tap evaluated, `a` formed in float32 in the written order, g from exp_plain), the guide images and the case list."""
import functools

import numpy as np

import rtw_amd as R
from tests.test_bilateral_cpu import F, libm_expf, random_image, ref_avg_gradient, rust_as_u8, smooth_image

SHAPES = [(3, 3), (17, 33), (37, 70)]                  # (h, w): 3x3, 33x17 and 70x37
SIZES = [0, 1, 3, 10]
PROXIMITIES = [R.PROXIMITY_SQUARE, R.PROXIMITY_EDGES]
FORMATS = [R.PIXELS_U8, R.PIXELS_F32_RUST2]
SIGMA_DEPTH, SIGMA_NORMAL = 0.5, 0.3
# which guide terms are on: each alone and all together
GUIDE_SETS = {"depth": (True, False, False), "normal": (False, True, False), "ids": (False, False, True), "all": (True, True, True)}


@functools.lru_cache(maxsize=None)
def case_image(h, w):
    return smooth_image(h, w, 300 + h) if (h + w) % 2 else random_image(h, w, 300 + h)


def as_f32_frame(img):
    """An f32 frame that Rust2's quantisation (quantize_u8_rust2) brings back to `img`."""
    frame = ((img.astype(F) + F(0.3)) / F(255.99)).astype(F)
    assert np.array_equal(R.quantize_u8_rust2(frame), img)
    return frame


@functools.lru_cache(maxsize=None)
def guides(h, w):
    """(depth, normal, ids): a depth step edge (plus a ramp, so that dz takes many values), two normal planes (slightly perturbed unit
    vectors), two objects split along the diagonal with a block and a sprinkle of -1 misses (depth 16, normal 0 0 0, as depth_map writes)."""
    rng = np.random.default_rng(1000 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    depth = (np.where(x < w // 2, 2.0, 5.0) + 0.02 * y + 0.01 * x).astype(F)
    n = np.where((x * h < y * w)[..., None], np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, 0.8])) + rng.normal(0, 0.02, (h, w, 3))
    normal = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    ids = np.where(x * h + y * w < h * w, 3, 7).astype(np.int32)
    miss = (rng.random((h, w)) < 0.05) | ((y < h // 4) & (x >= w - max(1, w // 4)))
    ids[miss] = -1
    depth[miss] = F(16.0)
    normal[miss] = 0.0
    return depth, normal, ids


def pick(gset, depth, normal, ids):
    """The keyword arguments of guided_filter for one of GUIDE_SETS."""
    d, n, i = GUIDE_SETS[gset]
    return dict(depth=depth if d else None, normal=normal if n else None, ids=ids if i else None,
                sigma_depth=SIGMA_DEPTH if d else 0.0, sigma_normal=SIGMA_NORMAL if n else 0.0, same_object=i)


@functools.lru_cache(maxsize=None)
def avg_of(h, w):
    return ref_avg_gradient(case_image(h, w))


def ref_guided(img, size, edges, avg, depth=None, normal=None, ids=None, sigma_depth=0.0, sigma_normal=0.0, same_object=False):
    """The definition, tap by tap (u8 image; avg as ref_avg_gradient gives it, or the given avg_gradient).  Offsets are walked dx outer, dy
    inner, both increasing, and a tap is taken iff it lies in the pixel's half-open window: every pixel's taps in the reference's order."""
    h, w = img.shape[:2]
    spatial = np.ceil(F(F(0.02) * np.sqrt(F(w * w + h * h))))
    avg = F(avg)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_range = F(F(0.5) / F(avg * avg))
        inv_spatial = F(F(0.5) / F(spatial * spatial))
        inv_depth = F(F(0.5) / F(F(sigma_depth) * F(sigma_depth))) if sigma_depth > 0 else None
        inv_normal = F(F(0.5) / F(F(sigma_normal) * F(sigma_normal))) if sigma_normal > 0 else None
    guided = inv_depth is not None or inv_normal is not None or same_object
    ys, xs = np.mgrid[0:h, 0:w]
    left, right = xs - np.minimum(xs, size), xs + np.minimum(w - xs - 1, size)
    up, down = ys - np.minimum(ys, size), ys + np.minimum(h - ys - 1, size)
    p = img.astype(np.int32)
    col = np.zeros((h, w, 3), F)
    wsum = np.zeros((h, w, 3), F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for dx in range(-size, size + 1):
            for dy in range(-size, size + 1):
                if edges and not abs(dx) + abs(dy) < size:
                    continue
                xi, yi = xs + dx, ys + dy
                take = (xi >= left) & (xi < right) & (yi >= up) & (yi < down)
                if not take.any():
                    continue
                cy, cx = np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)
                q = p[cy, cx]
                t = (q - p).astype(F) / F(255.0)
                arg = F(-inv_spatial) * F(dx * dx + dy * dy) - inv_range * (t * t)
                wt = libm_expf(arg.astype(F))
                if guided:
                    a = np.zeros((h, w), F)
                    if inv_depth is not None:
                        dz = (depth[cy, cx] - depth).astype(F)
                        a = (a + inv_depth * (dz * dz).astype(F)).astype(F)
                    if inv_normal is not None:
                        d = (normal[cy, cx] - normal).astype(F)
                        d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F) + d[..., 2] * d[..., 2]).astype(F)
                        a = (a + (inv_normal * d2).astype(F)).astype(F)
                    ok = a >= 0
                    g = np.where(ok, R.exp_plain(np.where(ok, -a, F(0.0)).astype(F)), F(0.0)).astype(F)
                    if same_object:
                        g = np.where(ids[cy, cx] != ids, F(0.0), g).astype(F)
                    wt = (wt * g[..., None]).astype(F)
                m = take[..., None].repeat(3, axis=2)
                col = np.where(m, col + (q.astype(F) * wt) / F(255.0), col).astype(F)
                wsum = np.where(m, wsum + wt, wsum).astype(F)
        return rust_as_u8((col * F(255.0)) / wsum)


TINY = 2.0 ** -126


def ulp_error(x: np.ndarray, got: np.ndarray):
    """(error in ulp per argument, early_flush mask, not_flushed mask) of got = exp_plain(x) for finite x <= 0."""
    exact = np.exp(x.astype(np.float64))
    _, e = np.frexp(exact)                                   # exact = m 2^e, m in [1/2, 1): the f32 spacing there is 2^(e - 24)
    ulp = np.ldexp(1.0, np.maximum(e - 24, -149))
    g = got.astype(np.float64)
    normal = exact >= TINY
    early = normal & (g == 0.0)
    late = ~normal & (g != 0.0)
    err = np.where(normal, np.abs(np.where(early, TINY, g) - exact) / ulp, 0.0)
    return err, early, late


def mismatch(out, ref):
    bad = np.argwhere(out != ref)
    return None if len(bad) == 0 else (len(bad), bad[:5].tolist(), out[tuple(bad[0])], ref[tuple(bad[0])])
