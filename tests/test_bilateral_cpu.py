"""Rust2's bilateral post-process (Rust2/src/postprocessing.rs:12-131) on the host: rtw_bilateral_filter against an independent numpy
restatement of the reference that evaluates every tap's weight with libm expf, byte for byte, plus known answers and the argument checks."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import rtw_amd as R

F = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
_exp_cache = {}


def libm_expf(a: np.ndarray) -> np.ndarray:
    """libm expf (what Rust's f32::exp lowers to) of every element of an f32 array; evaluated once per distinct argument."""
    bits = np.ascontiguousarray(a, F).view(np.uint32)
    uniq, inv = np.unique(bits.ravel(), return_inverse=True)
    vals = np.empty(len(uniq), F)
    for i, b in enumerate(uniq.tolist()):
        v = _exp_cache.get(b)
        if v is None:
            v = _exp_cache[b] = F(_libm.expf(float(np.uint32(b).view(F))))
        vals[i] = v
    return vals[inv].reshape(a.shape)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def intensity(p):
    """postprocessing.rs:64-68, f32, left to right."""
    r, g, b = (F(v) for v in p)
    return F(F(F(0.2989) * r) / F(255.0)) + F(F(F(0.5870) * g) / F(255.0)) + F(F(F(0.1140) * b) / F(255.0))


def ref_avg_gradient(img):
    """postprocessing.rs:74-87: the serial f32 sum over y in 1..h-1 (outer), x in 1..w-1, then / ((w-2)*(h-2)) as f32."""
    h, w = img.shape[:2]
    inten = np.empty((h, w), F)
    for y in range(h):
        for x in range(w):
            inten[y, x] = intensity(img[y, x])
    s = F(0.0)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            iu, id_, ir, il = inten[y - 1, x], inten[y + 1, x], inten[y, x + 1], inten[y, x - 1]
            s = F(s + np.sqrt(F(F(F(iu - id_) * F(iu - id_)) + F(F(il - ir) * F(il - ir)))))
    return F(s / F((w - 2) * (h - 2)))


def rust_as_u8(v):
    out = np.zeros(v.shape, np.uint8)
    ok = ~np.isnan(v)
    out[ok] = np.clip(np.trunc(v[ok]), 0, 255).astype(np.uint8)
    return out


def ref_bilateral(img, size, edges, avg=None):
    """postprocessing.rs:70-131 with every tap evaluated: returns (out, avg_gradient, taps).  For each pixel the window is
    left..right x up..down (half-open; Proximity::get_pixels, :30-61), column outer, row inner; a tap is taken iff its offset lies in
    the pixel's window, so walking the offsets (dx outer, dy inner, both increasing) visits every pixel's taps in the reference's order."""
    h, w = img.shape[:2]
    spatial = np.ceil(F(F(0.02) * np.sqrt(F(w * w + h * h))))
    if avg is None:
        avg = ref_avg_gradient(img)
    avg = F(avg)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_range = F(F(0.5) / F(avg * avg))
    inv_spatial = F(F(0.5) / F(spatial * spatial))
    ys, xs = np.mgrid[0:h, 0:w]
    left, right = xs - np.minimum(xs, size), xs + np.minimum(w - xs - 1, size)
    up, down = ys - np.minimum(ys, size), ys + np.minimum(h - ys - 1, size)
    p = img.astype(np.int32)
    col = np.zeros((h, w, 3), F)
    wsum = np.zeros((h, w, 3), F)
    taps = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for dx in range(-size, size + 1):
            for dy in range(-size, size + 1):
                if edges and not abs(dx) + abs(dy) < size:
                    continue
                xi, yi = xs + dx, ys + dy
                take = (xi >= left) & (xi < right) & (yi >= up) & (yi < down)
                if not take.any():
                    continue
                taps += int(take.sum())
                q = p[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)]
                k = (q - p).astype(F)
                t = k / F(255.0)
                arg = F(-inv_spatial) * F(dx * dx + dy * dy) - inv_range * (t * t)
                wt = libm_expf(arg.astype(F))
                m = take[..., None].repeat(3, axis=2)
                col = np.where(m, col + (q.astype(F) * wt) / F(255.0), col).astype(F)
                wsum = np.where(m, wsum + wt, wsum).astype(F)
        out = rust_as_u8((col * F(255.0)) / wsum)
    return out, avg, taps


# ---- test images -------------------------------------------------------------------------------------------------------------------
def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_image(h, w, seed):
    """Smooth gradients with a little noise: neighbouring pixels differ by a few levels, as in a rendered frame."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([x / max(1, w - 1) * 200, y / max(1, h - 1) * 180, (x + y) / max(1, w + h - 2) * 150 + 40], axis=2)
    return np.clip(base + rng.normal(0, 2.0, base.shape), 0, 255).astype(np.uint8)


SHAPES = [(3, 3), (5, 7), (48, 64), (61, 97)]          # (h, w): 3x3, 7x5, 64x48, 97x61
SIZES = [0, 1, 3, 10]
PROXIMITIES = [R.PROXIMITY_SQUARE, R.PROXIMITY_EDGES]


def image_cases():
    for i, (h, w) in enumerate(SHAPES):
        yield f"random{w}x{h}", random_image(h, w, 100 + i)
        yield f"smooth{w}x{h}", smooth_image(h, w, 200 + i)


@pytest.mark.parametrize("prox", PROXIMITIES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name,img", list(image_cases()), ids=[n for n, _ in image_cases()])
def test_host_filter_matches_restatement(name, img, size, prox):
    ref, avg, taps = ref_bilateral(img, size, prox == R.PROXIMITY_EDGES)
    out, st = R.bilateral_filter(img, size, prox)
    assert np.float32(st.avg_gradient).view(np.uint32) == avg.view(np.uint32), (st.avg_gradient, avg)
    assert st.taps == taps
    assert st.spatial == np.ceil(F(F(0.02) * np.sqrt(F(img.shape[0] ** 2 + img.shape[1] ** 2))))
    bad = np.argwhere(out != ref)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), out[tuple(bad[0])], ref[tuple(bad[0])])


def test_given_avg_gradient_is_used():
    img = smooth_image(48, 64, 7)
    for avg in (0.01, 0.25, 3.0):
        ref, _, _ = ref_bilateral(img, 3, False, avg=avg)
        out, st = R.bilateral_filter(img, 3, avg_gradient=avg)
        assert st.avg_gradient == F(avg) and np.array_equal(out, ref)
    assert not np.array_equal(R.bilateral_filter(img, 3, avg_gradient=0.01)[0], R.bilateral_filter(img, 3, avg_gradient=3.0)[0])


def test_f32_input_is_quantised_with_rust2_rule():
    rng = np.random.default_rng(5)
    frame = rng.uniform(-0.1, 1.2, (20, 30, 3)).astype(F)
    frame[3, 4, 1] = np.nan
    frame[5, 6, 0] = np.inf
    for prox in PROXIMITIES:
        a, sa = R.bilateral_filter(frame, 4, prox)
        b, sb = R.bilateral_filter(R.quantize_u8_rust2(frame), 4, prox)
        assert np.array_equal(a, b) and sa.avg_gradient == sb.avg_gradient


# ---- known answers -------------------------------------------------------------------------------------------------------------------
def test_uniform_image_is_all_zero():
    """avg = 0 -> inv_range = inf -> the dc = 0 weight is exp(inf * 0) = exp(NaN): every output byte becomes 0 (as u8 of NaN)."""
    img = np.full((16, 20, 3), 137, np.uint8)
    for prox in PROXIMITIES:
        out, st = R.bilateral_filter(img, 3, prox)
        assert st.avg_gradient == 0.0 and not out.any()


def test_size_zero_is_all_zero():
    """An empty window: 0 / 0 -> NaN -> 0."""
    img = random_image(12, 9, 3)
    for prox in PROXIMITIES:
        out, st = R.bilateral_filter(img, 0, prox)
        assert st.taps == 0 and not out.any()


def test_window_excludes_the_plus_size_column_and_row():
    """3x3, size 1: the window of (x, y) is x - min(x,1) .. x + min(2-x,1) by y - min(y,1) .. y + min(2-y,1), half-open, so no pixel
    ever sees its right-hand or lower neighbour, and the last column and row never see themselves.  Black with a white last column
    (or row): every tap any pixel takes is black, so the whole output is black -- a symmetric window would mix the white in."""
    for axis in (1, 0):
        img = np.zeros((3, 3, 3), np.uint8)
        if axis == 1:
            img[:, 2] = 255
        else:
            img[2, :] = 255
        out, st = R.bilateral_filter(img, 1)
        assert st.taps == 4 + 2 * 2 + 2 * 2 + 1 * 4        # centre 2x2; edge-middles 2x1 or 1x2 (4 of them); corners 1x1
        assert np.isfinite(st.avg_gradient) and st.avg_gradient > 0
        assert not out.any(), out[..., 0]
        ref, _, _ = ref_bilateral(img, 1, False)
        assert np.array_equal(out, ref)
    # the bottom-right pixel's only tap is (1, 1): with a given range term (avg 1 -> inv_range 0.5) its value comes through, weighted
    img = np.zeros((3, 3, 3), np.uint8)
    img[1, 1] = (255, 128, 8)
    out, st = R.bilateral_filter(img, 1, avg_gradient=1.0)
    assert st.spatial == 1.0                                                     # ceil(0.02 * sqrt(18)); inv_spatial = 0.5
    for c, v in enumerate((255, 128, 8)):
        t = F(F(v) / F(255.0))
        wt = F(_libm.expf(float(F(F(-0.5) * F(2.0)) - F(F(0.5) * F(t * t)))))     # d2 = 2, k = v - 0
        assert out[2, 2, c] == int(F(F(F(F(F(v) * wt) / F(255.0)) * F(255.0)) / wt)), (c, out[2, 2])
    assert out[2, 2].tolist() != [0, 0, 0]


def count_taps(w, h, s, edges):
    """Proximity::get_pixels (postprocessing.rs:30-61) counted pixel by pixel."""
    n = 0
    for y in range(h):
        for x in range(w):
            left, right = x - min(x, s), x + min(w - x - 1, s)
            up, down = y - min(y, s), y + min(h - y - 1, s)
            for i in range(left, right):
                for j in range(up, down):
                    if not edges or abs(x - i) + abs(y - j) < s:
                        n += 1
    return n


@pytest.mark.parametrize("w,h,s", [(3, 3, 1), (7, 5, 3), (20, 11, 4), (13, 17, 10)])
def test_tap_count(w, h, s):
    img = random_image(h, w, 9)
    for prox in PROXIMITIES:
        _, st = R.bilateral_filter(img, s, prox)
        assert st.taps == count_taps(w, h, s, prox == R.PROXIMITY_EDGES)
    _, sq = R.bilateral_filter(img, s, R.PROXIMITY_SQUARE)
    _, ed = R.bilateral_filter(img, s, R.PROXIMITY_EDGES)
    assert ed.taps < sq.taps


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def _raw(img_ptr, w, h, prm, out_ptr, st=None):
    return R.lib().rtw_bilateral_filter(img_ptr, w, h, prm, out_ptr, st)


def test_error_paths_host():
    img = random_image(8, 8, 1)
    out = np.empty_like(img)
    ip, op = C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    ok = R.RtwBilateral(2, R.PROXIMITY_SQUARE, R.PIXELS_U8, 0.0)
    assert _raw(ip, 8, 8, C.byref(ok), op) == 0                               # stats may be NULL
    assert _raw(None, 8, 8, C.byref(ok), op) == -1
    assert _raw(ip, 8, 8, None, op) == -1
    assert _raw(ip, 8, 8, C.byref(ok), None) == -1
    assert _raw(ip, 2, 8, C.byref(ok), op) == -1                              # (w-2)*(h-2) underflows
    assert _raw(ip, 8, 2, C.byref(ok), op) == -1
    assert _raw(ip, 65536, 3, C.byref(ok), op) == -1                          # w*w + h*h overflows u32 (checked before any read)
    bad = [R.RtwBilateral(2, 2, R.PIXELS_U8, 0.0), R.RtwBilateral(2, R.PROXIMITY_SQUARE, 2, 0.0),
           R.RtwBilateral(R.BILATERAL_MAX_SIZE + 1, R.PROXIMITY_SQUARE, R.PIXELS_U8, 0.0)]
    bad += [R.RtwBilateral(2, R.PROXIMITY_SQUARE, R.PIXELS_U8, v) for v in (-1.0, float("nan"), float("inf"))]
    for prm in bad:
        assert _raw(ip, 8, 8, C.byref(prm), op) == -1, (prm.size, prm.proximity, prm.in_format, prm.avg_gradient)
    big = random_image(3, 3, 2)
    out, _ = R.bilateral_filter(big, R.BILATERAL_MAX_SIZE)                    # the cap itself is accepted
    with pytest.raises(R.RtwError):
        R.bilateral_filter(big, R.BILATERAL_MAX_SIZE + 1)
    with pytest.raises(ValueError):
        R.bilateral_filter(big.astype(np.int16), 1)
    with pytest.raises(ValueError):
        R.bilateral_filter(big[..., :2], 1)


def test_pod_layout():
    assert C.sizeof(R.RtwBilateral) == 16 and C.sizeof(R.RtwFilterStats) == 32 and R.RtwFilterStats.taps.offset == 24
