"""Shared by the post-process edge tests (test_filter_edges_cpu.py, test_gpu_filter_edges.py): the case tables and numpy references for
A. Rust2's quantisation at its ties and special values, B. the gradient sum at its vector, chunk and tail boundaries, C. the guided filter
with non-finite and extreme guides, D. small frame geometries.  numpy only; every reference here is independent of the library except
ref_guided's exp_plain (pinned on its own by test_guided_cpu.py and test_gpu_device_math.py)."""
import functools

import numpy as np

import rtw_amd as R
from tests.guided_common import guides, ref_guided
from tests.test_bilateral_cpu import F, intensity, random_image, ref_avg_gradient, ref_bilateral, smooth_image

PROXIMITIES = [R.PROXIMITY_SQUARE, R.PROXIMITY_EDGES]
PROX_IDS = ["square", "edges"]
INF, NAN = F(np.inf), F(np.nan)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- A. quantisation ---------------------------------------------------------------------------------------------------------------
Q = F(255.99)


def product(c):
    """c * 255.99 in f32, as Vec3::to_rgb_u8 forms it."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(c, F) * Q).astype(F)


def _clamped(c):
    """(the product clamped to [0, 255] as float64, the NaN mask)"""
    v = product(c)
    nan = np.isnan(v)
    return np.clip(np.where(nan, F(0.0), v), F(0.0), F(255.0)).astype(np.float64), nan


def ref_quantize_rust2(c):
    """Rust2 Vec3::to_rgb_u8: (c * 255.99f32).clamp(0, 255).round() as u8.  f32::round rounds half away from zero, and `as u8` of NaN is 0.
    The rounding is done in float64, where v - floor(v) is exact: no f32 `floor(v + 0.5)`, whose sum rounds."""
    v, nan = _clamped(c)
    fl = np.floor(v)
    return np.where(nan, 0.0, fl + (v - fl >= 0.5)).astype(np.uint8)


def quantize_half_even(c):
    """The first wrong rule the value set must expose: ties to even (rint)."""
    v, nan = _clamped(c)
    return np.where(nan, 0.0, np.rint(v)).astype(np.uint8)


def quantize_floor_plus_half_f32(c):
    """The second: floor(v + 0.5f) with the sum formed in f32 -- pred(0.5) + 0.5 rounds up to 1."""
    v, nan = _clamped(c)
    return np.where(nan, F(0.0), np.floor((v.astype(F) + F(0.5)).astype(F))).astype(np.uint8)


def _neighbours(c, k=3):
    out, lo, hi = [c], c, c
    for _ in range(k):
        lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        out += [lo, hi]
    return out


def tie_values():
    """For every byte k the f32 nearest (k + 0.5) / 255.99 and its three neighbours on either side: 1792 values around the 256 ties."""
    vals = []
    for k in range(256):
        vals += _neighbours(F((k + 0.5) / 255.99))
    return np.array(vals, F)


def special_values():
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FA00001, 0xFFA00001], np.uint32).view(F)      # quiet, both signs; signalling with a payload
    top = F(255.0) / Q
    return np.concatenate([
        np.array([0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126], F),         # zeros, the smallest denormals, the smallest normal
        np.array(_neighbours(top, 1), F),                                           # 255 / 255.99: where the clamp starts to matter
        np.array([1.0, np.nextafter(F(1.0), INF), -1e-3, 1e30, -1e30, 3.4e38], F),  # 3.4e38 * 255.99 overflows to +inf
        np.array([np.inf, -np.inf], F), nans])


@functools.lru_cache(maxsize=None)
def quantize_values():
    v = np.concatenate([tie_values(), special_values()])
    v.setflags(write=False)
    return v


QUANT_H, QUANT_W = 19, 32                                   # 19 * 32 * 3 = 1824 slots for the 1792 + 20 values


@functools.lru_cache(maxsize=None)
def quantize_frame():
    """The values laid into the [0:H, 0:W] part of an (H+1) x (W+1) x 3 f32 frame (the rest 0.25): with size 1, Edges and a given
    avg_gradient of 1 every pixel outside the last row and column takes the single tap (0, 0) with weight expf(-0) = 1, and the output byte
    trunc(f32(f32(q / 255) * 255)) is q itself -- the filter shows the quantised bytes exactly (read_out_holds_for_every_byte pins that)."""
    v = quantize_values()
    assert len(v) <= QUANT_H * QUANT_W * 3
    inner = np.full(QUANT_H * QUANT_W * 3, 0.25, F)
    inner[:len(v)] = v
    frame = np.full((QUANT_H + 1, QUANT_W + 1, 3), 0.25, F)
    frame[:-1, :-1] = inner.reshape(QUANT_H, QUANT_W, 3)
    frame.setflags(write=False)
    return frame


READ_OUT = dict(size=1, proximity=R.PROXIMITY_EDGES, avg_gradient=1.0)


def check_read_out(out, want_bytes):
    """`out` of a READ_OUT filter call shows `want_bytes` (a frame of the same shape) outside the last row and column, which are 0."""
    bad = np.argwhere(out[:-1, :-1] != want_bytes[:-1, :-1])
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), out[tuple(bad[0])], want_bytes[tuple(bad[0])])
    assert not out[-1].any() and not out[:, -1].any()


# ---- B. the gradient sum ------------------------------------------------------------------------------------------------------------
# every n % 4, the terms kernel's block of 256, both sides of one and of two 2048-term chunks, an exact multiple of the chunk
TERM_COUNTS = [1, 2, 3, 4, 5, 6, 7, 255, 256, 257, 2046, 2047, 2048, 2049, 2050, 2051, 4095, 4096, 4097, 6144, 6146]
TAIL_COUNTS = [2049, 2050, 2051, 4097]                      # the last chunk holds 1, 2, 3 and 1 terms
REF_BYTES_MAX_N = 2051                                      # up to here the filter's bytes are compared with ref_bilateral's as well
ORIENTATIONS = ["wide", "tall"]
# The draw of a frame is seed 7000 + n, except where that draw does not pin the order of the sum (test_filter_edges_cpu.py: one of the
# other orders gives the serial sum's avg_gradient bits); there the first of 17000 + n, 27000 + n, ... that does.
RESEEDED = {255: 17255, 256: 27256, 2046: 19046, 6144: 23144}


@functools.lru_cache(maxsize=None)
def thin_frame(n, orientation):
    """3 x (n + 2) random pixels: one interior row, n terms; "tall" is its transpose, (n + 2) x 3: n interior rows of one term (the same
    terms in the same order, reached through the other index arithmetic)."""
    img = random_image(3, n + 2, RESEEDED.get(n, 7000 + n))
    if orientation == "tall":
        img = np.ascontiguousarray(img.transpose(1, 0, 2))
    img.setflags(write=False)
    return img


def gradient_terms(img):
    """The terms of postprocessing.rs:74-87 in the order the reference adds them (y outer, x inner), each operation one f32 rounding."""
    p = img.astype(F)
    inten = (F(0.2989) * p[..., 0]) / F(255.0) + (F(0.5870) * p[..., 1]) / F(255.0) + (F(0.1140) * p[..., 2]) / F(255.0)
    iu, id_, ir, il = inten[:-2, 1:-1], inten[2:, 1:-1], inten[1:-1, 2:], inten[1:-1, :-2]
    t = np.sqrt((iu - id_) * (iu - id_) + (il - ir) * (il - ir))
    assert t.dtype == F
    return t.ravel()


def serial_sum(terms):
    s = F(0.0)
    for t in terms:
        s = F(s + t)
    return s


def other_order_sums(terms):
    """The same terms added in three other orders, in f32: pairwise, as four strided partial sums, and from the far end."""
    parts = [serial_sum(terms[i::4]) for i in range(4)]
    return {"pairwise": F(np.sum(terms, dtype=F)), "four strided partial sums": F(F(F(parts[0] + parts[1]) + parts[2]) + parts[3]),
            "reversed": serial_sum(terms[::-1])}


@functools.lru_cache(maxsize=None)
def thin_avg(n, orientation):
    """ref_avg_gradient of thin_frame: the serial Python loop, computed once per frame."""
    return ref_avg_gradient(thin_frame(n, orientation))


@functools.lru_cache(maxsize=None)
def thin_bytes(n, orientation):
    """ref_bilateral(thin_frame, 3, Square) with the reference's own range term: (bytes, taps)."""
    out, _, taps = ref_bilateral(thin_frame(n, orientation), 3, False, avg=thin_avg(n, orientation))
    return out, taps


TAIL_PIXEL = (200, 0, 0), (0, 131, 0), (0, 0, 255), (17, 0, 0)        # one channel each, in the order of TAIL_COUNTS


def single_term_frame(n, last, value):
    """All zero but one pixel of the top row, above interior pixel x = w - 2 (`last`) or x = 1: only term n - 1 (or term 0) is non-zero and
    equals that pixel's intensity, so avg_gradient = f32(intensity / f32(n)) -- and 0 if that term is dropped."""
    img = np.zeros((3, n + 2, 3), np.uint8)
    img[0, n if last else 1] = value
    return img, F(intensity(value) / F(n))


def single_term_cases():
    for n, value in zip(TAIL_COUNTS, TAIL_PIXEL):
        for last in (True, False):
            yield n, last, value


SINGLE_TERM_IDS = [f"{n}-{'last' if last else 'first'}" for n, last, _ in single_term_cases()]


# ---- C. the guided filter with non-finite and extreme guides --------------------------------------------------------------------------
GUIDED_SHAPES = [(17, 33), (37, 70)]
GUIDED_SIZES = [3, 10]
GUIDED_AVG = 0.1
GUIDED_LAYOUTS = {"guides in LDS": 2, "guides in global memory": 4}       # RTW_OPT_GUIDED_LAYOUT
SD, SN = 0.5, 0.3                                                         # the ordinary sigmas
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def guided_image(h, w):
    img = smooth_image(h, w, 400 + h)
    img.setflags(write=False)
    return img


def _sprinkle(h, w, seed, p=0.08):
    return np.random.default_rng(seed).random((h, w)) < p


def _block(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return (y >= h // 3) & (y < 2 * h // 3) & (x >= w // 3) & (x < 2 * w // 3)


def _steps(h, w, seed, lo, hi):
    """A plane whose neighbouring pixels differ by a step in [lo, hi) each way."""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.uniform(lo, hi, w))[None, :] + np.cumsum(rng.uniform(lo, hi, h))[:, None]


def _depth_case(fill):
    def make(h, w):
        depth = guides(h, w)[0].copy()
        fill(depth, h, w)
        return dict(depth=depth, sigma_depth=SD)
    return make


def _d_nan(d, h, w):
    d[_sprinkle(h, w, 1)] = NAN


def _d_pinf(d, h, w):                                   # scene_hits' miss plane: a block of +inf (neighbours: inf - inf) beside finite depths
    d[_block(h, w) | _sprinkle(h, w, 2, 0.04)] = INF


def _d_ninf(d, h, w):
    d[_sprinkle(h, w, 3) | (_block(h, w) & (np.mgrid[0:h, 0:w][1] % 2 == 0))] = -INF


def _d_checker(value):
    def fill(d, h, w):                                  # +value next to -value inside the block, ordinary depths around it
        y, x = np.mgrid[0:h, 0:w]
        d[_block(h, w)] = np.where((x + y) % 2 == 0, F(value), F(-value))[_block(h, w)]
    return fill


def _d_all_nan(d, h, w):
    d[:] = NAN


def _depth_huge_sigma(h, w):                            # inv_depth = 0.5 / 1e38: a denormal; steps of 1e18 .. 1e19 give a in [0.005, 0.5]
    return dict(depth=_steps(h, w, 4, 1e18, 1e19).astype(F), sigma_depth=1e19)


def _depth_tiny_sigma(h, w):                            # inv_depth = 5e37; steps of 1e-19: dz^2 = 1e-38 is a denormal, a = 0.5
    rng = np.random.default_rng(5)
    k = np.cumsum(rng.integers(0, 3, w))[None, :] + np.cumsum(rng.integers(0, 3, h))[:, None]
    return dict(depth=(F(1e-19) * k.astype(F)).astype(F), sigma_depth=1e-19)


def _normal_huge_sigma(h, w):                           # |dn|^2 up to 1e38 (a miss against a unit normal): finite, a up to 0.5
    return dict(normal=(guides(h, w)[1] * F(1e19)).astype(F), sigma_normal=1e19)


def _normal_tiny_sigma(h, w):                           # |dn|^2 of 4e-39 .. 1e-38: denormals, a of 0.2 .. 0.5
    return dict(normal=(guides(h, w)[1] * F(1e-19)).astype(F), sigma_normal=1e-19)


def _normal_nonfinite(h, w):
    n = guides(h, w)[1].copy()
    for c, (v, seed) in enumerate(((NAN, 6), (INF, 7), (-INF, 8))):
        n[_sprinkle(h, w, seed, 0.04), c] = v
    blk = _block(h, w)
    n[blk, 1] = INF                                      # inf next to inf: inf - inf
    return dict(normal=n, sigma_normal=SN)


def _normal_1e20(h, w):                                 # the squared distance overflows: a = +inf, the tap weighs +0
    n = guides(h, w)[1].copy()
    y, x = np.mgrid[0:h, 0:w]
    blk = _block(h, w)
    n[blk] = np.where(((x + y) % 2 == 0)[..., None], np.array([1e20, 0.0, -1e20], F), np.array([-1e20, 1e20, 0.0], F))[blk]
    return dict(normal=n, sigma_normal=SN)


def _id_plane(h, w):
    y, x = np.mgrid[0:h, 0:w]
    ids = np.array([I32_MIN, I32_MAX, -1, -2, 0], np.int64)[(x // 3 + 2 * (y // 2)) % 5]
    ids[_sprinkle(h, w, 9, 0.05)] = I32_MAX
    return ids.astype(np.int32)


def _ids_extremes(h, w):
    return dict(ids=_id_plane(h, w), same_object=True)


def _combined(h, w):
    """All three terms on, the edge values of each plane at pixels of their own."""
    y, x = np.mgrid[0:h, 0:w]
    depth, normal, _ = (g.copy() for g in guides(h, w))
    depth[_sprinkle(h, w, 10, 0.03)] = NAN
    depth[(y < h // 4) & (x < w // 4)] = INF
    depth[_sprinkle(h, w, 11, 0.03)] = -INF
    depth[(y >= 3 * h // 4) & (x < w // 4)] = np.where((x + y) % 2 == 0, F(3e38), F(-3e38))[(y >= 3 * h // 4) & (x < w // 4)]
    normal[_sprinkle(h, w, 12, 0.03), 0] = NAN
    normal[_sprinkle(h, w, 13, 0.03), 2] = -INF
    normal[(y >= 3 * h // 4) & (x >= 3 * w // 4)] = np.array([1e20, -1e20, 1e20], F)
    y0 = (y >= h // 3) & (y < 2 * h // 3)
    ids = np.where(y0, _id_plane(h, w), 0).astype(np.int32)
    return dict(depth=depth, sigma_depth=SD, normal=normal, sigma_normal=SN, ids=ids, same_object=True)


# name -> (h, w) -> the guide arguments of guided_filter / ref_guided
GUIDED_CASES = {
    "depth-nan": _depth_case(_d_nan), "depth-plus-inf": _depth_case(_d_pinf), "depth-minus-inf": _depth_case(_d_ninf),
    "depth-3e38": _depth_case(_d_checker(3e38)), "depth-1e20": _depth_case(_d_checker(1e20)), "depth-all-nan": _depth_case(_d_all_nan),
    "depth-sigma-1e19": _depth_huge_sigma, "depth-sigma-1e-19": _depth_tiny_sigma,
    "normal-sigma-1e19": _normal_huge_sigma, "normal-sigma-1e-19": _normal_tiny_sigma,
    "normal-nonfinite": _normal_nonfinite, "normal-1e20": _normal_1e20,
    "ids-extremes": _ids_extremes, "combined": _combined,
}
DEAD_CENTRE_CASES = {"depth-nan", "depth-plus-inf", "depth-minus-inf", "depth-all-nan", "combined"}     # they hold non-finite depths
BLACK_CASES = {"depth-all-nan"}                             # every tap dropped: the frame comes out all zero
# the cases whose term must stay visible with a denormal inv_* or a denormal squared distance: a flushed operand would make g = 1
DENORMAL_CASES = {"depth-sigma-1e19": "sigma_depth", "depth-sigma-1e-19": "sigma_depth", "normal-sigma-1e19": "sigma_normal",
                  "normal-sigma-1e-19": "sigma_normal"}


@functools.lru_cache(maxsize=None)
def guided_case(name, h, w):
    kw = GUIDED_CASES[name](h, w)
    for a in kw.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return kw


def ordinary_guides(kw, h, w):
    """The same call with guided_common's ordinary planes and sigmas in place of the case's."""
    depth, normal, ids = guides(h, w)
    out = dict(kw)
    if "depth" in kw:
        out.update(depth=depth, sigma_depth=SD)
    if "normal" in kw:
        out.update(normal=normal, sigma_normal=SN)
    if "ids" in kw:
        out.update(ids=ids)
    return out


@functools.lru_cache(maxsize=None)
def guided_ref(name, h, w, size, prox):
    """ref_guided of one case, computed once."""
    out = ref_guided(guided_image(h, w), size, prox == R.PROXIMITY_EDGES, GUIDED_AVG, **guided_case(name, h, w))
    out.setflags(write=False)
    return out


def dead_centres(kw):
    """Pixels whose depth is NaN or infinite (with the depth term on): all their taps are dropped or weigh +0 -> 0 / 0 -> bytes 0 0 0."""
    return ~np.isfinite(kw["depth"]) if kw.get("sigma_depth", 0.0) > 0 else None


# ---- D. frame geometry ----------------------------------------------------------------------------------------------------------------
GEOMETRY_SHAPES = [(3, 64), (3, 65), (15, 31), (16, 32), (17, 33), (32, 3), (33, 3)]       # (h, w) around the 32 x 16 workgroup
GEOMETRY_SIZES = [1, 16, 64]                                                                # 16, 64: clipped on both sides, wider than the frame
ALL_TERMS = dict(sigma_depth=SD, sigma_normal=SN, same_object=True)
# a given avg_gradient whose square underflows to 0 (inv_range = inf: all zero), is a denormal (inv_range finite), overflows (inv_range = 0)
AVG_EXTREMES = [1e-30, 1e-19, 1e30]


@functools.lru_cache(maxsize=None)
def geometry_image(h, w):
    img = random_image(h, w, 500 + 7 * h + w) if (h + w) % 2 else smooth_image(h, w, 500 + 7 * h + w)
    img.setflags(write=False)
    return img


def geometry_guides(h, w):
    return dict(zip(("depth", "normal", "ids"), guides(h, w)), **ALL_TERMS)
