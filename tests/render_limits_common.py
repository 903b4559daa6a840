"""Shared cases of the render-limit tests (test_render_limits_cpu.py, test_gpu_render_limits.py, test_gpu_resolve_edges.py).

A: frame shapes at the limits rtw.h declares (width, height <= 65535): the render kernels keep `column | row << 16` in one register, the
pixel id `j * width + i` in 32 bits.  B: sample counts at the shim's limit (2^24 - 1: `sample | samples left << 24`).  C: the value edges
of the resolve (sum in sample order, division, powf(mean, 1 / gamma)), fed through the background colour of an empty scene.

Everything here is host work (numpy and the CPU oracle); the oracle's frames are computed once per process and handed out unchanged."""
import functools

import numpy as np

import rtw_amd as R
from tests import oracle_binding as O

f32 = np.float32
DIM_MAX = 65535                     # RtwParams.width / height (rtw.h)
SAMPLES_MAX = (1 << 24) - 1         # the count a sampler may trace (rtw_shim.hip)
ROOT_MAX = 4095                     # the largest s_root: 4095^2 = 16 769 025 < 2^24 <= 4096^2
E_INVALID = -1
THREADS = 16

# ---- A: frames ----------------------------------------------------------------------------------------------------------------------
# The part of the bench camera's viewport every frame is stretched over, whatever its aspect: left .. right, top .. bottom as fractions.
# Below the horizon of Book-1's final scene, where the ground and the sphere field are.
WINDOW = (0.1, 0.9, 0.45, 0.95)


def field_camera(width, height):
    """The bench camera (origin, lens) with pixel00 / delta_u / delta_v written by hand: pixel (0, 0) .. (width, height) spans WINDOW."""
    cam, p = R.default_view(R.SCENE_C5)           # the framing bench.py renders; static scene: no shutter
    cam.shutter, cam.time0 = 0.0, 0.0
    p00 = np.array(cam.pixel00[:], np.float64)
    full_u = np.array(cam.delta_u[:], np.float64) * p.width
    full_v = np.array(cam.delta_v[:], np.float64) * p.height
    l, r, t, b = WINDOW
    for k in range(3):
        cam.pixel00[k] = p00[k] + l * full_u[k] + t * full_v[k]
        cam.delta_u[k] = (r - l) * full_u[k] / width
        cam.delta_v[k] = (b - t) * full_v[k] / height
    return cam


def frame_params(width, height, samples=1, partition=(8, 0, 1), flags=0):
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth = width, height, samples, 3
    p.gamma, p.mint, p.maxt = 1.0, 0.001, 100000.0
    p.integrator, p.sampler, p.accel, p.flags, p.seed = R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, R.ACCEL_BVH, flags, 1
    p.row_block, p.part_index, p.part_count = partition
    return p


# name -> (width, height, samples, (row_block, part_index, part_count), rows rendered)
FRAMES = {
    "65535x1": (DIM_MAX, 1, 1, (8, 0, 1), 1),                              # 8192 tiles in one tile row, 7 of 8 rows of each padding
    "65534x1": (DIM_MAX - 1, 1, 1, (8, 0, 1), 1),
    "1x65535": (1, DIM_MAX, 1, (8, 0, 1), DIM_MAX),                        # one tile column, 8192 tile rows
    "corner row": (DIM_MAX, DIM_MAX, 1, (1, DIM_MAX - 1, DIM_MAX), 1),     # image row 65534 alone: pixel ids up to 4 294 836 224, (column, row) up to 0xFFFEFFFE
    "corner block": (DIM_MAX, DIM_MAX, 1, (8, 8191, 8192), 7),             # the ragged last block: rows 65528 .. 65534
    "corner block 6spp": (DIM_MAX, DIM_MAX, 6, (8, 8191, 8192), 7),
    "65535x24": (DIM_MAX, 24, 1, (8, 0, 1), 24),                           # the multi-context frame, 786 420-byte rows
}

# The four kinds of build every frame runs through: (expected build, accel, RTW_OPT_NODE_FORMAT, extra flags); the tree is forced
# (RTW_OPT_LIST_WALK_MAX = 0) for the three that want it.
BUILDS = (
    ("render_brute<", R.ACCEL_BRUTE, 0, 0),
    ("render_bvh<0,1,1,0>", R.ACCEL_BVH, 0, 0),                             # 768 threads, f32 planes: the automatic choice
    ("render_bvh<0,2,1,0>", R.ACCEL_BVH, 1, 0),                             # f16 nodes, geometry in LDS
    ("render_bvh<0,0,1,0>", R.ACCEL_BVH, 0, R.FLAG_GLOBAL_NODES),           # nodes in global memory
)


def book1():
    return R.Scene.generate(R.SCENE_C2, 42)


def frame_case(name):
    """(camera, params) of a frame of FRAMES."""
    w, h, n, part, _ = FRAMES[name]
    return field_camera(w, h), frame_params(w, h, n, part)


@functools.lru_cache(maxsize=None)
def _frame_oracle(name):
    cam, p = frame_case(name)
    img, st = O.render(cam, book1(), p, THREADS)
    img.setflags(write=False)
    return img, st


def frame_oracle(name):
    """(frame, RtwStats) of the CPU oracle for a frame of FRAMES: computed once, read-only."""
    return _frame_oracle(name)


def bank_gb_for_band(tiles_x, slots, band_tile_rows):
    """RTW_OPT_SAMPLE_BANK_GB for bands of `band_tile_rows` tile rows: the documented bank is 64 slots of 12 bytes per tile and
    sample (per tile and unit under RTW_FLAG_CHUNK_SUMS), `slots` of them per tile.  Half a tile row on top keeps the budget clear of
    the rounding of the GiB figure."""
    tile_row_bytes = tiles_x * slots * 64 * 12
    return (band_tile_rows + 0.5) * tile_row_bytes / float(1 << 30)


# ---- B: sample counts ---------------------------------------------------------------------------------------------------------------
def sampler_count(sampler, samples):
    """The rays a sampler traces per pixel (rtw.h RTW_SAMPLER_*), in the f32 arithmetic of the library: (count, root)."""
    if sampler == R.SAMPLER_STRATIFIED:
        root = int(np.ceil(np.sqrt(f32(samples))))
        return root * root, root
    if sampler == R.SAMPLER_CENTRES:
        root = int(np.floor(np.sqrt(f32(samples))))
        return root * root, root
    if sampler == R.SAMPLER_NO_RAND:
        return 1, 0
    return samples, 0


# (integrator, sampler, samples, camera rays per pixel or None when the render is refused)
SAMPLE_CASES = (
    (R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, SAMPLES_MAX, SAMPLES_MAX),
    (R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, 1 << 24, None),
    (R.INTEGRATOR_GRADIENT, R.SAMPLER_STRATIFIED, ROOT_MAX * ROOT_MAX, ROOT_MAX * ROOT_MAX),
    (R.INTEGRATOR_GRADIENT, R.SAMPLER_STRATIFIED, ROOT_MAX * ROOT_MAX + 1, None),       # root 4096
    (R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, SAMPLES_MAX, ROOT_MAX * ROOT_MAX),
    (R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 1 << 24, None),
    (R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 1, 1),
    (R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 2, 1),
    (R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 3, 1),
    (R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, 0, None),
)


def empty_scene(background=(0.0, 0.0, 0.0)):
    return R.Scene((), background=background)


def pixel_camera():
    """A camera for the 1 x 1 frames of an empty scene: every path is a miss, whatever it looks at."""
    return field_camera(1, 1)


def pixel_params(integrator, sampler, samples, flags=0, width=1, height=1, depth=3):
    p = frame_params(width, height, samples, flags=flags)
    p.integrator, p.sampler, p.depth, p.accel = integrator, sampler, depth, R.ACCEL_BRUTE
    return p


@functools.lru_cache(maxsize=None)
def _pixel_oracle(integrator, sampler, samples, flags, background):
    img, st = O.render(pixel_camera(), empty_scene(background), pixel_params(integrator, sampler, samples, flags), 1)
    img.setflags(write=False)
    return img, st


def pixel_oracle(integrator, sampler, samples, flags=0, background=(0.0, 0.0, 0.0)):
    """The oracle's 1 x 1 frame of the empty scene (one thread; 16.7 M misses take it a second or two): once per process, read-only."""
    return _pixel_oracle(integrator, sampler, samples, flags, tuple(background))


# ---- C: the resolve ---------------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(f32).max)
INF, NAN = float("inf"), float("nan")
# twenty edge values, and 1e-20 in the slot left over: with gamma 0.5 it is the one input of the grid whose result (1e-40) is subnormal
RESOLVE_VALUES = (0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 1e-30, 1e-3, 0.18, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 2.0, 255.0, 1e30,
                  FLT_MAX, INF, -1e-30, -0.5, -INF, NAN, 1e-20)
RESOLVE_FRAMES = tuple(RESOLVE_VALUES[k:k + 3] for k in range(0, len(RESOLVE_VALUES), 3))          # seven backgrounds of three
RESOLVE_GAMMAS = (1.0, 2.0, 2.2, 2.4, 0.5, 3.0, 1e-3, 1e3, 0.0, INF, -2.0, NAN)
RESOLVE_SAMPLES = (1, 4)
RESOLVE_ULP = 2                     # DESIGN.md "Parity": powf is the one stage with a tolerance


def resolve_params(gamma, samples, width=8, height=8):
    """RUST2 at depth 0 through the fixed-centre sampler: every sample of every pixel is the background colour as given (rtw.h)."""
    p = pixel_params(R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, samples, width=width, height=height, depth=0)
    p.gamma = gamma
    return p


def pow_reference(L, gamma):
    """The plain f64 reference of the gamma step for a gamma-1 frame L (f32), rounded to f32."""
    with np.errstate(all="ignore"):
        e = np.float64(f32(1) / f32(gamma))
        return np.power(np.asarray(L, np.float64), e).astype(f32)


def ordered(x):
    """f32 -> int64 that orders like the reals and counts units of the last place, subnormals and the two zeros (one place) included."""
    i = np.ascontiguousarray(x, f32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def value_class(x):
    """0 for a finite non-zero value, else a code of its own for NaN, +inf, -inf, +0, -0."""
    x = np.asarray(x, f32)
    c = np.zeros(x.shape, np.int8)
    c[np.isnan(x)] = 1
    c[np.isposinf(x)] = 2
    c[np.isneginf(x)] = 3
    zero = x == 0
    c[zero & ~np.signbit(x)] = 4
    c[zero & np.signbit(x)] = 5
    return c


def same_bits(a, b):
    """Bit equality with every NaN equal to every NaN; the sign of zero counts."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def compare_pow(got, want):
    """(same class everywhere, worst distance in units of the last place over the finite non-zero `want`, all of those finite in `got`)."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    cw = value_class(want)
    special = cw != 0
    classes_ok = bool(np.all(value_class(got)[special] == cw[special]))
    fin = ~special
    finite_ok = bool(np.all(np.isfinite(got[fin])))
    worst = int(np.abs(ordered(got[fin]) - ordered(want[fin])).max()) if fin.any() else 0
    return classes_ok, worst, finite_ok


def nan_pixel_count(img):
    return int(np.isnan(np.asarray(img)).any(axis=-1).sum())


# the sum's order: every sample of every pixel is the background b, so a pixel is sum_n(b) / n in the order the image's definition fixes
SUM_BACKGROUND = (0.1, 3.0, 1e-3)
SUM_COUNTS = (3, 4, 5, 37, 255, 256, 257, 1000)
SUM_CHUNK_LENS = (0, 1, 7, 255)
SUM_BIG_BACKGROUND = (3.0, 0.1, 1.0)
SUM_CHUNK = 4                       # RTW_SUM_CHUNK (rtw.h)


def sum_params(samples, flags=0, width=9, height=9):
    return pixel_params(R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, samples, flags, width, height)


def mean_in_order(background, n):
    """viewport.rs:299-301 for n equal samples: (((0 + b) + b) + b) + .. left to right, then / n, per channel: [3] f32.  The sum starts from
    +0 as the reference's does, so this is np.add.accumulate(np.full(n, b, f32))[-1] / f32(n) for every b but -0, which it turns into +0."""
    return f32([np.add.accumulate(np.concatenate((f32([0]), np.full(n, b, f32))))[-1] / f32(n) for b in background])


def mean_chunk_sums(background, n):
    """RTW_FLAG_CHUNK_SUMS (rtw.h): chunks of RTW_SUM_CHUNK samples added left to right, the chunks' sums added in chunk order, then / n."""
    out = []
    for b in background:
        run = np.add.accumulate(np.full(SUM_CHUNK, b, f32))           # run[k - 1] = a chunk of k samples
        parts = np.full((n + SUM_CHUNK - 1) // SUM_CHUNK, run[SUM_CHUNK - 1], f32)
        if n % SUM_CHUNK:
            parts[-1] = run[n % SUM_CHUNK - 1]
        out.append(np.add.accumulate(parts)[-1] / f32(n))
    return f32(out)
