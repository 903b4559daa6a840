#!/usr/bin/env python3
"""The guided filter's numbers for DESIGN.md 8b.

  timings  filter_ms (the kernel alone, hipEvent) at 1920 x 1080, size 10, Square: rtw_ctx_bilateral_filter, and rtw_ctx_guided_filter with
           all three guides under every RTW_OPT_GUIDED_LAYOUT (the LDS A/B) and with each guide alone under the layout chosen by size.
           Median, min and max of `repeats` calls after a warm-up call.
  quality  tests/golden/rust2_light_scene.json at 400 x 300 under RTW_INTEGRATOR_LIGHT_BIASED: the mean squared error of the 100-spp frame
           (and of a 4-spp one) against a 10 000-spp render, unfiltered, after the bilateral filter at size 10, and after the guided filter at size 10 with
           depth, normal and same_object (guides from depth_map on the same context).  8-bit frames, error in units of the full range.

    python scripts/measure_guided.py [repeats] [--no-quality]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtw_amd as R                               # noqa: E402
from tests import lights_common as LC             # noqa: E402
from tests.test_bilateral_cpu import smooth_image  # noqa: E402

W, H, SIZE = 1920, 1080, 10
SIGMA_DEPTH, SIGMA_NORMAL = 0.2, 0.3
LAYOUTS = ["by size", "table + guides in LDS", "guides in LDS, table global", "table in LDS, guides global", "table and guides global"]


def frame_guides(h, w):
    """A frame-like set of guides: depth ramps with steps, two normal planes in bands, a grid of objects with misses."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:h, 0:w]
    depth = (2.0 + 3.0 * ((x * 8) // w % 2) + 0.002 * y + rng.normal(0, 0.01, (h, w))).astype(np.float32)
    n = np.where(((x + y) % 256 < 128)[..., None], np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, 0.8])) + rng.normal(0, 0.02, (h, w, 3))
    normal = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    ids = ((x * 6) // w + 6 * ((y * 4) // h)).astype(np.int32)
    ids[rng.random((h, w)) < 0.01] = -1
    return depth, normal, ids


def timed(call, reps):
    call()
    ms = [call()[1].filter_ms for _ in range(reps)]
    return f"{np.median(ms):7.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {reps} runs)"


def timings(gpu, reps):
    img = smooth_image(H, W, 3)
    print(f"filter_ms at {W} x {H}, size {SIZE}, Square  [{os.path.basename(R.LIB_PATH)}]")
    print(f"  bilateral_filter                         {timed(lambda: gpu.bilateral_filter(img, SIZE), reps)}")
    depth, normal, ids = frame_guides(H, W)
    full = dict(depth=depth, normal=normal, ids=ids, sigma_depth=SIGMA_DEPTH, sigma_normal=SIGMA_NORMAL, same_object=True)
    ref = None
    for lay, name in enumerate(LAYOUTS):
        gpu.set_option(R.OPT_GUIDED_LAYOUT, lay)
        print(f"  guided, all three, {name:28s} {timed(lambda: gpu.guided_filter(img, SIZE, **full), reps)}")
        out = gpu.guided_filter(img, SIZE, **full)[0]
        ref = out if ref is None else ref
        assert np.array_equal(out, ref), "a layout changed the image"
    gpu.set_option(R.OPT_GUIDED_LAYOUT, 0)
    for name, kw in (("depth", dict(depth=depth, sigma_depth=SIGMA_DEPTH)), ("normal", dict(normal=normal, sigma_normal=SIGMA_NORMAL)),
                     ("same_object", dict(ids=ids, same_object=True)), ("no term", dict())):
        print(f"  guided, {name:12s} by size                {timed(lambda: gpu.guided_filter(img, SIZE, **kw), reps)}")
    print(f"  bilateral_filter (again)                 {timed(lambda: gpu.bilateral_filter(img, SIZE), reps)}")


def quality(gpu):
    ls, g = LC.golden()
    w, h = g["width"], g["height"]
    cam = LC.camera(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)

    def render(samples, seed):
        p = ls.params(w, h, R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"], seed=seed, sampler=R.SAMPLER_CENTRES, samples=samples,
                      gamma=g["gamma"], mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
        return R.quantize_u8_rust2(gpu.render(cam, p)[0])

    truth = render(10000, 2).astype(np.float64) / 255.0
    depth, ids, normals, _ = gpu.depth_map(cam, w, h, g["mint"], g["maxt"], ids=True, normals=True)

    def mse(a):
        return float(np.mean((a.astype(np.float64) / 255.0 - truth) ** 2))

    print(f"quality: rust2_light_scene {w} x {h}, LIGHT_BIASED, against 10000 spp; size {SIZE}, Square, avg_gradient computed, "
          f"sigma_depth {SIGMA_DEPTH}, sigma_normal {SIGMA_NORMAL}, same_object")
    for samples in (g["samples"], 4):                      # the issue's 100-spp frame, and a low-sample one
        noisy = render(samples, 1)
        plain, sp = gpu.bilateral_filter(noisy, SIZE)
        guided, _ = gpu.guided_filter(noisy, SIZE, depth=depth, normal=normals, ids=ids, sigma_depth=SIGMA_DEPTH, sigma_normal=SIGMA_NORMAL,
                                      same_object=True)
        print(f"  {samples:4d} spp (avg_gradient {sp.avg_gradient:.5f}): MSE unfiltered {mse(noisy):.6e}   bilateral {mse(plain):.6e}   "
              f"guided {mse(guided):.6e}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 9
    with R.Renderer(0) as gpu:
        timings(gpu, reps)
        if "--no-quality" not in sys.argv:
            quality(gpu)


if __name__ == "__main__":
    main()
