#!/usr/bin/env python3
"""The a-trous filter's numbers for DESIGN.md 8c and profiles/atrous.log.

  timings  filter_ms (all launches of a call, hipEvent) at 1920 x 1080 with every term on, albedo and emission, for levels = 1 .. 6 under
           RTW_OPT_ATROUS_LAYOUT 1 (an LDS tile wherever it fits) and 2 (global memory), median of `repeats` calls after a warm-up call.
           The time of level i under a layout is the difference between the calls with i + 1 and with i levels (the call with one level
           also holds the demodulation launch, the same under both layouts).  Then the 5-level filter under layout 0, and for scale, in the
           same run: guided_filter at size 10 with all guides and depth_map with ids and normals of the Book-1 final scene.
  quality  (--quality) the mean squared error against a 4096-spp render of the same view, gamma 1, of a 4-spp and a 16-spp frame:
           unfiltered, after guided_filter at size 10, and after the a-trous filter without and with albedo and emission over a sweep of
           levels and sigmas; guides from surface_map at the pixel centres.  Then the seed-to-seed spread of the best row's 4-spp ratio
           over 8 seeds, the Python defaults, render_denoised, and the light scene under RUST2 and LIGHT_BIASED with the best row
           (--sweep-lights: the whole sweep there too).

    python scripts/measure_atrous.py [repeats] [--quality [--sweep-lights]] [--out profiles/atrous.log]
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtw_amd as R                                    # noqa: E402
from scripts.measure_guided import frame_guides        # noqa: E402
from tests.test_bilateral_cpu import smooth_image      # noqa: E402

W, H = 1920, 1080
MINT, MAXT = 0.001, 1000.0
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def median_ms(call, reps):
    call()
    ms = [call()[1].filter_ms for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms)


def timings(gpu, reps):
    rng = np.random.default_rng(9)
    depth, normal, ids = frame_guides(H, W)
    albedo = (0.2 + 0.7 * rng.random((H, W, 3))).astype(np.float32)
    emitted = np.where((ids == 3)[..., None], np.float32(1.5), np.float32(0.0)).astype(np.float32) * np.ones(3, np.float32)
    frame = (albedo * (0.5 + 0.5 * rng.random((H, W, 3))) + emitted).astype(np.float32)
    kw = dict(depth=depth, normal=normal, ids=ids, albedo=albedo, emitted=emitted, sigma_color=0.5, sigma_depth=0.5, sigma_normal=0.3,
              same_object=True, albedo_floor=0.01)
    log(f"# a-trous filter_ms at {W} x {H}, every term on, albedo + emission: median of {reps} after a warm-up (min .. max)")
    total = {1: [], 2: []}
    ref = {}
    for levels in range(1, 7):
        for lay in (1, 2):
            gpu.set_option(R.OPT_ATROUS_LAYOUT, lay)
            med, lo, hi = median_ms(lambda: gpu.atrous_filter(frame, levels=levels, **kw), reps)
            total[lay].append(med)
            out = gpu.atrous_filter(frame, levels=levels, **kw)[0]
            assert np.array_equal(ref.setdefault(levels, out).view(np.uint32), out.view(np.uint32)), "a layout changed the image"
            log(f"  levels {levels}  layout {lay} ({'LDS tile where it fits' if lay == 1 else 'global memory'})".ljust(52) + f"{med:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    log("# per level: the difference of consecutive rows above (level 0: the whole one-level call, demodulation launch included)")
    for i in range(6):
        t = total[1][i] - (total[1][i - 1] if i else 0.0)
        d = total[2][i] - (total[2][i - 1] if i else 0.0)
        log(f"  level {i} (step {1 << i:2d})   tile {t:7.3f} ms   global {d:7.3f} ms")
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)
    med, lo, hi = median_ms(lambda: gpu.atrous_filter(frame, levels=5, **kw), reps)
    log(f"  the 5-level filter, layout 0 (the choice kept)".ljust(52) + f"{med:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    med, lo, hi = median_ms(lambda: gpu.atrous_filter(frame, levels=5, sigma_color=0.5), reps)
    log(f"  the 5-level filter, colour term only, layout 0".ljust(52) + f"{med:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    img = smooth_image(H, W, 3)
    med, lo, hi = median_ms(lambda: gpu.guided_filter(img, 10, depth=depth, normal=normal, ids=ids, sigma_depth=0.2, sigma_normal=0.3, same_object=True), reps)
    log(f"  for scale: guided_filter, size 10, all guides".ljust(52) + f"{med:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    cam2 = R.camera2_new(W / H, (13.0, 2.0, 3.0), (0.0, 1.0, 0.0), tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0])), 20.0, 0.0)
    run = lambda: gpu.depth_map(cam2, W, H, MINT, MAXT, ids=True, normals=True)[-1].kernel_ms
    run()
    ms = [run() for _ in range(reps)]
    log(f"  for scale: depth_map + ids + normals, Book-1 scene".ljust(52) + f"{np.median(ms):7.3f} ms ({min(ms):.3f} .. {max(ms):.3f})")
    vp = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0])), vup=(0.0, 1.0, 0.0))
    run = lambda: gpu.surface_map(vp.camera(), W, H, MINT, MAXT, R.INTEGRATOR_GRADIENT)["stats"].kernel_ms
    run()
    ms = [run() for _ in range(reps)]
    log(f"  surface_map (all six buffers), Book-1 scene".ljust(52) + f"{np.median(ms):7.3f} ms ({min(ms):.3f} .. {max(ms):.3f})")


def sweep(gpu, frames, truth, guides, label):
    """The table of one scene: per frame the unfiltered error, guided_filter at size 10, and the a-trous sweep without and with albedo and
    emission.  Returns the best 4-spp row with albedo: (mse, levels, sigma_color, sigma_depth, sigma_normal)."""
    mse = lambda img: float(((img.astype(np.float64) - truth) ** 2).mean())
    g = dict(depth=guides["depth"], normal=guides["normal"], ids=guides["idx"])
    best = None
    for spp, frame in frames:
        base = mse(frame)
        log(f"  {label} {spp:2d} spp unfiltered                                            MSE {base:.6f}")
        g8 = gpu.guided_filter(frame, 10, sigma_depth=0.2, sigma_normal=0.3, same_object=True, **g)[0]
        log(f"  {label} {spp:2d} spp guided_filter size 10 (8-bit frame)                   MSE {mse(g8.astype(np.float64) / 255.0):.6f}  ratio {mse(g8.astype(np.float64) / 255.0) / base:.3f}")
        for levels, sc, sd, sn in itertools.product((3, 4, 5, 6), (0.25, 1.0, 4.0), (0.25, 1.0, 4.0), (0.1, 0.3, 1.0)):
            kw = dict(levels=levels, sigma_color=sc, sigma_depth=sd, sigma_normal=sn, **g)
            plain = mse(gpu.atrous_filter(frame, **kw)[0])
            full = mse(gpu.atrous_filter(frame, albedo=guides["albedo"], emitted=guides["emitted"], **kw)[0])
            log(f"  {label} {spp:2d} spp a-trous levels {levels} color {sc:4.2f} depth {sd:4.2f} normal {sn:4.2f}   no albedo MSE {plain:.6f} ratio {plain / base:.3f}"
                f"   albedo + emission MSE {full:.6f} ratio {full / base:.3f}")
            if spp == 4 and (best is None or full < best[0]):
                best = (full, levels, sc, sd, sn)
    return best


def quality(gpu):
    from tests import lights_common as LC
    from tests.test_oracle_golden import small_view
    w, h = 400, 225
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)

    def render(samples, seed):
        p.samples, p.seed = samples, seed
        return gpu.render(cam, p)[0]

    truth = render(4096, 1).astype(np.float64)
    guides = gpu.surface_map(cam, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, (0.5, 0.5))
    mse = lambda img: float(((img.astype(np.float64) - truth) ** 2).mean())
    log(f"# quality: Book-1 final scene {w} x {h}, SAMPLER_ROW, gamma 1; MSE against a 4096-spp render (linear, full range 1)")
    log(f"#   guides: surface_map at the pixel centres ({int((guides['idx'] < 0).sum())} misses)")
    best = sweep(gpu, [(4, render(4, 7)), (16, render(16, 7))], truth, guides, "book1")
    _, levels, sc, sd, sn = best
    log(f"# best 4-spp row with albedo: levels {levels} color {sc} depth {sd} normal {sn}; the same parameters over 8 seeds:")
    kw = dict(depth=guides["depth"], normal=guides["normal"], ids=guides["idx"], albedo=guides["albedo"], emitted=guides["emitted"])
    ratios = []
    for seed in range(11, 19):
        frame = render(4, seed)
        out = gpu.atrous_filter(frame, levels=levels, sigma_color=sc, sigma_depth=sd, sigma_normal=sn, **kw)[0]
        ratios.append(mse(out) / mse(frame))
        log(f"  seed {seed}: unfiltered {mse(frame):.6f}  filtered {mse(out):.6f}  ratio {ratios[-1]:.3f}")
    log(f"  ratio over 8 seeds: min {min(ratios):.3f} max {max(ratios):.3f} mean {np.mean(ratios):.3f}")
    frame = render(4, 7)
    log(f"# Python defaults {R.ATROUS_DEFAULTS}: ratio {mse(gpu.atrous_filter(frame, **kw)[0]) / mse(frame):.3f}")
    p.gamma = 2.0
    den = gpu.render_denoised(cam, p)[0]
    log(f"# render_denoised at gamma 2, 4 spp: MSE against the 4096-spp frame ** 0.5 {float(((den.astype(np.float64) - np.sqrt(truth)) ** 2).mean()):.6f}"
        f" (unfiltered {float(((np.sqrt(frame.astype(np.float64)) - np.sqrt(truth)) ** 2).mean()):.6f})")

    # the light scene: nothing is asserted on it (its unbiased frames are dominated by fireflies); the best Book-1 row and the defaults only
    ls, g = LC.golden()
    w, h = 400, 300
    lcam = LC.camera(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    for name, integ, depth in (("RUST2", R.INTEGRATOR_RUST2, g.get("depth", 8)), ("LIGHT_BIASED", R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"])):
        def lrender(samples, seed):
            lp = ls.params(w, h, integ, depth, seed=seed, sampler=R.SAMPLER_CENTRES, samples=samples, gamma=1.0, mint=g["mint"], maxt=g["maxt"],
                           accel=R.ACCEL_BVH)
            return gpu.render(lcam, lp)[0]
        ltruth = lrender(4096, 2).astype(np.float64)
        lg = gpu.surface_map(lcam, w, h, g["mint"], g["maxt"], integ, R.RAYS_DEPTH_MAP)
        lmse = lambda img: float(((img.astype(np.float64) - ltruth) ** 2).mean())
        log(f"# quality: rust2_light_scene {w} x {h}, {name}, SAMPLER_CENTRES, gamma 1; MSE against 4096 spp; guides: surface_map, RTW_RAYS_DEPTH_MAP")
        lkw = dict(depth=lg["depth"], normal=lg["normal"], ids=lg["idx"])
        if "--sweep-lights" in sys.argv:
            lbest = sweep(gpu, [(4, lrender(4, 1)), (16, lrender(16, 1))], ltruth, lg, name)
            log(f"# {name}: best 4-spp row with albedo: levels {lbest[1]} color {lbest[2]} depth {lbest[3]} normal {lbest[4]}, MSE {lbest[0]:.6f}")
        for spp in (4, 16):
            frame = lrender(spp, 1)
            g8 = gpu.guided_filter(frame, 10, sigma_depth=0.2, sigma_normal=0.3, same_object=True, **lkw)[0]
            a0 = gpu.atrous_filter(frame, levels=levels, sigma_color=sc, sigma_depth=sd, sigma_normal=sn, **lkw)[0]
            a1 = gpu.atrous_filter(frame, levels=levels, sigma_color=sc, sigma_depth=sd, sigma_normal=sn, albedo=lg["albedo"], emitted=lg["emitted"], **lkw)[0]
            log(f"  {name} {spp:2d} spp: unfiltered {lmse(frame):.6f}  guided size 10 {lmse(g8.astype(np.float64) / 255.0):.6f}  a-trous (best Book-1 row) no albedo "
                f"{lmse(a0):.6f}  albedo + emission {lmse(a1):.6f}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0])) if args and args[0].isdigit() else 9
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    with R.Renderer(0) as gpu:
        timings(gpu, reps)
        if "--quality" in sys.argv:
            quality(gpu)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
