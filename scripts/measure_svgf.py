#!/usr/bin/env python3
"""The numbers of the variance estimate and the variance-steered a-trous filter for DESIGN.md 8e and profiles/svgf.log.

  timings  filter_ms (hipEvent) at 1920 x 1080 on the Book-1 final scene's own guides, median of `repeats` calls after a warm-up, under
           RTW_OPT_ATROUS_LAYOUT 1 (tile), 2 (direct) and 0 (the shipped choice): variance_estimate on a first frame (every pixel reads its
           window), on a long history (none does) and on the history a 0.5-degree camera move leaves after five static frames; svgf_filter at 1 .. 5 levels, the
           level's own time being the difference of two totals.  For scale, in the same run: atrous_filter, temporal_accumulate, surface_map.
  parent   (--parent-tree PATH) atrous_filter's filter_ms at 3 levels and bench.py --gpus 1 through a built checkout of the parent commit
           at PATH and through this tree, alternating, a child process each: nothing existing moved.
  quality  (--quality) DESIGN.md 8d's sequences -- small_view(SCENE_C2, 400, 225), 4 spp, SAMPLER_ROW, gamma 1, a 0.25-degree orbit and a
           static camera, 16 frames, MSE against 4096 spp; the light scene likewise -- accumulated with TEMPORAL_DEFAULTS, with a fifth
           column beside 8d's four: accumulated + variance-steered a-trous.  The sweep sigma_luminance {1, 2, 4, 8} x levels {3, 4, 5} x
           min_history {1, 4} x prefilter {0, 1} at sigma_color 0 on the Book-1 orbit; the best row by the mean of frames 8 .. 15; that row
           and the library's SVGF_DEFAULTS on every sequence; and, over 8 seeds, the ratio on frames 8 .. 11 of the new chain's MSE to that of
           TemporalDenoiser's chain (the fixed a-trous filter over the same accumulated frames).

    python scripts/measure_svgf.py [repeats] [--quality] [--parent-tree PATH] [--out profiles/svgf.log]
"""
import itertools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R                                    # noqa: E402
from tests.temporal_common import orbit                # noqa: E402

W, H = 1920, 1080
MINT, MAXT = 0.001, 1000.0
OFFSET = (0.5, 0.5)
LINES = []
# what a child process of the parent A/B runs in either tree: only calls both trees have
ATROUS_CHILD = """
import numpy as np, rtw_amd as R
W, H = 1920, 1080
look = tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]))
cam = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=look, vup=(0.0, 1.0, 0.0)).camera()
with R.Renderer(0) as gpu:
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    g = gpu.surface_map(cam, W, H, 0.001, 1000.0, R.INTEGRATOR_GRADIENT, R.RAYS_PIXEL, (0.5, 0.5))
    f = (np.random.default_rng(9).random((H, W, 3)) * 2.0).astype(np.float32)
    call = lambda: gpu.atrous_filter(f, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"], levels=3)[1].filter_ms
    call()
    ms = [call() for _ in range(15)]
    print(f"atrous_filter 3 levels at {W} x {H}: median of 15 {np.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})")
"""


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def median_of(call, reps):
    call()
    ms = [call() for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms)


def fmt(t):
    return f"{t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def timings(gpu, reps):
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    look = tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]))
    cam0 = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=look, vup=(0.0, 1.0, 0.0)).camera()
    cam1 = orbit(cam0, 0.5)
    g0, g1 = (gpu.surface_map(c, W, H, MINT, MAXT, R.INTEGRATOR_GRADIENT, R.RAYS_PIXEL, OFFSET) for c in (cam0, cam1))
    rng = np.random.default_rng(9)
    f0, f1 = ((rng.random((H, W, 3)) * 2.0).astype(np.float32) for _ in range(2))
    guides = lambda g: dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
    first = gpu.temporal_accumulate(f0, cam0, **guides(g0), offset=OFFSET)[0]
    still = first
    for _ in range(4):                                  # four more frames under the static camera, then the move: lengths of 6, and of 1 where
        still = gpu.temporal_accumulate(f1, cam0, **guides(g0), history=still, offset=OFFSET)[0]       # the move uncovered or rejected
    moved = gpu.temporal_accumulate(f1, cam1, **guides(g1), history=still, offset=OFFSET)[0]
    long_len = np.full((H, W), 9.0, np.float32)
    names = {1: "tile", 2: "direct", 0: "shipped"}

    log(f"# variance_estimate filter_ms at {W} x {H}, Book-1 final scene's guides, every guide on, min_history 4: median of {reps} after a warm-up (min .. max)")
    for radius in (1, 3):
        for hname, mom, length, g in (("first frame (every pixel reads its window)", first["moments"], first["len"], g0),
                                      ("long history (no pixel does)", first["moments"], long_len, g0),
                                      (f"after a 0.5-degree move ({float((moved['len'] < 4).mean()):.3f} of the pixels do)", moved["moments"], moved["len"], g1)):
            row = []
            for lay in (1, 2, 0):
                gpu.set_option(R.OPT_ATROUS_LAYOUT, lay)
                row.append(f"{names[lay]} " + fmt(median_of(lambda: gpu.variance_estimate(mom, length, **guides(g), min_history=4, radius=radius)[1].filter_ms, reps)))
            log(f"  radius {radius}, {hname}:".ljust(72) + "   ".join(row))
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)

    variance = gpu.variance_estimate(moved["moments"], moved["len"], **guides(g1), min_history=4, radius=3)[0]
    kw = dict(guides(g1), albedo=g1["albedo"], emitted=g1["emitted"])
    log(f"# svgf_filter filter_ms at {W} x {H} (demodulation + levels), every guide, albedo, emission, sigma_luminance 4, prefilter 1, sigma_color 0:")
    log(f"# median of {reps} (min .. max); a level's own time is the difference of two medians")
    totals = {}
    for lay in (1, 2, 0):
        gpu.set_option(R.OPT_ATROUS_LAYOUT, lay)
        for levels in (1, 2, 3, 4, 5):
            t = median_of(lambda: gpu.svgf_filter(moved["color"], variance, levels=levels, sigma_luminance=4.0, **kw)[2].filter_ms, reps)
            totals[lay, levels] = t[0]
            own = t[0] - totals.get((lay, levels - 1), 0.0)
            log(f"  {names[lay]:8s} {levels} levels: total {fmt(t)}   level {levels - 1}{' + demodulation' if levels == 1 else ''}: {own:6.3f} ms")
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)
    t = median_of(lambda: gpu.svgf_filter(moved["color"], variance, levels=3, sigma_luminance=4.0, prefilter=False, **kw)[2].filter_ms, reps)
    log(f"  shipped  3 levels, prefilter 0: total {fmt(t)}")
    t = median_of(lambda: gpu.svgf_filter(moved["color"], variance, levels=3, sigma_luminance=0.0, **kw)[2].filter_ms, reps)
    log(f"  shipped  3 levels, sigma_luminance 0 (the a-trous filter's bytes): total {fmt(t)}")
    log("# for scale, in the same run:")
    for levels in (3, 5):
        t = median_of(lambda: gpu.atrous_filter(moved["color"], levels=levels, **kw)[1].filter_ms, reps)
        log(f"  atrous_filter {levels} levels (its defaults)".ljust(52) + fmt(t))
    t = median_of(lambda: gpu.temporal_accumulate(f0, cam1, **guides(g1), history=first, offset=OFFSET)[2].filter_ms, reps)
    log("  temporal_accumulate after a 0.5-degree move".ljust(52) + fmt(t))
    t = median_of(lambda: gpu.surface_map(cam0, W, H, MINT, MAXT, R.INTEGRATOR_GRADIENT)["stats"].kernel_ms, reps)
    log("  surface_map (all six buffers)".ljust(52) + fmt(t))


def parent_ab(parent_tree, rounds=2):
    log("# atrous_filter and bench.py --gpus 1 through the parent commit's package and library and through this tree's, alternating, a child process each")
    env = dict(os.environ)
    env.pop("RTW_HIP_LIB", None)
    for rnd in range(1, rounds + 1):
        for name, tree in (("parent", os.path.abspath(parent_tree)), ("this", ROOT)):
            for what, cmd in (("atrous", [sys.executable, "-c", ATROUS_CHILD]),
                              ("bench", [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"])):
                out = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=400)
                tail = [ln for ln in out.stdout.splitlines() if ln.strip()][-1:] if out.returncode == 0 else [out.stderr[-1500:]]
                if what == "bench" and out.returncode == 0:
                    j = json.loads(tail[0])
                    tail = [f"{j['value']:.1f} {j['unit']}, {j['ms_per_step']:.3f} ms per step (--steps {j['steps']} --warmup {j['warmup']})"]
                log(f"  {what} {name} {rnd}: " + (tail[0] if tail else "") + ("" if out.returncode == 0 else f"  (exit status {out.returncode})"))
                if out.returncode != 0:
                    return


def accumulate(gpu, frames, gs, cams):
    """The histories of a sequence under TEMPORAL_DEFAULTS (copies: each call's outputs are new arrays)."""
    hist, out = None, []
    for cur, g, cam in zip(frames, gs, cams):
        hist, _, _ = gpu.temporal_accumulate(cur, cam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist, offset=OFFSET)
        out.append(hist)
    return out


def steered(gpu, hist, g, prm):
    """The filter stage of SvgfDenoiser.step on one accumulated frame."""
    kw = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
    var = gpu.variance_estimate(hist["moments"], hist["len"], min_history=prm["min_history"], radius=prm.get("radius", R.SVGF_DEFAULTS["radius"]), **kw)[0]
    return gpu.svgf_filter(hist["color"], var, albedo=g["albedo"], emitted=g["emitted"], levels=prm["levels"], sigma_color=prm.get("sigma_color", 0.0),
                           sigma_luminance=prm["sigma_luminance"], prefilter=prm["prefilter"], **kw)[0]


def mse(img, t):
    return float(((img.astype(np.float64) - t) ** 2).mean())


def columns(gpu, frames, gs, hists, truths, prm):
    """Per frame the MSE of (single, a-trous alone, accumulated, accumulated + a-trous, accumulated + variance-steered a-trous)."""
    rows = []
    for cur, g, hist, t in zip(frames, gs, hists, truths):
        kw = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"])
        rows.append((mse(cur, t), mse(gpu.atrous_filter(cur, **kw)[0], t), mse(hist["color"], t), mse(gpu.atrous_filter(hist["color"], **kw)[0], t),
                     mse(steered(gpu, hist, g, prm), t)))
    return rows


def report(label, rows):
    names = ("single", "a-trous", "accumulated", "accumulated + a-trous", "accumulated + steered")
    for k, r in enumerate(rows):
        log(f"  {label} frame {k:2d}: " + "  ".join(f"{n} {v:.6f} ({v / r[0]:.3f})" for n, v in zip(names, r)))
    for lo, hi in ((0, 3), (len(rows) // 2, len(rows))):
        m = np.array(rows[lo:hi]).mean(axis=0)
        log(f"  {label} mean of frames {lo} .. {hi - 1}: " + "  ".join(f"{n} {v:.6f} ({v / m[0]:.3f})" for n, v in zip(names, m)))


def quality(gpu):
    from tests import lights_common as LC
    from tests.test_oracle_golden import small_view
    w, h, n_frames, step = 400, 225, 16, 0.25
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)

    def render(c, samples, seed):
        p.samples, p.seed = samples, seed
        return gpu.render(c, p)[0]

    guides = lambda c: gpu.surface_map(c, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, OFFSET)
    log(f"# quality: Book-1 final scene {w} x {h}, SAMPLER_ROW, gamma 1, 4 spp per frame; MSE against a 4096-spp render of each view (ratio to the single frame)")
    log(f"#   accumulation at TEMPORAL_DEFAULTS {R.TEMPORAL_DEFAULTS}; a-trous at ATROUS_DEFAULTS {R.ATROUS_DEFAULTS}; both filters with albedo and emission")
    book = {}
    for label, deg in (("book1 orbit", step), ("book1 static", 0.0)):
        cams = [orbit(cam, deg * k) for k in range(n_frames)]
        truths = [render(c, 4096, 1).astype(np.float64) for c in (cams if deg else cams[:1])] * (1 if deg else n_frames)
        frames = [render(c, 4, 100 + k) for k, c in enumerate(cams)]
        gs = [guides(c) for c in cams]
        book[label] = (frames, gs, accumulate(gpu, frames, gs, cams), truths, cams)

    frames, gs, hists, truths, cams = book["book1 orbit"]
    half = n_frames // 2
    single = np.mean([mse(f, t) for f, t in zip(frames[half:], truths[half:])])
    log(f"# sweep on the Book-1 orbit, sigma_color 0, radius {R.SVGF_DEFAULTS['radius']}, epsilon {R.SVGF_DEFAULTS['epsilon']}: mean MSE of frames {half} .. {n_frames - 1} and of frames 0 .. 2")
    log(f"#   (ratio to the single frames' mean {single:.6f})")
    best = None
    for sl, levels, mh, pre in itertools.product((1.0, 2.0, 4.0, 8.0), (3, 4, 5), (1, 4), (0, 1)):
        prm = dict(sigma_luminance=sl, levels=levels, min_history=mh, prefilter=bool(pre))
        e = [mse(steered(gpu, hist, g, prm), t) for hist, g, t in zip(hists, gs, truths)]
        tail, head = float(np.mean(e[half:])), float(np.mean(e[:3]))
        head1 = float(np.mean([mse(f, t) for f, t in zip(frames[:3], truths[:3])]))
        log(f"  sigma_luminance {sl:3.0f} levels {levels} min_history {mh} prefilter {pre}   frames {half}..{n_frames - 1} {tail:.6f} ({tail / single:.3f})   frames 0..2 {head:.6f} ({head / head1:.3f})")
        if best is None or tail < best[0]:
            best = (tail, prm)
    log(f"# best row by the mean of frames {half} .. {n_frames - 1}: {best[1]}, MSE {best[0]:.6f} ({best[0] / single:.3f})")
    lib = {k: R.SVGF_DEFAULTS[k] for k in ("sigma_luminance", "levels", "min_history", "prefilter", "sigma_color", "radius")}
    log(f"# the library's SVGF_DEFAULTS {R.SVGF_DEFAULTS}")
    for label in book:
        f_, g_, h_, t_, _ = book[label]
        report(label + ", best row", columns(gpu, f_, g_, h_, t_, best[1]))
        if any(lib[k] != best[1][k] for k in best[1]):
            report(label + ", SVGF_DEFAULTS", columns(gpu, f_, g_, h_, t_, lib))

    log("# the quality assertion's figure: on the orbit's frames 8 .. 11, MSE of accumulated + steered (the best row) over MSE of accumulated + a-trous")
    log("#   (TemporalDenoiser's chain), the sequence rendered with 8 other sets of seeds")
    ratios = []
    for s in range(8):
        fr = [render(c, 4, 1000 * (s + 1) + k) for k, c in enumerate(cams[:12])]
        hs = accumulate(gpu, fr, gs[:12], cams[:12])
        new = old = 0.0
        for k in range(8, 12):
            g = gs[k]
            kw = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"])
            new += mse(steered(gpu, hs[k], g, best[1]), truths[k])
            old += mse(gpu.atrous_filter(hs[k]["color"], **kw)[0], truths[k])
        ratios.append(new / old)
        log(f"  seeds {1000 * (s + 1)}..: steered {new / 4:.6f}  fixed {old / 4:.6f}  ratio {new / old:.4f}")
    log(f"# ratio: worst {max(ratios):.4f}, best {min(ratios):.4f}, spread {max(ratios) - min(ratios):.4f}; asserted below 1 only if worst < 1 - 2 * spread = {1 - 2 * (max(ratios) - min(ratios)):.4f}")

    # the light scene under LIGHT_BIASED, through a Viewport camera at the golden camera's place
    ls, g = LC.golden()
    w, h = 400, 300
    lcam = LC.camera_no_rand(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    integ, depth = R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"]

    def lrender(c, samples, seed):
        lp = ls.params(w, h, integ, depth, seed=seed, sampler=R.SAMPLER_ROW, samples=samples, gamma=1.0, mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
        return gpu.render(c, lp)[0]

    lguides = lambda c: gpu.surface_map(c, w, h, g["mint"], g["maxt"], integ, R.RAYS_PIXEL, OFFSET)
    log(f"# quality: rust2_light_scene {w} x {h}, LIGHT_BIASED, SAMPLER_ROW, gamma 1, 4 spp per frame, a Viewport camera; MSE against 4096 spp")
    try:
        for label, deg in (("lights orbit", step), ("lights static", 0.0)):
            cams = [orbit(lcam, deg * k) for k in range(n_frames)]
            truths = [lrender(c, 4096, 2).astype(np.float64) for c in (cams if deg else cams[:1])] * (1 if deg else n_frames)
            frames = [lrender(c, 4, 100 + k) for k, c in enumerate(cams)]
            gs = [lguides(c) for c in cams]
            report(label + ", best row", columns(gpu, frames, gs, accumulate(gpu, frames, gs, cams), truths, best[1]))
    except R.RtwError as e:
        log(f"  unmeasured: {e}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0])) if args and args[0].isdigit() else 9
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    try:
        if "--parent-tree" in sys.argv:
            parent_ab(sys.argv[sys.argv.index("--parent-tree") + 1])
        with R.Renderer(0) as gpu:
            if "--no-timings" not in sys.argv:
                timings(gpu, reps)
            if "--quality" in sys.argv:
                quality(gpu)
    finally:
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
