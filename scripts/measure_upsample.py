#!/usr/bin/env python3
"""The guide-steered upsampling's numbers for DESIGN.md 8i and profiles/upsample.log.  Needs the GPU.

  timings  filter_ms (hipEvent) of upsample_filter at an output of 1920 x 1080 for scales 2, 3, 4 and radius 1, 2 with every term on, albedo
           and emission, under RTW_OPT_ATROUS_LAYOUT 1 (the LDS tile) and 2 (direct), alternated in one process, median and range of
           `repeats` calls after a warm-up; the bytes the pass must move, from the shapes, over the peak HBM rate as a share of the
           measured time, and the taps a nanosecond; the pass with every term off; and for comparison in the same run one a-trous level
           and surface_map with six buffers.  Every buffer is a device tensor, so no staging enters.
  quality  (--quality) MSE against a 4096-spp render at the output size, gamma 1, as a share of the single 4-spp full-size frame's MSE, 8
           seeds, of the 4-spp Book-1 view of profiles/atrous.log at 400 x 225 and 1920 x 1080: full size 4 spp with atrous_filter; half
           size 16 spp and quarter size 64 spp, each upsampled, a-trous filtered at the low size then upsampled, and both again with every
           term and the albedo off (plain bilinear); render and filter times of every column; a sweep of radius, sigma_depth, sigma_normal
           and same_object at 400 x 225; the fallback share of pixels from wsum; the light scene's light-biased frames; and the Book-1
           orbit of profiles/temporal.log through SvgfDenoiser(scale=2) at 16 spp against scale=1 at 4 spp.

    python scripts/measure_upsample.py [repeats] [--quality] [--out profiles/upsample.log]
"""
import itertools
import os
import sys

import numpy as np

import torch                                           # before the first rtw call: the library then shares the HIP runtime torch loaded (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtw_amd as R                                    # noqa: E402
from tests.temporal_common import orbit                # noqa: E402

W, H = 1920, 1080
HBM_GBS = 8000.0                                       # MI355X peak HBM3E bandwidth, GB/s
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def save(out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


def median_ms(call, reps):
    call()
    ms = [call() for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms)


def book1(gpu, w, h):
    from tests.test_oracle_golden import small_view
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    return cam, p


def surf(gpu, cam, p):
    return gpu.surface_map(cam, p.width, p.height, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, (0.5, 0.5), accel=p.accel)


def low_view(cam, p, s):
    lp = R.RtwParams.from_buffer_copy(p)
    lp.width, lp.height = -(-p.width // s), -(-p.height // s)
    return R.camera_scaled(cam, s), lp


def timings(gpu, reps):
    dev = torch.device("cuda:0")
    T = lambda g: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in g.items() if k in ("depth", "normal", "idx", "albedo", "emitted")}
    cam, p = book1(gpu, W, H)
    hi = surf(gpu, cam, p)
    t_hi = T(hi)
    n_hi = W * H
    rng = np.random.default_rng(3)
    log(f"# upsample_filter filter_ms at an output of {W} x {H}, Book-1 guides, device tensors: median of {reps} after a warm-up (min .. max)")
    log(f"#   floor = the bytes the pass must move (12 of the frame and up to 44 of guides a low pixel, up to 44 of guides and 12 of out an output pixel) at {HBM_GBS:.0f} GB/s")
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    ahead = {1: 0, 2: 0}
    for s in (2, 3, 4):
        lcam, lp = low_view(cam, p, s)
        lo = surf(gpu, lcam, lp)
        t_lo = T(lo)
        n_lo = lp.width * lp.height
        fr = torch.from_numpy(((0.5 + 0.5 * rng.random((lp.height, lp.width, 3))).astype(np.float32) * np.maximum(lo["albedo"], np.float32(0.05)) + lo["emitted"])).to(dev)
        for radius, on in itertools.product((1, 2), (True, False)):
            kw = dict(scale=s, radius=radius, sigma_depth=0.25 if on else 0.0, sigma_normal=0.3 if on else 0.0, same_object=on, albedo_floor=1e-3)
            a_lo, a_hi = (t_lo, t_hi) if on else ({}, {})
            taps = gpu.upsample_filter(fr, (W, H), lo=a_lo, hi=a_hi, out=out, **kw)[2].taps
            floor_ms = ((12 + (44 if on else 0)) * n_lo + ((44 if on else 0) + 12) * n_hi) / (HBM_GBS * 1e9) * 1e3
            row, ref = {}, None
            for _ in range(2):                                                    # tile, direct, tile, direct: alternated
                for lay in (1, 2):
                    gpu.set_option(R.OPT_ATROUS_LAYOUT, lay)
                    row.setdefault(lay, []).append(median_ms(lambda: gpu.upsample_filter(fr, (W, H), lo=a_lo, hi=a_hi, out=out, **kw)[2].filter_ms, reps))
                    got = out.cpu().numpy()
                    ref = got if ref is None else ref
                    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)), "a layout changed the image"
            med = {lay: min(m[0] for m in row[lay]) for lay in row}
            rng_ = {lay: (min(m[1] for m in row[lay]), max(m[2] for m in row[lay])) for lay in row}
            best = min(med, key=med.get)
            if on:
                ahead[best] += 1
            log(f"  scale {s} radius {radius} {'every term on, albedo + emission' if on else 'every term off, no albedo        '}"
                f"   tile {med[1]:6.3f} ms ({rng_[1][0]:.3f} .. {rng_[1][1]:.3f})   direct {med[2]:6.3f} ms ({rng_[2][0]:.3f} .. {rng_[2][1]:.3f})"
                f"   floor {floor_ms:.3f} ms = {100 * floor_ms / med[best]:4.1f} % of the faster   {taps / med[best] * 1e-6:7.1f} taps/ns")
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)
    log(f"# the tile is ahead in {ahead[1]} of {ahead[1] + ahead[2]} rows with the terms on, direct in {ahead[2]}")
    fr = torch.from_numpy((0.5 + 0.5 * rng.random((H, W, 3))).astype(np.float32)).to(dev)
    g = dict(depth=t_hi["depth"], normal=t_hi["normal"], ids=t_hi["idx"], albedo=t_hi["albedo"], emitted=t_hi["emitted"])
    med, lo_, hi_ = median_ms(lambda: gpu.atrous_filter(fr, levels=1, out=out, **g)[1].filter_ms, reps)
    med2, _, _ = median_ms(lambda: gpu.atrous_filter(fr, levels=2, out=out, **g)[1].filter_ms, reps)
    log(f"  for scale: atrous_filter, 1 level (with the demodulation launch)   {med:6.3f} ms ({lo_:.3f} .. {hi_:.3f});  2 levels {med2:6.3f} ms: one more level {med2 - med:6.3f} ms")
    med, lo_, hi_ = median_ms(lambda: surf(gpu, cam, p)["stats"].kernel_ms, reps)
    log(f"  for scale: surface_map (all six buffers), Book-1 scene           {med:6.3f} ms ({lo_:.3f} .. {hi_:.3f})")
    lcam, lp = low_view(cam, p, 2)
    med, lo_, hi_ = median_ms(lambda: surf(gpu, lcam, lp)["stats"].kernel_ms, reps)
    log(f"  for scale: surface_map at the half size {lp.width} x {lp.height}                {med:6.3f} ms ({lo_:.3f} .. {hi_:.3f})")


BILINEAR = dict(radius=1, sigma_depth=0.0, sigma_normal=0.0, same_object=False)


def columns(gpu, cam, p, seeds, truth, ukw, render, label):
    """The table of one view: per column the mean over `seeds` of MSE / MSE(single 4-spp full-size frame), and of the times."""
    w, h = p.width, p.height
    mse = lambda img: float(((img.astype(np.float64) - truth) ** 2).mean())
    hi = surf(gpu, cam, p)
    rows = {}

    def add(name, ratio, ms):
        rows.setdefault(name, []).append((ratio, ms))

    fallback = {}
    for seed in seeds:
        full, st = render(cam, p, 4, seed)
        base = mse(full)
        add("full size  4 spp, single frame", 1.0, st.kernel_ms)
        out, sa = gpu.atrous_filter(full, depth=hi["depth"], normal=hi["normal"], ids=hi["idx"], albedo=hi["albedo"], emitted=hi["emitted"])
        add("full size  4 spp + atrous_filter (the present chain)", mse(out) / base, st.kernel_ms + hi["stats"].kernel_ms + sa.filter_ms)
        for s, spp in ((2, 16), (4, 64)):
            lcam, lp = low_view(cam, p, s)
            lo = surf(gpu, lcam, lp)
            fr, st = render(lcam, lp, spp, seed)
            t_guides = lo["stats"].kernel_ms + hi["stats"].kernel_ms
            size = "half   " if s == 2 else "quarter"
            up, ws, su = gpu.upsample_filter(fr, (w, h), lo=lo, hi=hi, scale=s, out_wsum=True, **ukw)
            add(f"{size} size {spp:2d} spp + upsample", mse(up) / base, st.kernel_ms + t_guides + su.filter_ms)
            fallback.setdefault(s, []).append(float((ws == 0).mean()))
            fa, sa = gpu.atrous_filter(fr, depth=lo["depth"], normal=lo["normal"], ids=lo["idx"], albedo=lo["albedo"], emitted=lo["emitted"])
            up, _, su = gpu.upsample_filter(fa, (w, h), lo=lo, hi=hi, scale=s, **ukw)
            add(f"{size} size {spp:2d} spp + a-trous at the low size + upsample", mse(up) / base, st.kernel_ms + t_guides + sa.filter_ms + su.filter_ms)
            up, _, su = gpu.upsample_filter(fr, (w, h), scale=s, **BILINEAR)
            add(f"{size} size {spp:2d} spp + plain bilinear (no term, no albedo)", mse(up) / base, st.kernel_ms + su.filter_ms)
            up, _, su = gpu.upsample_filter(fa, (w, h), scale=s, **BILINEAR)
            add(f"{size} size {spp:2d} spp + a-trous at the low size + plain bilinear", mse(up) / base, st.kernel_ms + lo["stats"].kernel_ms + sa.filter_ms + su.filter_ms)
    log(f"# {label}: mean over seeds {list(seeds)} of MSE / MSE(single 4-spp frame) (min .. max), and the column's device time (render + guides + filters)")
    for name, v in rows.items():
        r, ms = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        log(f"  {name:70s} ratio {r.mean():.3f} ({r.min():.3f} .. {r.max():.3f})   {ms.mean():8.3f} ms")
    for s, v in fallback.items():
        log(f"  fallback share of pixels at scale {s} (wsum == 0): {np.mean(v):.5f}")
    return {k: float(np.mean([x[0] for x in v])) for k, v in rows.items()}


def quality(gpu, out_path):
    from tests import lights_common as LC
    seeds = range(11, 19)

    def make_render(p0):
        def render(c, p, samples, seed):
            p.samples, p.seed = samples, seed
            return gpu.render(c, p)
        return render

    # the sweep, at 400 x 225 on one seed: half size 16 spp, upsampled with and without the a-trous filter in front
    w, h = 400, 225
    cam, p = book1(gpu, w, h)
    render = make_render(p)
    truth = render(cam, p, 4096, 1)[0].astype(np.float64)
    mse = lambda img: float(((img.astype(np.float64) - truth) ** 2).mean())
    base = mse(render(cam, p, 4, 7)[0])
    hi = surf(gpu, cam, p)
    log(f"# sweep: Book-1 final scene, output {w} x {h}, SAMPLER_ROW, gamma 1, seed 7; MSE against 4096 spp at the output size as a share of the 4-spp full-size frame's ({base:.6f})")
    best = None
    for s, spp in ((2, 16), (4, 64)):
        lcam, lp = low_view(cam, p, s)
        lo = surf(gpu, lcam, lp)
        fr = render(lcam, lp, spp, 7)[0]
        fa = gpu.atrous_filter(fr, depth=lo["depth"], normal=lo["normal"], ids=lo["idx"], albedo=lo["albedo"], emitted=lo["emitted"])[0]
        for radius, sd, sn, same in itertools.product((1, 2), (0.0, 0.05, 0.25, 1.0), (0.0, 0.1, 0.3, 1.0), (False, True)):
            kw = dict(radius=radius, sigma_depth=sd, sigma_normal=sn, same_object=same)
            a, ws, _ = gpu.upsample_filter(fr, (w, h), lo=lo, hi=hi, scale=s, out_wsum=True, **kw)
            b = gpu.upsample_filter(fa, (w, h), lo=lo, hi=hi, scale=s, **kw)[0]
            log(f"  scale {s} radius {radius} depth {sd:4.2f} normal {sn:4.2f} same_object {int(same)}   upsample {mse(a) / base:.3f}   a-trous + upsample {mse(b) / base:.3f}"
                f"   fallback {float((ws == 0).mean()):.5f}")
            if s == 2:
                score = mse(a) + mse(b)
                if best is None or score < best[0]:
                    best = (score, kw)
    ukw = best[1]
    log(f"# the sweep's best row at scale 2 (least sum of the two columns): {ukw}; UPSAMPLE_DEFAULTS is {R.UPSAMPLE_DEFAULTS}")
    save(out_path)
    columns(gpu, cam, p, seeds, truth, ukw, render, f"Book-1 {w} x {h}, the best row")
    defaults = {k: R.UPSAMPLE_DEFAULTS[k] for k in ("radius", "sigma_depth", "sigma_normal", "same_object")}
    if defaults != ukw:
        columns(gpu, cam, p, seeds, truth, defaults, render, f"Book-1 {w} x {h}, UPSAMPLE_DEFAULTS")
    columns(gpu, cam, p, seeds, truth, dict(radius=1, sigma_depth=0.25, sigma_normal=0.3, same_object=True), render,
            f"Book-1 {w} x {h}, the a-trous filter's sigmas at radius 1 (depth 0.25, normal 0.3, same_object)")
    save(out_path)

    cam, p = book1(gpu, W, H)
    render = make_render(p)
    truth = render(cam, p, 4096, 1)[0].astype(np.float64)
    columns(gpu, cam, p, seeds, truth, ukw, render, f"Book-1 {W} x {H}, the best row")
    save(out_path)

    # the Book-1 orbit of profiles/temporal.log through SvgfDenoiser: scale 2 at 16 spp against scale 1 at 4 spp
    w, h, n_frames, step = 400, 225, 16, 0.25
    cam, p = book1(gpu, w, h)
    render = make_render(p)
    cams = [orbit(cam, step * k) for k in range(n_frames)]
    truths = [render(c, p, 4096, 1)[0].astype(np.float64) for c in cams]
    log(f"# Book-1 orbit, {n_frames} cameras {step} degrees apart, {w} x {h}: SvgfDenoiser, MSE of the filtered frame against 4096 spp, mean of frames {n_frames // 2} .. {n_frames - 1}")
    singles = []
    for c, t in zip(cams, truths):
        singles.append(float(((render(c, p, 4, 100)[0].astype(np.float64) - t) ** 2).mean()))
    single = float(np.mean(singles[n_frames // 2:]))
    for scale, spp in ((1, 4), (2, 16), (4, 64)):
        den = R.SvgfDenoiser(gpu, scale=scale, upsample=ukw)
        p.samples, p.seed = spp, 200
        errs, ms = [], []
        for c, t in zip(cams, truths):
            frame, _, _, st = den.step(c, p)
            errs.append(float(((frame.astype(np.float64) - t) ** 2).mean()))
            ms.append(st["render"].kernel_ms + st["temporal"].filter_ms + st["variance"].filter_ms + st["svgf"].filter_ms
                      + (st["upsample"].filter_ms if scale > 1 else 0.0))
        late = float(np.mean(errs[n_frames // 2:]))
        log(f"  SvgfDenoiser(scale={scale}) at {spp:2d} spp   MSE {late:.6f} = {late / single:.3f} of a single 4-spp frame's   {np.mean(ms):7.3f} ms a frame (render + passes)")
    save(out_path)

    # the light scene's light-biased frames, through a Viewport camera at the golden camera's place
    ls, g = LC.golden()
    w, h = 400, 300
    lcam = LC.camera_no_rand(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    integ, depth = R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"]
    lp0 = ls.params(w, h, integ, depth, seed=1, sampler=R.SAMPLER_ROW, samples=4, gamma=1.0, mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
    try:
        render = make_render(lp0)
        truth = render(lcam, lp0, 4096, 2)[0].astype(np.float64)
        columns(gpu, lcam, lp0, seeds, truth, ukw, render, f"rust2_light_scene {w} x {h}, LIGHT_BIASED, the best row")
    except R.RtwError as e:
        log(f"  unmeasured: {e}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0])) if args and args[0].isdigit() else 9
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if R.device_count() < 1:
        sys.exit("measure_upsample.py: no HIP device visible; the measurements need the MI355X")
    with R.Renderer(0) as gpu:
        timings(gpu, reps)
        save(out)
        if "--quality" in sys.argv:
            quality(gpu, out)
    save(out)


if __name__ == "__main__":
    main()
