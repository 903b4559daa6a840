#!/usr/bin/env python3
"""The temporal accumulation's numbers for DESIGN.md 8d and profiles/temporal.log.

  timings  filter_ms (the one launch, hipEvent) at 1920 x 1080 on the Book-1 final scene's own guides (surface_map at the pixel centres):
           a static camera and a camera carried 0.5 degrees along an orbit, each with every test on and with none, median of `repeats`
           calls after a warm-up, with the history coverage of the call.  For scale, in the same run: one a-trous level and surface_map.
  depth    (--parent-tree PATH) scripts/measure_depth.py in child processes, alternating between a built checkout of the parent commit
           at PATH and this tree, twice each: nothing else moved.
  quality  (--quality) the mean squared error against a 4096-spp render of the same view, gamma 1, along an orbit of 16 cameras 0.25 degrees
           apart and under a static camera, 4 spp per frame, of: the single frames, the a-trous filter on each (render_denoised's chain),
           the accumulation alone, and accumulation + a-trous -- all four from the same rendered frames.  The Book-1 small view, and the
           light scene under INTEGRATOR_LIGHT_BIASED, with the parameters the sweep starts from (START).  Then a sweep of alpha, depth_tol and
           normal_cos on the Book-1 orbit, alpha 0 at three history caps, and the library's TEMPORAL_DEFAULTS on every sequence.

    python scripts/measure_temporal.py [repeats] [--quality] [--parent-tree PATH] [--out profiles/temporal.log]
"""
import itertools
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
START = dict(alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1)     # SVGF's alpha; unmeasured guesses
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def median_ms(call, reps):
    call()
    ms = [call()[2].filter_ms for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms)


def timings(gpu, reps):
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    look = tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]))
    cam0 = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=look, vup=(0.0, 1.0, 0.0)).camera()
    cam1 = orbit(cam0, 0.5)
    g0, g1 = (gpu.surface_map(c, W, H, MINT, MAXT, R.INTEGRATOR_GRADIENT, R.RAYS_PIXEL, OFFSET) for c in (cam0, cam1))
    rng = np.random.default_rng(9)
    f0, f1 = ((rng.random((H, W, 3)) * 2.0).astype(np.float32) for _ in range(2))
    on = dict(alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1, offset=OFFSET)
    off = dict(on, depth_tol=0.0, normal_cos=0.0, same_object=0)
    hist = gpu.temporal_accumulate(f0, cam0, depth=g0["depth"], normal=g0["normal"], ids=g0["idx"], **on)[0]
    log(f"# temporal_accumulate filter_ms at {W} x {H}, Book-1 final scene's guides: median of {reps} after a warm-up (min .. max), history coverage")
    for cname, cam, g in (("static camera", cam0, g0), ("camera moved 0.5 degrees", cam1, g1)):
        for tname, prm in (("every test on", on), ("no test", off)):
            call = lambda: gpu.temporal_accumulate(f1, cam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist, **prm)
            med, lo, hi = median_ms(call, reps)
            cover = float((call()[0]["len"] > 1).mean())
            log(f"  {cname}, {tname}".ljust(52) + f"{med:7.3f} ms ({lo:.3f} .. {hi:.3f})   coverage {cover:.4f}")
    med, lo, hi = median_ms(lambda: gpu.temporal_accumulate(f1, cam0, depth=g0["depth"], normal=g0["normal"], ids=g0["idx"], **on), reps)
    log(f"  first frame (no history)".ljust(52) + f"{med:7.3f} ms ({lo:.3f} .. {hi:.3f})")
    kw = dict(depth=g0["depth"], normal=g0["normal"], ids=g0["idx"], albedo=g0["albedo"], emitted=g0["emitted"])
    call = lambda: gpu.atrous_filter(f1, levels=1, **kw)
    call()
    ms = [call()[1].filter_ms for _ in range(reps)]
    log(f"  for scale: one a-trous level (with demodulation)".ljust(52) + f"{np.median(ms):7.3f} ms ({min(ms):.3f} .. {max(ms):.3f})")
    run = lambda: gpu.surface_map(cam0, W, H, MINT, MAXT, R.INTEGRATOR_GRADIENT)["stats"].kernel_ms
    run()
    ms = [run() for _ in range(reps)]
    log(f"  for scale: surface_map (all six buffers)".ljust(52) + f"{np.median(ms):7.3f} ms ({min(ms):.3f} .. {max(ms):.3f})")


def depth_ab(parent_tree):
    log("# depth_map through the parent commit's package and library and through this tree's, alternating, a child process each (scripts/measure_depth.py)")
    env = dict(os.environ)
    env.pop("RTW_HIP_LIB", None)
    for rnd in (1, 2):
        for name, tree in (("parent", os.path.abspath(parent_tree)), ("this", ROOT)):
            out = subprocess.run([sys.executable, os.path.join(tree, "scripts", "measure_depth.py"), "7"], env=env, cwd=tree, capture_output=True,
                                 text=True, timeout=300)
            log(f"## depth {name} {rnd}" + ("" if out.returncode == 0 else f"  (exit status {out.returncode})"))
            for line in out.stdout.splitlines():
                log(line)
            if out.returncode != 0:
                log(out.stderr[-2000:])
                return


def sequence(render, guides, cams, truths):
    """The rendered frames, their guides and the 4096-spp frames of a list of cameras."""
    frames = [render(c, 4, 100 + k) for k, c in enumerate(cams)]
    return frames, [guides(c) for c in cams], truths


def evaluate(gpu, frames, gs, cams, truths, prm, atrous=True):
    """Per frame the MSE of (single, a-trous alone, accumulated, accumulated + a-trous) and the coverage."""
    mse = lambda img, t: float(((img.astype(np.float64) - t) ** 2).mean())
    hist, rows = None, []
    for cur, g, cam, t in zip(frames, gs, cams, truths):
        kw = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
        hist, _, _ = gpu.temporal_accumulate(cur, cam, history=hist, offset=OFFSET, **kw, **prm)
        acc = hist["color"]
        if atrous:
            a_only = gpu.atrous_filter(cur, albedo=g["albedo"], emitted=g["emitted"], **kw)[0]
            both = gpu.atrous_filter(acc, albedo=g["albedo"], emitted=g["emitted"], **kw)[0]
            rows.append((mse(cur, t), mse(a_only, t), mse(acc, t), mse(both, t), float((hist["len"] > 1).mean())))
        else:
            rows.append((mse(cur, t), float("nan"), mse(acc, t), float("nan"), float((hist["len"] > 1).mean())))
    return rows


def report(label, rows):
    for k, (single, a_only, acc, both, cover) in enumerate(rows):
        log(f"  {label} frame {k}: single {single:.6f}  a-trous {a_only:.6f} ({a_only / single:.3f})  accumulated {acc:.6f} ({acc / single:.3f})"
            f"  accumulated + a-trous {both:.6f} ({both / single:.3f})  coverage {cover:.3f}")
    tail = np.array(rows[len(rows) // 2:])
    m = tail.mean(axis=0)
    log(f"  {label} mean of frames {len(rows) // 2} .. {len(rows) - 1}: single {m[0]:.6f}  a-trous {m[1]:.6f} ({m[1] / m[0]:.3f})  accumulated {m[2]:.6f} ({m[2] / m[0]:.3f})"
        f"  accumulated + a-trous {m[3]:.6f} ({m[3] / m[0]:.3f})")
    return m


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
    defaults = dict(START)
    log(f"# quality: Book-1 final scene {w} x {h}, SAMPLER_ROW, gamma 1, 4 spp per frame; MSE against a 4096-spp render of each view (ratio to the single frame)")
    log(f"#   parameters {defaults}; a-trous at its defaults {R.ATROUS_DEFAULTS} with albedo and emission")
    book = {}
    for label, deg in (("book1 orbit", step), ("book1 static", 0.0)):
        cams = [orbit(cam, deg * k) for k in range(n_frames)]
        truths = [render(c, 4096, 1).astype(np.float64) for c in (cams if deg else cams[:1])] * (1 if deg else n_frames)
        frames, gs, truths = sequence(render, guides, cams, truths)
        book[label] = (frames, gs, cams, truths)
        report(label, evaluate(gpu, frames, gs, cams, truths, defaults))

    log(f"# sweep on the Book-1 orbit: mean MSE of frames {n_frames // 2} .. {n_frames - 1}, accumulated and accumulated + a-trous (ratio to the single frames' mean)")
    frames, gs, cams, truths = book["book1 orbit"]
    best = best2 = None
    for alpha, tol, cos in itertools.product((0.05, 0.1, 0.2, 0.4), (0.01, 0.05, 0.2), (0.0, 0.5, 0.9, 0.99)):
        prm = dict(defaults, alpha=alpha, alpha_moments=alpha, depth_tol=tol, normal_cos=cos)
        m = np.array(evaluate(gpu, frames, gs, cams, truths, prm)[n_frames // 2:]).mean(axis=0)
        log(f"  alpha {alpha:4.2f} depth_tol {tol:4.2f} normal_cos {cos:4.2f}   accumulated {m[2]:.6f} ({m[2] / m[0]:.3f})   accumulated + a-trous {m[3]:.6f} ({m[3] / m[0]:.3f})"
            f"   coverage {m[4]:.3f}")
        if best is None or m[2] < best[0]:
            best = (m[2], alpha, tol, cos)
        if best2 is None or m[3] < best2[0]:
            best2 = (m[3], alpha, tol, cos)
    log(f"# best row by the accumulated colour: alpha {best[1]} depth_tol {best[2]} normal_cos {best[3]}, MSE {best[0]:.6f}")
    log(f"# best row by accumulated + a-trous:  alpha {best2[1]} depth_tol {best2[2]} normal_cos {best2[3]}, MSE {best2[0]:.6f}")
    for hist_max in (8, 32, 128):
        prm = dict(defaults, alpha=0.0, alpha_moments=0.0, max_history=hist_max, depth_tol=best[2], normal_cos=best[3])
        m = np.array(evaluate(gpu, frames, gs, cams, truths, prm)[n_frames // 2:]).mean(axis=0)
        log(f"  alpha 0 (running mean), max_history {hist_max:3d}, the best row's tests   accumulated {m[2]:.6f} ({m[2] / m[0]:.3f})   accumulated + a-trous {m[3]:.6f} ({m[3] / m[0]:.3f})")

    # the light scene under LIGHT_BIASED, through a Viewport camera at the golden camera's place (the accumulation is built for those only)
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
    lib_defaults = dict(R.TEMPORAL_DEFAULTS)
    log(f"# the library's TEMPORAL_DEFAULTS {lib_defaults}")
    for label in book:
        report(label + ", TEMPORAL_DEFAULTS", evaluate(gpu, *book[label], lib_defaults))
    log(f"# quality: rust2_light_scene {w} x {h}, LIGHT_BIASED, SAMPLER_ROW, gamma 1, 4 spp per frame, a Viewport camera; MSE against 4096 spp")
    try:
        for label, deg in (("lights orbit", step), ("lights static", 0.0)):
            cams = [orbit(lcam, deg * k) for k in range(n_frames)]
            truths = [lrender(c, 4096, 2).astype(np.float64) for c in (cams if deg else cams[:1])] * (1 if deg else n_frames)
            frames, gs, truths = sequence(lrender, lguides, cams, truths)
            report(label, evaluate(gpu, frames, gs, cams, truths, defaults))
            report(label + ", TEMPORAL_DEFAULTS", evaluate(gpu, frames, gs, cams, truths, lib_defaults))
    except R.RtwError as e:
        log(f"  unmeasured: {e}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0])) if args and args[0].isdigit() else 9
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if "--parent-tree" in sys.argv:
        depth_ab(sys.argv[sys.argv.index("--parent-tree") + 1])
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
