#!/usr/bin/env python3
"""The numbers of temporal accumulation with moving objects for DESIGN.md 8f and profiles/temporal_motion.log.

  timings  filter_ms (hipEvent) at 1920 x 1080 on the Book-1 final scene's own guides (485 objects), median of `repeats` calls after a
           warm-up, in one run: the existing call; the new call without rows; with a table of 1024 and of 65 536 rows, none moving; the
           same tables with every row moving, under a static and under a moved camera; and rtw_ctx_mesh_instance_motion for 1024 and
           65 536 placements (device tensors, the call's wall time) beside move_mesh_instances of the same.
  parent   (--parent-tree PATH) the existing call's filter_ms and bench.py --gpus 1 through a built checkout of the parent commit at PATH
           and through this tree, alternating, a child process each: the existing path did not move.
  quality  (--quality) placed icospheres that translate and turn every frame over a ground sphere and three spheres, 400 x 225, 4 spp,
           INTEGRATOR_RUST2, SAMPLER_ROW, gamma 1, 16 frames, a static camera and DESIGN.md 8d's 0.25-degree orbit; MSE against a 4096-spp
           render of each frame's own poses: the single frame, accumulated under the static-world rule, accumulated with motion, and the
           SVGF chain with motion -- over the whole frame and over the moving objects' pixels alone, with the history coverage of each.

    python scripts/measure_temporal_motion.py [repeats] [--quality] [--parent-tree PATH] [--out profiles/temporal_motion.log]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

try:                                                   # before the first rtw call: the library then shares the HIP runtime torch loaded (tests/conftest.py)
    import torch
except Exception:                                      # (only the timings need it)
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R                                    # noqa: E402
from tests.temporal_common import orbit                # noqa: E402

W, H = 1920, 1080
MINT, MAXT = 0.001, 1000.0
OFFSET = (0.5, 0.5)
OUT = [None]                                           # the log file, written line by line
# what a child process of the parent A/B runs in either tree: only calls both trees have
TEMPORAL_CHILD = """
import numpy as np, rtw_amd as R
from tests.temporal_common import orbit
W, H = 1920, 1080
look = tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]))
cam0 = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=look, vup=(0.0, 1.0, 0.0)).camera()
cam1 = orbit(cam0, 0.5)
with R.Renderer(0) as gpu:
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    g0, g1 = (gpu.surface_map(c, W, H, 0.001, 1000.0, R.INTEGRATOR_GRADIENT, R.RAYS_PIXEL, (0.5, 0.5)) for c in (cam0, cam1))
    rng = np.random.default_rng(9)
    f0, f1 = ((rng.random((H, W, 3)) * 2.0).astype(np.float32) for _ in range(2))
    kw = lambda g: dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
    first = gpu.temporal_accumulate(f0, cam0, offset=(0.5, 0.5), **kw(g0))[0]
    for name, cam, g in (("static", cam0, g0), ("moved", cam1, g1)):
        call = lambda: gpu.temporal_accumulate(f1, cam, history=first, offset=(0.5, 0.5), **kw(g))[2].filter_ms
        call()
        ms = [call() for _ in range(15)]
        print(f"temporal_accumulate {name} camera: median of 15 {np.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})", end="; ")
print()
"""


def log(s=""):
    print(s, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as f:
            f.write(s + "\n")


def median_of(call, reps):
    call()
    ms = [call() for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms)


def fmt(t):
    return f"{t[0]:7.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


def small_motions(n, seed):
    """(prev, cur) poses [n][7] of n small rigid motions about the origin: a shift of a few hundredths, a turn of a degree or two."""
    rng = np.random.default_rng(seed)
    prev, cur = np.zeros((n, 7), np.float32), np.zeros((n, 7), np.float32)
    prev[:, 3] = 1.0
    cur[:, :3] = rng.uniform(-0.03, 0.03, (n, 3))
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    half = np.deg2rad(rng.uniform(0.5, 2.0, n)) / 2.0
    cur[:, 3], cur[:, 4:] = np.cos(half), ax * np.sin(half)[:, None]
    return prev, cur


def timings(gpu, reps):
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    look = tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]))
    cam0 = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=look, vup=(0.0, 1.0, 0.0)).camera()
    cam1 = orbit(cam0, 0.5)
    g0, g1 = (gpu.surface_map(c, W, H, MINT, MAXT, R.INTEGRATOR_GRADIENT, R.RAYS_PIXEL, OFFSET) for c in (cam0, cam1))
    rng = np.random.default_rng(9)
    f0, f1 = ((rng.random((H, W, 3)) * 2.0).astype(np.float32) for _ in range(2))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    kw = lambda g: dict(depth=dev(g["depth"]), normal=dev(g["normal"]), ids=dev(g["idx"]))
    k0, k1 = kw(g0), kw(g1)
    t0, t1 = dev(f0), dev(f1)
    first = gpu.temporal_accumulate(t0, cam0, offset=OFFSET, **k0)[0]
    ids = g0["idx"]
    log(f"# temporal_accumulate filter_ms at {W} x {H}, Book-1 final scene's guides ({int(ids.max()) + 1} objects, {float((ids < 0).mean()):.3f} of the pixels a miss),")
    log(f"# every term on (TEMPORAL_DEFAULTS), every buffer a device tensor: median of {reps} after a warm-up (min .. max), one run")
    tables = {}
    for n in (1024, 65536):
        prev, cur = small_motions(n, n)
        tables[n] = (dev(R.motion_rows(n).view(np.float32).reshape(n, 32)), gpu.mesh_instance_motion(dev(prev), dev(cur))[0])
    for name, cam, k in (("static camera", cam0, k0), ("moved camera (0.5 degrees of orbit)", cam1, k1)):
        base = dict(history=first, offset=OFFSET, **k)
        rows = [("existing call (rtw_ctx_temporal_accumulate)", {}), ("new call, rows NULL, out_prev_xy NULL", dict(motion_first=1)),
                ("new call, out_prev_xy alone", dict(out_prev_xy=True))]
        for n in (1024, 65536):
            rows.append((f"table of {n} rows, none moving", dict(motion=tables[n][0])))
            rows.append((f"table of {n} rows, every row moving", dict(motion=tables[n][1])))
            rows.append((f"table of {n} rows, every row moving, out_prev_xy", dict(motion=tables[n][1], out_prev_xy=True)))
        for label, extra in rows:
            t = median_of(lambda: gpu.temporal_accumulate(t1, cam, **base, **extra)[2].filter_ms, reps)
            cover = float((gpu.temporal_accumulate(t1, cam, **base, **extra)[0]["len"] > 1).float().mean())
            log(f"  {name}: {label}".ljust(92) + fmt(t) + f"   coverage {cover:.3f}")

    log(f"# rtw_ctx_mesh_instance_motion beside move_mesh_instances, device tensors in place, the call's wall time (it ends in its one synchronise): median of {reps} (min .. max)")
    vtx, faces = R.mesh_icosphere(1, radius=0.3)
    gpu.set_scene(R.Scene([R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), R.SCATTER_M)], background=(0.7, 0.8, 1.0)))
    gpu.set_triangles(R.Triangle.from_mesh(vtx, faces))
    for n in (1024, 65536):
        side = int(round(n ** 0.5))
        grid = np.zeros((n, 7), np.float32)
        grid[:, 0], grid[:, 2], grid[:, 1], grid[:, 3] = np.repeat(np.arange(side), side)[:n], np.tile(np.arange(side), side)[:n], 0.5, 1.0
        moved = grid.copy()
        moved[:, :3] += small_motions(n, 5)[1][:, :3]
        moved[:, 3:] = small_motions(n, 5)[1][:, 3:]
        gpu.set_mesh_instances([(p[:3], p[3:]) for p in grid])
        tp, tc = dev(grid), dev(moved)
        torch.cuda.synchronize()

        def wall(call):
            t = time.perf_counter()
            call()
            return (time.perf_counter() - t) * 1e3
        t_rows = median_of(lambda: wall(lambda: gpu.mesh_instance_motion(tp, tc)), reps)
        t_move = median_of(lambda: wall(lambda: gpu.move_mesh_instances(tc)), reps)
        log(f"  {n:6d} placements: mesh_instance_motion {fmt(t_rows)}   move_mesh_instances {fmt(t_move)}")
    gpu.set_mesh_instances(None)


def parent_ab(parent_tree, rounds=2):
    log("# the existing call and bench.py --gpus 1 through the parent commit's package and library and through this tree's, alternating, a child process each")
    env = dict(os.environ)
    env.pop("RTW_HIP_LIB", None)
    for rnd in range(1, rounds + 1):
        for name, tree in (("parent", os.path.abspath(parent_tree)), ("this", ROOT)):
            for what, cmd in (("temporal", [sys.executable, "-c", TEMPORAL_CHILD]),
                              ("bench", [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"])):
                out = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=400)
                tail = [ln for ln in out.stdout.splitlines() if ln.strip()][-1:] if out.returncode == 0 else [out.stderr[-1500:]]
                if what == "bench" and out.returncode == 0:
                    j = json.loads(tail[0])
                    tail = [f"{j['value']:.1f} {j['unit']}, {j['ms_per_step']:.3f} ms per step (--steps {j['steps']} --warmup {j['warmup']})"]
                log(f"  {what} {name} {rnd}: " + (tail[0] if tail else "") + ("" if out.returncode == 0 else f"  (exit status {out.returncode})"))
                if out.returncode != 0:
                    return


def mse(img, t, mask=None):
    d = (np.asarray(img, np.float64) - t) ** 2
    return float(d.mean() if mask is None else d[mask].mean())


def quality(gpu):
    w, h, n_frames, step = 400, 225, 16, 0.25
    eye = np.array([13.0, 2.0, 3.0])
    vp = R.Viewport.new_from_res(w, h, 4, 8, 1.0, vfov=20.0, origin=tuple(eye), direction=tuple(-eye / np.linalg.norm(eye)), vup=(0.0, 1.0, 0.0))
    assert vp.height == h
    cam = vp.camera()
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = w, h, 4, 8, 1.0
    p.mint, p.maxt = MINT, MAXT
    p.integrator, p.sampler, p.accel, p.flags = R.INTEGRATOR_RUST2, R.SAMPLER_ROW, R.ACCEL_BVH, 0
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    spheres = [R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), R.SCATTER_M), R.Sphere.new((0.0, 1.0, 0.0), 1.0, (0.7, 0.3, 0.3), R.SCATTER_M),
               R.Sphere.new((-4.0, 1.0, 0.0), 1.0, (0.3, 0.4, 0.7), R.SCATTER_M), R.Sphere.new((4.0, 1.0, 0.0), 1.0, (0.7, 0.6, 0.5), R.SCATTER_M)]
    gpu.set_scene(R.Scene(spheres, background=(0.7, 0.8, 1.0)))
    vtx, faces = R.mesh_icosphere(2, radius=0.45)
    gpu.set_triangles(R.Triangle.from_mesh(vtx, faces, color=(0.8, 0.7, 0.2)))
    first = gpu.mesh_instance_first()
    n_obj = 6

    def poses(k):
        """Frame k: six icospheres on a circle of radius 2.4 about the middle sphere, each carried 1.5 degrees along it per frame and turned
        by 8 degrees per frame about an axis of its own."""
        out = np.zeros((n_obj, 7), np.float32)
        for j in range(n_obj):
            a = np.deg2rad(60.0 * j + 1.5 * k)
            out[j, :3] = (2.4 * np.cos(a), 0.45 + 0.25 * (j % 3), 2.4 * np.sin(a))
            ax = np.array([np.sin(1.0 + j), 1.0, np.cos(2.0 * j)])
            ax /= np.linalg.norm(ax)
            t = np.deg2rad(8.0 * k + 20.0 * j) / 2.0
            out[j, 3], out[j, 4:] = np.cos(t), np.sin(t) * ax
        return out

    gpu.set_mesh_instances([(q[:3], q[3:]) for q in poses(0)])

    def render(c, samples, seed):
        p.samples, p.seed = samples, seed
        return gpu.render(c, p)[0]

    log(f"# quality: {n_obj} placed icospheres (level 2, radius 0.45) that move 1.5 degrees along a circle and turn by 8 degrees every frame, over a ground sphere")
    log(f"#   and three spheres; {w} x {h}, INTEGRATOR_RUST2, SAMPLER_ROW, depth 8, gamma 1, 4 spp per frame; MSE against a 4096-spp render of each frame's own poses")
    log(f"#   accumulation at TEMPORAL_DEFAULTS {R.TEMPORAL_DEFAULTS}; the SVGF chain at SVGF_DEFAULTS {R.SVGF_DEFAULTS}")
    log("#   columns: single frame | accumulated, static-world rule | accumulated with motion | SVGF chain with motion; (coverage) = share of the pixels with len > 1")
    for label, deg in (("static camera", 0.0), ("orbit", step)):
        hist_s = hist_m = None
        rows_all, rows_obj = [], []
        for k in range(n_frames):
            c = orbit(cam, deg * k)
            gpu.move_mesh_instances(poses(k))
            truth = render(c, 4096, 1).astype(np.float64)
            cur = render(c, 4, 100 + k)
            g = gpu.surface_map(c, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, OFFSET)
            gk = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
            motion = None if k == 0 else gpu.mesh_instance_motion(poses(k - 1), poses(k))[0]
            hist_s = gpu.temporal_accumulate(cur, c, history=hist_s, offset=OFFSET, **gk)[0]
            hist_m = gpu.temporal_accumulate(cur, c, history=hist_m, motion=motion, motion_first=first, offset=OFFSET, **gk)[0]
            var = gpu.variance_estimate(hist_m["moments"], hist_m["len"], **gk)[0]
            svgf = gpu.svgf_filter(hist_m["color"], var, albedo=g["albedo"], emitted=g["emitted"], **gk)[0]
            obj = g["idx"] >= first
            cov = lambda hs, m=None: float((hs["len"] > 1).mean() if m is None else (hs["len"] > 1)[m].mean())
            rows_all.append((mse(cur, truth), mse(hist_s["color"], truth), mse(hist_m["color"], truth), mse(svgf, truth), cov(hist_s), cov(hist_m)))
            rows_obj.append((mse(cur, truth, obj), mse(hist_s["color"], truth, obj), mse(hist_m["color"], truth, obj), mse(svgf, truth, obj),
                             cov(hist_s, obj), cov(hist_m, obj), float(obj.mean())))
        line = lambda r: (f"single {r[0]:.6f} | static-world {r[1]:.6f} ({r[1] / r[0]:.3f}, coverage {r[4]:.3f}) | with motion {r[2]:.6f} "
                          f"({r[2] / r[0]:.3f}, coverage {r[5]:.3f}) | SVGF with motion {r[3]:.6f} ({r[3] / r[0]:.3f})")
        for k in range(n_frames):
            log(f"  {label} frame {k:2d}, whole frame:    " + line(rows_all[k]))
            log(f"  {label} frame {k:2d}, moving objects: " + line(rows_obj[k]) + f"   [{rows_obj[k][6]:.4f} of the pixels]")
        for name, rows in (("whole frame", rows_all), ("moving objects", rows_obj)):
            m = np.array([r[:6] for r in rows[n_frames // 2:]]).mean(axis=0)
            log(f"  {label} mean of frames {n_frames // 2} .. {n_frames - 1}, {name}: " + line(m))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0])) if args and args[0].isdigit() else 9
    if "--out" in sys.argv:
        OUT[0] = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(OUT[0])), exist_ok=True)
        open(OUT[0], "w").close()
    if "--parent-tree" in sys.argv:
        parent_ab(sys.argv[sys.argv.index("--parent-tree") + 1])
    with R.Renderer(0) as gpu:
        if "--no-timings" not in sys.argv:
            timings(gpu, reps)
        if "--quality" in sys.argv:
            quality(gpu)


if __name__ == "__main__":
    main()
