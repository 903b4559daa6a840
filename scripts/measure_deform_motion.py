#!/usr/bin/env python3
"""The numbers of per-pixel motion for DESIGN.md 8g and profiles/deform_motion.log.

  timings  at 1920 x 1080, median of `repeats` calls after a warm-up, in one run, on a waving sheet of 8192 triangles placed over a ground
           sphere (the Book-1 view): surface_map's kernel_ms (hipEvent) without the two outputs, with tri, with bary and with both, and the
           same on the Book-1 final scene (no triangle: every tri is -1); rtw_ctx_deform_motion unplaced and placed (device tensors, the
           call's wall time, which ends in its one synchronise); temporal_accumulate's filter_ms (hipEvent) through the _motion call and
           through the _points call with points on no pixel (all NaN), on the sheet's pixels, and on every pixel, with and without
           carried_normal.
  parent   (--parent-tree PATH) surface_map's kernel_ms, the existing temporal call's filter_ms and bench.py --gpus 1 through a built
           checkout of the parent commit at PATH and through this tree, alternating, a child process each: the existing paths did not move.
  quality  (--quality) the sheet waving and swaying over a ground sphere and three spheres, 400 x 225, 4 spp, INTEGRATOR_RUST2, SAMPLER_ROW,
           gamma 1, 12 frames, a static camera and DESIGN.md 8d's 0.25-degree orbit; MSE on the sheet's pixels against a 1024-spp render of
           each frame's own shape: the single frame, accumulated under the static-world rule, accumulated with per-pixel points.

    python scripts/measure_deform_motion.py [repeats] [--quality] [--parent-tree PATH] [--out profiles/deform_motion.log]
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
CHILD = """
import numpy as np, rtw_amd as R
from tests.temporal_common import orbit
W, H = 1920, 1080
look = tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]))
cam0 = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=look, vup=(0.0, 1.0, 0.0)).camera()
cam1 = orbit(cam0, 0.5)
with R.Renderer(0) as gpu:
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    smap = lambda c: gpu.surface_map(c, W, H, 0.001, 1000.0, R.INTEGRATOR_GRADIENT, R.RAYS_PIXEL, (0.5, 0.5))
    smap(cam0)
    ms = [smap(cam0)["stats"].kernel_ms for _ in range(15)]
    print(f"surface_map: median of 15 {np.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})", end="; ")
    g0, g1 = smap(cam0), smap(cam1)
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


def sheet(n_side, phase, half_y=1.6, half_z=2.4, amplitude=0.25):
    """A grid in the plane x = 0 bent by a wave that travels with `phase` (tests/deform_motion_common.py's): (vertices, faces)."""
    g = np.linspace(-1.0, 1.0, n_side + 1)
    yy, zz = np.meshgrid(g * half_y, g * half_z, indexing="ij")
    x = amplitude * np.sin(1.3 * zz + 0.9 * yy + phase)
    v = np.stack([x, yy + 0.10 * np.sin(phase + zz), zz + 0.08 * np.cos(phase + 1.7 * yy)], -1).reshape(-1, 3).astype(np.float32)
    k = np.arange(n_side * n_side)
    a = k // n_side * (n_side + 1) + k % n_side
    return v, np.concatenate([np.stack([a, a + 1, a + n_side + 1], 1), np.stack([a + 1, a + n_side + 2, a + n_side + 1], 1)])


def pose(k):
    """Frame k's pose of the sheet [1][7]: it stands 1.8 above the ground, sways by 0.04 a frame and turns by one degree a frame."""
    t = np.deg2rad(20.0 + 1.0 * k) / 2.0
    ax = np.array([0.2, 1.0, -0.3]) / np.linalg.norm([0.2, 1.0, -0.3])
    return np.array([[0.0, 1.8 + 0.04 * np.sin(0.7 * k), 0.04 * k, np.cos(t), *(np.sin(t) * ax)]], np.float32)


def book1_camera(w, h):
    look = tuple(float(x) for x in -np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]))
    return R.Viewport.new_from_res(w, h, 1, 1, 1.0, vfov=20.0, origin=(13.0, 2.0, 3.0), direction=look, vup=(0.0, 1.0, 0.0)).camera()


def timings(gpu, reps):
    cam0 = book1_camera(W, H)
    cam1 = orbit(cam0, 0.5)
    smap = lambda c, **kw: gpu.surface_map(c, W, H, MINT, MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, OFFSET, **kw)
    log(f"# surface_map kernel_ms at {W} x {H}, host outputs: median of {reps} after a warm-up (min .. max), one run")
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    for label, kw in (("existing call", {}), ("tri", dict(tri=True)), ("bary", dict(bary=True)), ("tri and bary", dict(tri=True, bary=True))):
        log(f"  Book-1 final scene (485 spheres, no triangle), {label}:".ljust(72) + fmt(median_of(lambda: smap(cam0, **kw)["stats"].kernel_ms, reps)))
    n_side = 64
    (v0, f), (v1, _) = sheet(n_side, 0.0), sheet(n_side, 0.35)
    ouv0, ouv1 = R.mesh_ouv(v0, f), R.mesh_ouv(v1, f)
    gpu.set_scene(R.Scene([R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), R.SCATTER_M)], background=(0.7, 0.8, 1.0)))
    gpu.set_triangles(R.Triangle.from_mesh(v0, f, color=(0.8, 0.7, 0.2)))
    gpu.set_mesh_instances([(pose(0)[0, :3], pose(0)[0, 3:])])
    first = gpu.mesh_instance_first()
    g0 = smap(cam0)
    gpu.move_mesh_instances(pose(1), ouv1)
    for label, kw in (("existing call", {}), ("tri", dict(tri=True)), ("bary", dict(bary=True)), ("tri and bary", dict(tri=True, bary=True))):
        log(f"  waving sheet ({len(f)} triangles, placed) over a ground sphere, {label}:".ljust(72) + fmt(median_of(lambda: smap(cam1, **kw)["stats"].kernel_ms, reps)))
    g1 = smap(cam1, tri=True, bary=True)
    on = g1["tri"] >= 0
    log(f"#   the sheet covers {float(on.mean()):.3f} of the frame")

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def wall(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        return (time.perf_counter() - t) * 1e3
    log(f"# rtw_ctx_deform_motion at {W} x {H}, every buffer a device tensor, the call's wall time (it ends in its one synchronise): median of {reps} (min .. max)")
    t_tri, t_bary, t_idx, t_ouv, t_pose = dev(g1["tri"]), dev(g1["bary"]), dev(g1["idx"]), dev(ouv0), dev(pose(0))
    outs = (torch.empty((H, W, 3), device="cuda:0"), torch.empty((H, W, 3), device="cuda:0"))
    C = R.C
    ptr = lambda t: C.c_void_p(t.data_ptr())
    raw = lambda placed: R.lib().rtw_ctx_deform_motion(gpu._h, ptr(t_tri), ptr(t_bary), W * H, ptr(t_ouv), len(f), ptr(t_idx) if placed else None,
                                                       ptr(t_pose) if placed else None, 1 if placed else 0, first, ptr(outs[0]), ptr(outs[1]))
    for label, placed in (("unplaced", False), ("placed", True)):
        log(f"  {label}:".ljust(72) + fmt(median_of(lambda: wall(lambda: raw(placed)), reps)))
    assert raw(True) == 0
    point, carried = outs

    log(f"# temporal_accumulate filter_ms at {W} x {H}, the sheet's guides, every term on (TEMPORAL_DEFAULTS), every buffer a device tensor:")
    log(f"# median of {reps} after a warm-up (min .. max), one run")
    rng = np.random.default_rng(9)
    t0, t1 = (dev((rng.random((H, W, 3)) * 2.0).astype(np.float32)) for _ in range(2))
    kw = lambda g: dict(depth=dev(g["depth"]), normal=dev(g["normal"]), ids=dev(g["idx"]))
    k0, k1 = kw(g0), kw(g1)
    hist = gpu.temporal_accumulate(t0, cam0, offset=OFFSET, **k0)[0]
    # points on every pixel: the sheet's own, and for the rest the pixel's world point itself (the static world, through the points rule)
    rays = R.pixel_rays(cam1, W, H, OFFSET).reshape(H, W, 6)
    world = (rays[..., :3] + rays[..., 3:] * g1["depth"][..., None]).astype(np.float32)
    every = torch.where(dev(on)[..., None], point, dev(world))
    nan = torch.full((H, W, 3), float("nan"), device="cuda:0")
    base = dict(history=hist, offset=OFFSET, **k1)
    for label, extra in (("existing call (rtw_ctx_temporal_accumulate)", {}), ("_motion call, rows NULL, out_prev_xy", dict(out_prev_xy=True)),
                         ("_points call, points on no pixel (all NaN)", dict(prev_point=nan)),
                         ("_points call, points on the sheet's pixels", dict(prev_point=point)),
                         ("_points call, points on the sheet's pixels, carried_normal", dict(prev_point=point, carried_normal=carried)),
                         ("_points call, points on every pixel", dict(prev_point=every)),
                         ("_points call, points on every pixel, carried_normal, out_prev_xy", dict(prev_point=every, carried_normal=k1["normal"], out_prev_xy=True))):
        t = median_of(lambda: gpu.temporal_accumulate(t1, cam1, **base, **extra)[2].filter_ms, reps)
        ln = gpu.temporal_accumulate(t1, cam1, **base, **extra)[0]["len"]
        log(f"  {label}:".ljust(72) + fmt(t) + f"   coverage {float((ln > 1).float().mean()):.3f}, on the sheet {float((ln > 1)[dev(on)].float().mean()):.3f}")
    gpu.set_mesh_instances(None)
    gpu.set_triangles(None)


def parent_ab(parent_tree, rounds=2):
    log("# surface_map, the existing temporal call and bench.py --gpus 1 through the parent commit's package and library and through this tree's, alternating, a child process each")
    env = dict(os.environ)
    env.pop("RTW_HIP_LIB", None)
    for rnd in range(1, rounds + 1):
        for name, tree in (("parent", os.path.abspath(parent_tree)), ("this", ROOT)):
            for what, cmd in (("passes", [sys.executable, "-c", CHILD]),
                              ("bench", [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"])):
                out = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=400)
                tail = [ln for ln in out.stdout.splitlines() if ln.strip()][-1:] if out.returncode == 0 else [out.stderr[-1500:]]
                if what == "bench" and out.returncode == 0:
                    j = json.loads(tail[0])
                    tail = [f"{j['value']:.1f} {j['unit']}, {j['ms_per_step']:.3f} ms per step (--steps {j['steps']} --warmup {j['warmup']})"]
                log(f"  {what} {name} {rnd}: " + (tail[0] if tail else "") + ("" if out.returncode == 0 else f"  (exit status {out.returncode})"))
                if out.returncode != 0:
                    return


def mse(img, t, mask):
    return float(((np.asarray(img, np.float64) - t) ** 2)[mask].mean())


def quality(gpu):
    w, h, n_frames, step, truth_spp = 400, 225, 12, 0.25, 1024
    eye = np.array([13.0, 2.0, 3.0])
    vp = R.Viewport.new_from_res(w, h, 4, 8, 1.0, vfov=20.0, origin=tuple(eye), direction=tuple(-eye / np.linalg.norm(eye)), vup=(0.0, 1.0, 0.0))
    assert vp.height == h
    cam = vp.camera()
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = w, h, 4, 8, 1.0
    p.mint, p.maxt = MINT, MAXT
    p.integrator, p.sampler, p.accel, p.flags = R.INTEGRATOR_RUST2, R.SAMPLER_ROW, R.ACCEL_BVH, 0
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    spheres = [R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), R.SCATTER_M), R.Sphere.new((-3.0, 1.0, -2.5), 1.0, (0.7, 0.3, 0.3), R.SCATTER_M),
               R.Sphere.new((-4.0, 1.0, 1.0), 1.0, (0.3, 0.4, 0.7), R.SCATTER_M), R.Sphere.new((-3.0, 1.0, 4.0), 1.0, (0.7, 0.6, 0.5), R.SCATTER_M)]
    gpu.set_scene(R.Scene(spheres, background=(0.7, 0.8, 1.0)))
    n_side = 24
    shape = lambda k: sheet(n_side, 0.35 * k)
    v, f = shape(0)
    gpu.set_triangles(R.Triangle.from_mesh(v, f, color=(0.8, 0.7, 0.2)))
    gpu.set_mesh_instances([(pose(0)[0, :3], pose(0)[0, 3:])])
    first = gpu.mesh_instance_first()

    def render(c, samples, seed):
        p.samples, p.seed = samples, seed
        return gpu.render(c, p)[0]

    log(f"# quality: a sheet of {len(f)} triangles whose wave advances by 0.35 rad a frame (every vertex moves) while its placement sways and turns by one degree a frame,")
    log(f"#   in front of three spheres over a ground sphere; {w} x {h}, INTEGRATOR_RUST2, SAMPLER_ROW, depth 8, gamma 1, 4 spp per frame; MSE on the sheet's pixels")
    log(f"#   against a {truth_spp}-spp render of each frame's own shape; accumulation at TEMPORAL_DEFAULTS {R.TEMPORAL_DEFAULTS}")
    log("#   columns: single frame | accumulated, static-world rule | accumulated with per-pixel points; (coverage) = share of the sheet's pixels with len > 1")
    for label, deg in (("static camera", 0.0), ("orbit", step)):
        hist_s = hist_p = None
        rows = []
        for k in range(n_frames):
            c = orbit(cam, deg * k)
            ouv = R.mesh_ouv(shape(k)[0], f)
            gpu.move_mesh_instances(pose(k), ouv)
            truth = render(c, truth_spp, 1).astype(np.float64)
            cur = render(c, 4, 100 + k)
            g = gpu.surface_map(c, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, OFFSET, tri=True, bary=True)
            gk = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
            points = {}
            if k:
                pt, cn = gpu.deform_motion(g["tri"], g["bary"], prev_ouv, g["idx"], pose(k - 1), first)
                points = dict(prev_point=pt, carried_normal=cn)
            hist_s = gpu.temporal_accumulate(cur, c, history=hist_s, offset=OFFSET, **gk)[0]
            hist_p = gpu.temporal_accumulate(cur, c, history=hist_p, offset=OFFSET, **points, **gk)[0]
            prev_ouv = ouv
            obj = g["tri"] >= 0
            rows.append((mse(cur, truth, obj), mse(hist_s["color"], truth, obj), mse(hist_p["color"], truth, obj), float((hist_s["len"] > 1)[obj].mean()),
                         float((hist_p["len"] > 1)[obj].mean()), float(obj.mean())))
        line = lambda r: (f"single {r[0]:.6f} | static-world {r[1]:.6f} ({r[1] / r[0]:.3f}, coverage {r[3]:.3f}) | with points {r[2]:.6f} "
                          f"({r[2] / r[0]:.3f}, coverage {r[4]:.3f})")
        for k in range(n_frames):
            log(f"  {label} frame {k:2d}: " + line(rows[k]) + f"   [{rows[k][5]:.4f} of the pixels]")
        log(f"  {label} mean of frames {n_frames // 2} .. {n_frames - 1}: " + line(np.array([r[:5] for r in rows[n_frames // 2:]]).mean(axis=0)))
    gpu.set_mesh_instances(None)
    gpu.set_triangles(None)


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
