#!/usr/bin/env python3
"""The numbers of the neighbourhood colour bounds and the bounded accumulation for DESIGN.md 8h and profiles/history_clamp.log.

  timings  at 1920 x 1080, device tensors, filter_ms (hipEvent), median of `repeats` calls after a warm-up, in one run: the bounds kernel per
           radius under RTW_OPT_ATROUS_LAYOUT 1 (tile) and 2 (direct), with and without same_object and out_clamped, and its share of the HBM
           floor of the bytes it moves; one a-trous level and variance_estimate, which it is priced against; temporal_accumulate through the
           _points call and through the _bounded call on the same inputs under a static and a moved camera.
  parent   (--parent-tree PATH) scripts/measure_deform_motion.py's A/B: surface_map's kernel_ms, the existing temporal call's filter_ms and
           bench.py --gpus 1 through a built checkout of the parent commit at PATH and through this tree, alternating, a child process each.
  quality  (--quality) the recorded sequences, 4 spp, the same seeds and references as the scripts that recorded them: the Book-1 orbit and
           static camera and the light scene's light-biased orbit (scripts/measure_temporal.py), the six moving icospheres
           (scripts/measure_temporal_motion.py), the waving sheet (scripts/measure_deform_motion.py); MSE of the accumulated colour as a
           ratio to the single frame's: as recorded, firefly alone, history_clamp alone, both; radius {1, 2, 3} x k {0.5, 1, 2, 4, 8}; the share of pixels with out_clipped > 0.

    python scripts/measure_history_clamp.py [repeats] [--quality] [--parent-tree PATH [--rounds N]] [--out profiles/history_clamp.log]
"""
import itertools
import os
import sys

import numpy as np

try:                                                   # before the first rtw call: the library then shares the HIP runtime torch loaded (tests/conftest.py)
    import torch
except Exception:                                      # (only the timings need it)
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import rtw_amd as R                                    # noqa: E402
import measure_deform_motion as MD                     # noqa: E402  (its log, its parent A/B, its sheet)
from tests.temporal_common import orbit                # noqa: E402

W, H = 1920, 1080
OFFSET = (0.5, 0.5)
RADII, KS = (1, 2, 3), (0.5, 1.0, 2.0, 4.0, 8.0)
HBM_GBS = 8000.0                                       # MI355X peak HBM3E bandwidth, GB/s: the floor below is bytes / this
log = MD.log


def timings(gpu, reps):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    rng = np.random.default_rng(9)
    cam0 = MD.book1_camera(W, H)
    cam1 = orbit(cam0, 0.5)
    gpu.set_scene(R.Scene.generate(R.SCENE_C2))
    smap = lambda c: gpu.surface_map(c, W, H, MD.MINT, MD.MAXT, R.INTEGRATOR_GRADIENT, R.RAYS_PIXEL, OFFSET)
    g0, g1 = smap(cam0), smap(cam1)
    f0, f1 = (dev((rng.random((H, W, 3)) * 2.0).astype(np.float32)) for _ in range(2))
    kw = lambda g: dict(depth=dev(g["depth"]), normal=dev(g["normal"]), ids=dev(g["idx"]))
    k0, k1 = kw(g0), kw(g1)
    outs = [torch.empty((H, W, 3), device="cuda:0") for _ in range(3)]
    n_px = W * H
    log(f"# colour_bounds filter_ms at {W} x {H}, every buffer a device tensor: median of {reps} after a warm-up (min .. max), one run;")
    log(f"#   floor = the bytes the pass must move (12 in, 4 of idx with same_object, 24 out, 12 more with out_clamped, per pixel) at {HBM_GBS:.0f} GB/s")
    for radius in RADII:
        for same, clamped in ((False, False), (True, True)):
            floor_ms = n_px * (12 + (4 if same else 0) + 24 + (12 if clamped else 0)) / (HBM_GBS * 1e9) * 1e3
            for layout, name in ((1, "tile"), (2, "direct")):
                gpu.set_option(R.OPT_ATROUS_LAYOUT, layout)
                call = lambda: gpu.colour_bounds(f1, ids=k1["ids"], radius=radius, k=2.0, same_object=same, out_lo=outs[0], out_hi=outs[1],
                                                 out_clamped=outs[2] if clamped else None)[3].filter_ms
                t = MD.median_of(call, reps)
                log(f"  radius {radius}, same_object {int(same)}, out_clamped {int(clamped)}, {name}:".ljust(72) + MD.fmt(t)
                    + f"   floor {floor_ms:.4f} ms, {floor_ms / t[0]:.2f} of it reached")
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)
    log("# what it is priced against, in the same run (layout 0):")
    t = MD.median_of(lambda: gpu.atrous_filter(f1, levels=1, **k1)[1].filter_ms, reps)
    log("  atrous_filter, one level, every guide term:".ljust(72) + MD.fmt(t))
    hist = gpu.temporal_accumulate(f0, cam0, offset=OFFSET, **k0)[0]
    t = MD.median_of(lambda: gpu.variance_estimate(hist["moments"], hist["len"], **k0)[1].filter_ms, reps)
    log("  variance_estimate, radius 3, a first frame (every pixel takes the window):".ljust(72) + MD.fmt(t))
    log(f"# temporal_accumulate filter_ms at {W} x {H}, every term on (TEMPORAL_DEFAULTS), device tensors, the same inputs: _points against _bounded")
    lo, hi = gpu.colour_bounds(f1, radius=1, k=2.0)[:2]
    nan = torch.full((H, W, 3), float("nan"), device="cuda:0")
    clipped = torch.empty((H, W), device="cuda:0")
    for name, cam, k in (("static", cam0, k0), ("moved", cam1, k1)):
        base = dict(history=hist, offset=OFFSET, **k)
        for label, extra in (("existing call (rtw_ctx_temporal_accumulate)", {}), ("_points call, points on no pixel (all NaN)", dict(prev_point=nan)),
                             ("_bounded call, bounds", dict(hist_lo=lo, hist_hi=hi)),
                             ("_bounded call, bounds and out_clipped", dict(hist_lo=lo, hist_hi=hi, out_clipped=clipped))):
            t = MD.median_of(lambda: gpu.temporal_accumulate(f1, cam, **base, **extra)[2].filter_ms, reps)
            log(f"  {name} camera, {label}:".ljust(72) + MD.fmt(t))


# ---- quality -------------------------------------------------------------------------------------------------------------------------------
def evaluate(gpu, seq, prm, firefly=None, clamp=None):
    """seq: per frame (cur, cam, guides, extra temporal arguments, truth, mask or None).  Per frame (MSE single, MSE accumulated, share of
    the pixels with out_clipped > 0), on the mask's pixels."""
    hist, rows = None, []
    for cur, cam, g, extra, truth, mask in seq:
        frame, kw = cur, {}
        if firefly:
            frame = gpu.colour_bounds(cur, exclude_centre=True, out_clamped=True, **firefly)[2]
        if clamp:
            lo, hi = gpu.colour_bounds(frame, **clamp)[:2]
            kw = dict(hist_lo=lo, hist_hi=hi, out_clipped=True)
        hist, _, _ = gpu.temporal_accumulate(frame, cam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist, offset=OFFSET, **extra(hist is None),
                                             **kw, **prm)
        m = mask if mask is not None else np.ones(cur.shape[:2], bool)
        mse = lambda img: float(((np.asarray(img, np.float64) - truth) ** 2)[m].mean())
        rows.append((mse(cur), mse(hist["color"]), float((hist["clipped"] > 0)[m].mean()) if clamp else 0.0))
    return rows


def late(rows):
    m = np.array(rows[len(rows) // 2:]).mean(axis=0)
    return m[1] / m[0], m[2]


def book_and_lights(gpu):
    """The Book-1 orbit and static camera and the light scene's orbit exactly as scripts/measure_temporal.py builds them."""
    from tests import lights_common as LC
    from tests.test_oracle_golden import small_view
    w, h, n_frames, step = 400, 225, 16, 0.25
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)

    def render(c, samples, seed):
        p.samples, p.seed = samples, seed
        return gpu.render(c, p)[0]

    none = lambda first: {}
    seqs = {}
    for label, deg in (("book1 orbit", step), ("book1 static", 0.0)):
        cams = [orbit(cam, deg * k) for k in range(n_frames)]
        truths = [render(c, 4096, 1).astype(np.float64) for c in (cams if deg else cams[:1])] * (1 if deg else n_frames)
        seqs[label] = [(render(c, 4, 100 + k), c, gpu.surface_map(c, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, OFFSET), none, t, None)
                       for k, (c, t) in enumerate(zip(cams, truths))]
    ls, g = LC.golden()
    w, h = 400, 300
    lcam = LC.camera_no_rand(g, w, h)
    gpu.set_scene(ls.scene)
    gpu.set_lights(ls.lights, ls.weight)
    integ, depth = R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"]

    def lrender(c, samples, seed):
        lp = ls.params(w, h, integ, depth, seed=seed, sampler=R.SAMPLER_ROW, samples=samples, gamma=1.0, mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
        return gpu.render(c, lp)[0]

    cams = [orbit(lcam, step * k) for k in range(n_frames)]
    seqs["lights orbit"] = [(lrender(c, 4, 100 + k), c, gpu.surface_map(c, w, h, g["mint"], g["maxt"], integ, R.RAYS_PIXEL, OFFSET), none,
                             lrender(c, 4096, 2).astype(np.float64), None) for k, c in enumerate(cams)]
    gpu.set_lights(None)
    return seqs


def sheet_orbit(gpu):
    """The waving sheet under the orbit exactly as scripts/measure_deform_motion.py's quality() builds it; MSE on the sheet's pixels."""
    w, h, n_frames, step, truth_spp = 400, 225, 12, 0.25, 1024
    eye = np.array([13.0, 2.0, 3.0])
    vp = R.Viewport.new_from_res(w, h, 4, 8, 1.0, vfov=20.0, origin=tuple(eye), direction=tuple(-eye / np.linalg.norm(eye)), vup=(0.0, 1.0, 0.0))
    cam = vp.camera()
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = w, h, 4, 8, 1.0
    p.mint, p.maxt = MD.MINT, MD.MAXT
    p.integrator, p.sampler, p.accel, p.flags = R.INTEGRATOR_RUST2, R.SAMPLER_ROW, R.ACCEL_BVH, 0
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    spheres = [R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), R.SCATTER_M), R.Sphere.new((-3.0, 1.0, -2.5), 1.0, (0.7, 0.3, 0.3), R.SCATTER_M),
               R.Sphere.new((-4.0, 1.0, 1.0), 1.0, (0.3, 0.4, 0.7), R.SCATTER_M), R.Sphere.new((-3.0, 1.0, 4.0), 1.0, (0.7, 0.6, 0.5), R.SCATTER_M)]
    gpu.set_scene(R.Scene(spheres, background=(0.7, 0.8, 1.0)))
    shape = lambda k: MD.sheet(24, 0.35 * k)
    v, f = shape(0)
    gpu.set_triangles(R.Triangle.from_mesh(v, f, color=(0.8, 0.7, 0.2)))
    gpu.set_mesh_instances([(MD.pose(0)[0, :3], MD.pose(0)[0, 3:])])
    first = gpu.mesh_instance_first()

    def render(c, samples, seed):
        p.samples, p.seed = samples, seed
        return gpu.render(c, p)[0]

    seq, prev_ouv = [], None
    for k in range(n_frames):
        c = orbit(cam, step * k)
        ouv = R.mesh_ouv(shape(k)[0], f)
        gpu.move_mesh_instances(MD.pose(k), ouv)
        truth = render(c, truth_spp, 1).astype(np.float64)
        cur = render(c, 4, 100 + k)
        g = gpu.surface_map(c, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, OFFSET, tri=True, bary=True)
        points = {}
        if k:
            pt, cn = gpu.deform_motion(g["tri"], g["bary"], prev_ouv, g["idx"], MD.pose(k - 1), first)
            points = dict(prev_point=pt, carried_normal=cn)
        prev_ouv = ouv
        seq.append((cur, c, g, (lambda first_frame, q=points: {} if first_frame else q), truth, g["tri"] >= 0))
    gpu.set_mesh_instances(None)
    gpu.set_triangles(None)
    return {"sheet orbit (the sheet's pixels)": seq}


def icospheres_orbit(gpu):
    """The six moving icospheres under the orbit exactly as scripts/measure_temporal_motion.py's quality() builds them; MSE on the moving
    objects' pixels."""
    w, h, n_frames, step = 400, 225, 16, 0.25
    eye = np.array([13.0, 2.0, 3.0])
    vp = R.Viewport.new_from_res(w, h, 4, 8, 1.0, vfov=20.0, origin=tuple(eye), direction=tuple(-eye / np.linalg.norm(eye)), vup=(0.0, 1.0, 0.0))
    cam = vp.camera()
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = w, h, 4, 8, 1.0
    p.mint, p.maxt = MD.MINT, MD.MAXT
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

    seq = []
    for k in range(n_frames):
        c = orbit(cam, step * k)
        gpu.move_mesh_instances(poses(k))
        truth = render(c, 4096, 1).astype(np.float64)
        cur = render(c, 4, 100 + k)
        g = gpu.surface_map(c, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, OFFSET)
        motion = {} if k == 0 else dict(motion=gpu.mesh_instance_motion(poses(k - 1), poses(k))[0], motion_first=first)
        seq.append((cur, c, g, (lambda first_frame, q=motion: {} if first_frame else q), truth, g["idx"] >= first))
    gpu.set_mesh_instances(None)
    gpu.set_triangles(None)
    return {"icospheres orbit (the moving objects' pixels)": seq}


def quality(gpu):
    prm = dict(R.TEMPORAL_DEFAULTS)
    seqs = book_and_lights(gpu)
    seqs.update(icospheres_orbit(gpu))
    seqs.update(sheet_orbit(gpu))
    log(f"# quality: the accumulated colour's MSE over the late frames (the second half) as a ratio to the single frames', TEMPORAL_DEFAULTS {prm};")
    log("#   references, seeds and sequences as scripts/measure_temporal.py (Book-1 final scene 400 x 225 and the light scene 400 x 300, 16 frames,")
    log("#   4096-spp references) and scripts/measure_deform_motion.py (the waving sheet, 12 frames, 1024-spp references, the sheet's pixels)")
    log("#   and scripts/measure_temporal_motion.py (six moving icospheres, 16 frames, 4096-spp references, the moving objects' pixels)")
    names = list(seqs)
    for n in names:
        rows = evaluate(gpu, seqs[n], prm)
        log(f"  as recorded, {n}: " + "  ".join(f"{k}: {r[1] / r[0]:.3f}" for k, r in enumerate(rows)) + f"   late frames {late(rows)[0]:.3f}")
    log("# columns per sequence: firefly alone | history_clamp alone (share of pixels clipped) | both (share clipped); same_object off")
    best = None
    for radius, k in itertools.product(RADII, KS):
        b = dict(radius=radius, k=k)
        cells, both = [], []
        for n in names:
            f_, c_, fc = (late(evaluate(gpu, seqs[n], prm, **kw)) for kw in (dict(firefly=b), dict(clamp=b), dict(firefly=b, clamp=b)))
            cells.append(f"{n}: {f_[0]:.3f} | {c_[0]:.3f} ({c_[1]:.3f}) | {fc[0]:.3f} ({fc[1]:.3f})")
            both.append(fc[0])
        mean = float(np.mean(both))
        log(f"  radius {radius} k {k:3.1f}   " + "   ".join(cells) + f"   mean of both {mean:.3f}")
        if best is None or mean < best[0]:
            best = (mean, radius, k)
    log(f"# the row with the least mean ratio of the column `both` over the sequences: radius {best[1]} k {best[2]} ({best[0]:.3f})")
    base = float(np.mean([late(evaluate(gpu, seqs[n], prm))[0] for n in names]))
    log(f"# the same mean as recorded (no firefly, no history_clamp): {base:.3f}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0])) if args and args[0].isdigit() else 9
    if "--out" in sys.argv:
        MD.OUT[0] = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(MD.OUT[0])), exist_ok=True)
        open(MD.OUT[0], "w").close()
    if "--parent-tree" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 2
        MD.parent_ab(sys.argv[sys.argv.index("--parent-tree") + 1], rounds)
    with R.Renderer(0) as gpu:
        if "--no-timings" not in sys.argv:
            timings(gpu, reps)
        if "--quality" in sys.argv:
            quality(gpu)


if __name__ == "__main__":
    main()
