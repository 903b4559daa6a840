#!/usr/bin/env python3
"""Rust2 triangle meshes on the GPU: the triangle tree (RTW_ACCEL_BVH) against the triangle list walk (RTW_ACCEL_BRUTE) on the same frames.

    python scripts/gpu_triangle_mesh.py [--out LOG] [--reps N]

Scenes (procedural, rtw_amd.mesh_icosphere / mesh_terrain): a subdivided icosphere (levels 2..5) over a ground sphere, and a height-field
terrain of ~2k, ~20k and ~200k triangles with a few spheres and a quad light (RTW_INTEGRATOR_BG_COLOR).  For each scene and strategy:
ms per frame (kernel time, median of --reps), G segments/s, triangle tests and triangle-tree node visits per segment.  Both images must be
identical bit for bit (the script fails otherwise).  The resource lines of the triangle build (csrc/build/resource_usage.txt of
`make asm`) are appended when that file exists.
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R  # noqa: E402


def camera(w, h, origin, target):
    d = tuple(float(t - o) for t, o in zip(target, origin))
    return R.Viewport.new_from_res(w, h, 1, 4, 1.0, vfov=45.0, origin=origin, direction=d, vup=(0.0, 1.0, 0.0)).camera()


def icosphere_scene(level):
    v, f = R.mesh_icosphere(level, (0.0, 1.0, 0.0), 1.0)
    tris = R.Triangle.from_mesh(v, f, mat=R.SCATTER_M, color=(0.7, 0.4, 0.3))
    sph = [R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5))]
    quads = [R.Quad.new((-2, 5, -2), (4, 0, 0), (0, 0, 4), R.SCATTER_M, (1, 1, 1), emitted=(6, 6, 6))]
    return R.Scene(sph, background=(0.2, 0.25, 0.3), quads=quads, triangles=tris), (0.0, 2.0, 4.5), (0.0, 1.0, 0.0)


def terrain_scene(n_side):
    v, f = R.mesh_terrain(n_side, 20.0, 1.5, 7)
    tris = R.Triangle.from_mesh(v, f, mat=R.SCATTER_M, color=(0.45, 0.5, 0.3))
    sph = [R.Sphere.new((-2.0, 2.0, 0.0), 1.0, (0.8, 0.8, 0.8), R.METALLIC_M), R.Sphere.new((1.5, 2.0, 1.0), 1.0, (1, 1, 1), R.GLASS_M),
           R.Sphere.new((3.0, 1.8, -2.0), 0.8, (0.7, 0.3, 0.3))]
    quads = [R.Quad.new((-3, 8, -3), (6, 0, 0), (0, 0, 6), R.SCATTER_M, (1, 1, 1), emitted=(5, 5, 5))]
    return R.Scene(sph, background=(0.35, 0.4, 0.5), quads=quads, triangles=tris), (0.0, 6.0, 12.0), (0.0, 0.5, 0.0)


def measure(r, cam, p, accel, reps):
    p.accel = accel
    img, st = r.render(cam, p)                       # warm-up (and the image)
    ms = []
    for _ in range(reps):
        _, s = r.render(cam, p)
        ms.append(s.kernel_ms)
    return img, st, float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--spp", type=int, default=4)
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# Rust2 triangle meshes, {a.width}x{a.height}, {a.spp} spp, depth 6, RTW_INTEGRATOR_BG_COLOR, render_row sampler; "
        f"kernel ms = median of {a.reps} after one warm-up  ({time.strftime('%Y-%m-%d %H:%M:%S')})")
    log(f"{'scene':<22}{'tris':>8}  {'accel':<6}{'ms/frame':>10}{'Gseg/s':>9}{'tri tests/seg':>15}{'nodes/seg':>11}{'BRUTE/BVH':>11}")
    scenes = [("icosphere L2", lambda: icosphere_scene(2)), ("icosphere L3", lambda: icosphere_scene(3)),
              ("icosphere L4", lambda: icosphere_scene(4)), ("icosphere L5", lambda: icosphere_scene(5)),
              ("terrain 2k", lambda: terrain_scene(32)), ("terrain 20k", lambda: terrain_scene(100)),
              ("terrain 200k", lambda: terrain_scene(317))]
    results = {}
    with R.Renderer(0) as r:
        for name, make in scenes:
            scene, eye, target = make()
            cam = camera(a.width, a.height, eye, target)
            p = R.RtwParams()
            p.width, p.height, p.samples, p.depth, p.gamma = a.width, a.height, a.spp, 6, 1.0
            p.mint, p.maxt = 0.001, 1e4
            p.integrator, p.sampler, p.seed = R.INTEGRATOR_BG_COLOR, R.SAMPLER_ROW, 5
            r.set_scene(scene)
            img_b, st_b, ms_b = measure(r, cam, p, R.ACCEL_BVH, a.reps)
            img_l, st_l, ms_l = measure(r, cam, p, R.ACCEL_BRUTE, a.reps)
            if not np.array_equal(img_b.view(np.uint32), img_l.view(np.uint32)):
                log(f"{name}: TREE AND LIST IMAGES DIFFER")
                sys.exit(1)
            for acc, st, ms in (("BVH", st_b, ms_b), ("BRUTE", st_l, ms_l)):
                seg = max(1, st.segments)
                ratio = f"{ms_l / ms_b:10.1f}x" if acc == "BVH" else ""
                log(f"{name:<22}{scene.n_triangles:>8}  {acc:<6}{ms:>10.2f}{st.segments / ms / 1e6:>9.3f}{st.quad_tests / seg:>15.1f}"
                    f"{st.node_tests / seg:>11.1f}{ratio:>11}")
            results[name] = (ms_b, ms_l)
    if "terrain 2k" in results and "terrain 200k" in results:
        log(f"# terrain 200k / 2k, BVH ms per frame: {results['terrain 200k'][0] / results['terrain 2k'][0]:.2f}x; "
            f"200k BRUTE / BVH: {results['terrain 200k'][1] / results['terrain 200k'][0]:.1f}x; images of tree and list identical in every row")
    res = os.path.join(ROOT, "raytracing-in-a-weekend_amd", "csrc", "build", "resource_usage.txt")
    if os.path.exists(res):
        log("# resource usage of the triangle build (SPEC 8) and the query kernel (make asm):")
        text = open(res).read()
        for fn in dict.fromkeys(re.findall(r"Function Name: (\S*(?:Li8ELb1E|tri_hits)\S*)", text)):
            blk = text[text.index(fn):].split("Function Name:")[0]
            keep = [re.sub(r".*:\d+:\d+:\s*|\s*\[-Rpass.*", "", x) for x in blk.splitlines() if re.search(r"VGPRs:|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill", x)]
            log(f"#   {fn}: " + "; ".join(keep))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
