#!/usr/bin/env python3
"""Mesh placements, measured: writes profiles/mesh_instances.log.

    python scripts/measure_mesh_instances.py            on the new tree: everything below
    python scripts/measure_mesh_instances.py --parent   on the parent commit (no placements there): the SPEC 8 yardstick alone

480 x 270, 4 spp, depth 6, RTW_INTEGRATOR_RUST2, RTW_ACCEL_BVH, as DESIGN.md 4.5's table.  One warm-up render, then the median of RUNS
kernel times (RtwStats.kernel_ms) with min - max.
  1. the transform's price: the 20k terrain through ONE identity placement (SPEC 12) against the same mesh as plain triangles (SPEC 8)
  2. scaling: the terrain placed 1, 4, 16, 64 times on a grid; ms, node visits and triangle tests per segment; beside it the same world
     geometry flattened on the host into one triangle list (SPEC 8).  The cost of one missed placement is the slope of ms per segment over
     the placement count between 16 and 64 (nearly every ray misses nearly every placement there)."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R  # noqa: E402

W, H, SPP, DEPTH, RUNS = 480, 270, 4, 6, 9
SIDE, SIZE = 100, 20.0                                           # 2 * 100^2 = 20k triangles over 20 x 20


def params():
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth = W, H, SPP, DEPTH
    p.gamma, p.mint, p.maxt = 1.0, 1e-3, 1e4
    p.integrator, p.sampler, p.accel = R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, R.ACCEL_BVH
    p.seed = 1
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    return p


def timed(gpu, cam, p):
    gpu.render(cam, p)                                           # warm-up
    ms, st = [], None
    for _ in range(RUNS):
        _, st = gpu.render(cam, p)
        ms.append(st.kernel_ms)
    return statistics.median(ms), min(ms), max(ms), st


def line(name, r):
    med, lo, hi, st = r
    return (f"{name:<44} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {1e6 * med / st.segments:7.3f} ns/segment  {st.segments:9d} segments  "
            f"{st.node_tests / st.segments:8.2f} node visits  {st.quad_tests / st.segments:7.2f} triangle tests per segment")


def main():
    parent = "--parent" in sys.argv
    out = [f"mesh placements: {W} x {H}, {SPP} spp, depth {DEPTH}, RUST2, BVH; warm-up + median of {RUNS} (min - max); kernel_ms"
           + ("  [PARENT COMMIT]" if parent else "")]
    vtx, faces = R.mesh_terrain(SIDE, SIZE, 1.0, seed=3)
    scene = R.Scene([R.Sphere.new((0.0, 3.0, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M)], background=(0.6, 0.7, 0.9))
    p = params()
    with R.Renderer(0) as gpu:
        def grid(n):
            side = int(round(n ** 0.5))
            return [((SIZE * (i - (side - 1) / 2), 0.0, SIZE * (j - (side - 1) / 2)), (1.0, 0.0, 0.0, 0.0)) for j in range(side) for i in range(side)]

        def camera(n):
            reach = SIZE * max(1.0, n ** 0.5)
            return R.camera2_new(W / H, (0.0, 0.45 * reach, -0.75 * reach), (0.0, 1.0, 0.0), (0.0, -0.5, 1.0), 50.0, 0.0)

        gpu.set_scene(scene)
        gpu.set_triangles(R.Triangle.from_mesh(vtx, faces))
        plain = timed(gpu, camera(1), p)
        out.append(line("20k terrain, plain triangles (SPEC 8)", plain))
        if not parent:
            gpu.set_mesh_instances(grid(1))
            one = timed(gpu, camera(1), p)
            out.append(line("20k terrain, one identity placement (SPEC 12)", one))
            out.append(f"the transform's price: {one[0] / plain[0]:.3f} x the plain build in this run")
            per_seg = {}
            for n in (1, 4, 16, 64):
                gpu.set_triangles(R.Triangle.from_mesh(vtx, faces))
                gpu.set_mesh_instances(grid(n))
                r = timed(gpu, camera(n), p)
                per_seg[n] = 1e6 * r[0] / r[3].segments
                out.append(line(f"placed {n:2d} x (SPEC 12)", r))
            out.append(f"one missed placement: {(per_seg[64] - per_seg[16]) / 48:.4f} ns per segment and placement (slope between 16 and 64)")
        for n in (1, 4, 16, 64):
            flat = np.concatenate([vtx + np.asarray(pos, np.float32)[None] for pos, _ in grid(n)])
            ff = np.concatenate([faces + k * len(vtx) for k in range(n)])
            gpu.set_triangles(R.Triangle.from_mesh(flat, ff))
            out.append(line(f"flattened {n:2d} x = {len(ff)} triangles (SPEC 8)", timed(gpu, camera(n), p)))
    text = "\n".join(out) + "\n"
    print(text, end="")
    dst = os.path.join(ROOT, "profiles", "mesh_instances_parent.log" if parent else "mesh_instances.log")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    open(dst, "w").write(text)


if __name__ == "__main__":
    main()
