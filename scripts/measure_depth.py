#!/usr/bin/env python3
"""Speed of the depth pass (rtw_ctx_depth_map): a 1920 x 1080 map with ids and normals off, then with both on, for the Book-1 final scene
under RTW_ACCEL_BVH and under RTW_ACCEL_BRUTE and for the 200k-triangle terrain of scripts/gpu_triangle_mesh.py through its tree --
against the only other way to a primary-hit image: rtw_ctx_render of the same view with RTW_INTEGRATOR_NORMAL, RTW_SAMPLER_NO_RAND,
depth 1, in the same run.  Every figure is kernel time (RtwStats.kernel_ms): the best of `repeats` after a warm-up, with the spread
(max - min) of the repeats next to it.

    python scripts/measure_depth.py [repeats] [--out profiles/depth_map.log]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtw_amd as R                                   # noqa: E402
from scripts.gpu_triangle_mesh import terrain_scene   # noqa: E402

W, H = 1920, 1080
MINT, MAXT = 0.001, 1000.0


def best(fn, reps):
    fn()                                              # warm-up
    ms = [fn() for _ in range(reps)]
    return min(ms), max(ms) - min(ms)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0])) if args else 7
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    book1 = R.Scene.generate(R.SCENE_C2)
    terrain, t_origin, t_target = terrain_scene(317)
    views = [("Book-1 final scene, %d spheres" % book1.n_spheres, book1, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, (R.ACCEL_BVH, R.ACCEL_BRUTE)),
             ("terrain, %d triangles" % terrain.n_triangles, terrain, t_origin, t_target, 45.0, (R.ACCEL_BVH,))]
    log(f"# depth map {W} x {H}, kernel ms: best of {reps} after a warm-up (spread = max - min of the repeats)")
    with R.Renderer(0) as gpu:
        for name, scene, origin, target, vfov, accels in views:
            d = np.array([float(t - o) for t, o in zip(target, origin)])
            d = tuple(float(x) for x in d / np.linalg.norm(d))           # a UNIT view direction: both cameras then span the same field of view
            cam2 = R.camera2_new(W / H, origin, (0.0, 1.0, 0.0), d, vfov, 0.0)
            vp = R.Viewport.new_from_res(W, H, 1, 1, 1.0, vfov=vfov, origin=origin, direction=d, vup=(0.0, 1.0, 0.0))
            gpu.set_scene(scene)
            for accel in accels:
                label = "RTW_ACCEL_BVH" if accel == R.ACCEL_BVH else "RTW_ACCEL_BRUTE"
                p = vp.params(R.INTEGRATOR_NORMAL, R.SAMPLER_NO_RAND, accel)
                p.mint, p.maxt = MINT, MAXT
                r_ms, r_sp = best(lambda: gpu.render(vp.camera(), p)[1].kernel_ms, reps)
                d_ms, d_sp = best(lambda: gpu.depth_map(cam2, W, H, MINT, MAXT, accel=accel)[-1].kernel_ms, reps)
                f_ms, f_sp = best(lambda: gpu.depth_map(cam2, W, H, MINT, MAXT, accel=accel, ids=True, normals=True)[-1].kernel_ms, reps)
                st = gpu.depth_map(cam2, W, H, MINT, MAXT, accel=accel)[-1]
                rst = gpu.render(vp.camera(), p)[1]
                margin = max(r_sp, d_sp)
                verdict = "not slower" if d_ms <= r_ms + margin else "SLOWER"
                log(f"{name}, {label}")
                log(f"  render (NORMAL, NO_RAND, depth 1)   {r_ms:8.3f} ms  spread {r_sp:.3f}")
                log(f"  depth_map                          {d_ms:8.3f} ms  spread {d_sp:.3f}   {verdict} than the render (margin {margin:.3f} ms)")
                log(f"  depth_map + ids + normals          {f_ms:8.3f} ms  spread {f_sp:.3f}")
                log(f"  per map:    {st.sphere_tests} sphere tests, {st.node_tests} node visits, {st.quad_tests} quad / triangle tests")
                log(f"  per render: {rst.sphere_tests} sphere tests, {rst.node_tests} node visits, {rst.quad_tests} quad / triangle tests")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
