#!/usr/bin/env python3
"""The any-hit pass against the closest-hit query, measured: writes profiles/occluded.log.  One MI355X.

    python scripts/measure_occluded.py [--out FILE]

The yardstick is rtw_ctx_scene_hits on the same context with the same device-resident rays and no normals.  The two calls alternate in one
process: a warm-up of each, then the median of RUNS with min - max; RtwStats.kernel_ms.  The counters are deterministic and reported beside
the times.  Every answer is checked: occluded == (index >= 0).

  (a) the 1920 x 1080 depth_rays of the Book-1 final scene (485 spheres), under both accels
  (b) shadow rays in the golden light scene plus the 60 spheres of scripts/measure_lights.py: segments from the primary hit points of a
      400 x 300 depth_map to each light's rtw_light_mid, formed with segments_occluded
  (c) the 200k-triangle terrain from the camera of scripts/measure_refit.py, 1920 x 1080
  (d) 1024 placements of the 20k terrain (the grid of scripts/measure_mesh_top.py) through the top-level tree, 1920 x 1080"""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import rtw_amd as R                      # noqa: E402
from tests import lights_common as LC    # noqa: E402

RUNS = 9
W, H = 1920, 1080
DEV = "cuda:0"


def pair(gpu, rays, mint, maxt, accel):
    """rays: a device tensor [n][6].  ((median, min, max, stats) of scene_hits, the same of scene_occluded, the share of occluded rays)."""
    n = rays.shape[0]
    t = torch.empty(n, dtype=torch.float32, device=DEV)
    idx = torch.empty(n, dtype=torch.int32, device=DEV)
    occ = torch.empty(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()

    def hits():
        st = R.RtwStats()
        rc = R.lib().rtw_ctx_scene_hits(gpu._h, rays.data_ptr(), n, 0.0, mint, maxt, accel, t.data_ptr(), idx.data_ptr(), None, C.byref(st))
        assert rc == R.RTW_OK, rc
        return st

    def occluded():
        return gpu.scene_occluded(rays, mint, maxt, accel=accel, out=occ)[1]
    hits(), occluded()
    assert torch.equal(occ.bool(), idx >= 0), "occluded != (index >= 0)"
    ms = {"hits": [], "occluded": []}
    last = {}
    for _ in range(RUNS):
        for name, call in (("hits", hits), ("occluded", occluded)):
            st = call()
            ms[name].append(st.kernel_ms)
            last[name] = st
    res = [(statistics.median(ms[k]), min(ms[k]), max(ms[k]), last[k]) for k in ("hits", "occluded")]
    return res[0], res[1], float(occ.float().mean())


def lines(name, n, res):
    h, o, share = res
    out = [f"{name}: {n} rays, {share:.1%} occluded"]
    for label, (med, lo, hi, st) in (("scene_hits", h), ("scene_occluded", o)):
        out.append(f"  {label:<15} {med:9.3f} ms ({lo:.3f} - {hi:.3f})  {1e6 * med / n:8.3f} ns/ray  sphere tests {st.sphere_tests / n:9.2f}  "
                   f"node visits {st.node_tests / n:8.2f}  quad + triangle tests {st.quad_tests / n:8.2f} per ray")
    spread = h[2] - h[1]
    verdict = "not slower" if o[0] <= h[0] + spread else "SLOWER than scene_hits by more than its min-max spread"
    out.append(f"  occluded / hits {o[0] / h[0]:.3f}  (scene_hits' spread {spread:.3f} ms: {verdict}); sphere tests x {ratio(o[3].sphere_tests, h[3].sphere_tests)}, "
               f"node visits x {ratio(o[3].node_tests, h[3].node_tests)}, quad + triangle tests x {ratio(o[3].quad_tests, h[3].quad_tests)}")
    return out


def ratio(a, b):
    return f"{a / b:.3f}" if b else "-"


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    torch.cuda.synchronize()
    return t


def main():
    out = [f"any-hit pass (scene_occluded) against the closest-hit query (scene_hits, no normals): the same context, the same device-resident rays, "
           f"alternating; warm-up + median of {RUNS} (min - max); kernel_ms"]
    with R.Renderer(0) as gpu:
        # (a) Book 1
        gpu.set_scene(R.Scene.generate(R.SCENE_C2))
        rays = device(R.depth_rays(R.camera2_new(W / H, (13.0, 2.0, 3.0), (0.0, 1.0, 0.0), (-13.0, -2.0, -3.0), 20.0, 0.0), W, H))
        for accel, label in ((R.ACCEL_BVH, "BVH"), (R.ACCEL_BRUTE, "BRUTE")):
            out += lines(f"(a) Book-1 final scene, 485 spheres, depth rays {W} x {H}, {label}", len(rays), pair(gpu, rays, 1e-3, 1e3, accel))
        # (b) shadow rays of the golden light scene + 60 spheres
        ls, g = LC.golden()
        field = LC.LightScene(LC.sphere_field(g), g["quads"], ls.lights, g["background"], weight=g["biased_weight"])
        gpu.set_scene(field.scene)
        cam = LC.camera(g, 400, 300)
        prim = R.depth_rays(cam, 400, 300)
        depth, ids, _ = gpu.depth_map(cam, 400, 300, g["mint"], g["maxt"], ids=True)
        hit = ids.reshape(-1) >= 0
        p = (prim[hit, :3] + prim[hit, 3:] * depth.reshape(-1)[hit, None]).astype(np.float32)
        mids = [R.light_mid(field.scene, light) for light in field.lights]
        tp = device(np.concatenate([p] * len(mids)))
        tq = device(np.concatenate([np.broadcast_to(m, p.shape) for m in mids]))
        gpu.use_torch_stream()
        seg_occ, _ = gpu.segments_occluded(tp, tq)
        rays = torch.cat([tp, tq - tp], 1).contiguous()
        torch.cuda.synchronize()
        gpu.set_stream(0)
        lo, hi = 1e-3, 1.0 - 1e-3
        for accel, label in ((R.ACCEL_BVH, "BVH"), (R.ACCEL_BRUTE, "BRUTE")):
            res = pair(gpu, rays, lo, hi, accel)
            assert torch.equal(seg_occ, gpu.scene_occluded(rays, lo, hi, accel=accel)[0]), "segments_occluded != scene_occluded of its rays"
            out += lines(f"(b) golden light scene + 60 spheres, {len(mids)} light(s) x {len(p)} primary hit points of a 400 x 300 depth_map, {label}", len(rays), res)
        # (c) the 200k terrain
        vtx, faces = R.mesh_terrain(317, seed=2)
        gpu.set_scene(R.Scene((), triangles=R.Triangle.from_mesh(vtx, faces)))
        blo, bhi = vtx.min(axis=0), vtx.max(axis=0)
        c, ext = (blo + bhi) / 2, float((bhi - blo).max())
        cam = R.camera2_new(W / H, (float(c[0]), float(c[1] + 0.6 * ext), float(c[2] - 0.9 * ext)), (0.0, 1.0, 0.0), (0.0, -0.55, 0.83), 50.0, 0.0)
        rays = device(R.depth_rays(cam, W, H))
        out += lines(f"(c) terrain, {len(faces)} triangles, depth rays {W} x {H}, BVH", len(rays), pair(gpu, rays, 1e-3, 1e4, R.ACCEL_BVH))
        # (d) 1024 placements of the 20k terrain
        size, n = 20.0, 1024
        vtx, faces = R.mesh_terrain(100, size, 1.0, seed=3)
        side = int(round(n ** 0.5))
        grid = [((size * (i - (side - 1) / 2), 0.0, size * (j - (side - 1) / 2)), (1.0, 0.0, 0.0, 0.0)) for j in range(side) for i in range(side)]
        gpu.set_scene(R.Scene(()))
        gpu.set_triangles(R.Triangle.from_mesh(vtx, faces))
        gpu.set_mesh_instances(grid)
        gpu.set_option(R.OPT_MESH_LIST_MAX, 0)
        reach = size * n ** 0.5
        cam = R.camera2_new(W / H, (0.0, 0.45 * reach, -0.75 * reach), (0.0, 1.0, 0.0), (0.0, -0.5, 1.0), 50.0, 0.0)
        rays = device(R.depth_rays(cam, W, H))
        out += lines(f"(d) {n} placements of the {len(faces)}-triangle terrain, top-level tree, depth rays {W} x {H}, BVH", len(rays),
                     pair(gpu, rays, 1e-3, 1e4, R.ACCEL_BVH))
        gpu.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)
    text = "\n".join(out) + "\n"
    print(text, end="")
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "profiles", "occluded.log")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    open(dst, "w").write(text)


if __name__ == "__main__":
    main()
