#!/usr/bin/env python3
"""Ambient occlusion, fused, against the any-hit pass over stored rays, measured: writes profiles/ao.log.  One MI355X.

    python scripts/measure_ao.py [--only a|c|d] [--out FILE]

Each workload runs as ao_map at 1920 x 1080 with 16 samples and at 480 x 270 with 64, the radius a tenth of the scene's extent.  The
yardstick is the code as it stood before the fused kernel: rtw_ctx_scene_occluded on the same rays, made beforehand by ao_rays from the
map's own points and faced normals and resident on the device (24 bytes per ray read, one byte per ray written; making and uploading the
rays is not timed).  Against it stands rtw_ctx_ambient_occlusion on the same points, device tensors in and out: the two calls alternate
in one process, a warm-up of each, then the median of RUNS with min - max; RtwStats.kernel_ms.  ao_map (both launches) and depth_map are
timed the same way beside them.  Every answer is checked: the fused kernel's floats are (samples - c) / samples of the yardstick's bytes,
ao_map's are the same floats, and the counters are equal.

  (a) the Book-1 final scene (485 spheres)
  (c) the 200k-triangle terrain from the camera of scripts/measure_refit.py
  (d) 1024 placements of the 20k terrain (the grid of scripts/measure_mesh_top.py) through the top-level tree"""
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import rtw_amd as R                      # noqa: E402

RUNS = 9
DEV = "cuda:0"
F = np.float32
SIZES = ((1920, 1080, 16), (480, 270, 64))
AO_MINT = 1e-3


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()
    return t


def points_of(gpu, cam, w, h, mint, maxt):
    """ao_map's points and faced normals by its definition (numpy, one f32 rounding per operation); misses get the normal 0 0 0."""
    depth, ids, nrm, _ = gpu.depth_map(cam, w, h, mint, maxt, ids=True, normals=True)
    rays = R.depth_rays(cam, w, h)
    o, d = rays[:, :3], rays[:, 3:]
    t, hit, n = depth.reshape(-1), ids.reshape(-1) >= 0, nrm.reshape(-1, 3)
    p = (o + (d * t[:, None]).astype(F)).astype(F)
    dot = ((d[:, 0] * n[:, 0]).astype(F) + (d[:, 1] * n[:, 1]).astype(F)).astype(F) + (d[:, 2] * n[:, 2]).astype(F)
    faced = np.where((dot > 0.0)[:, None], -n, n).astype(F)
    faced[~hit] = 0.0
    p[~hit] = 0.0
    return p, faced, hit


def timed(calls):
    """calls: name -> a function that returns RtwStats.  Alternating, a warm-up of each, then RUNS of each: name -> (median, min, max, stats)."""
    for call in calls.values():
        call()
    ms, last = {k: [] for k in calls}, {}
    for _ in range(RUNS):
        for name, call in calls.items():
            st = call()
            ms[name].append(st.kernel_ms)
            last[name] = st
    return {k: (statistics.median(v), min(v), max(v), last[k]) for k, v in ms.items()}


def workload(gpu, name, cam, mint, maxt, extent):
    out = []
    radius = 0.1 * extent
    for w, h, samples in SIZES:
        p, faced, hit = points_of(gpu, cam, w, h, mint, maxt)
        n_hit = int(hit.sum())
        full = R.ao_rays(p, faced, samples, 0)                          # (ray [i][k] depends on i: made at the pixels' own indices)
        d_rays = device(full[hit].reshape(-1, 6))
        del full
        n_rays = n_hit * samples
        d_p, d_n = device(p), device(faced)
        d_occ = torch.empty(n_rays, dtype=torch.uint8, device=DEV)
        d_ao = torch.empty(len(p), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        res = timed({
            "scene_occluded": lambda: gpu.scene_occluded(d_rays, AO_MINT, radius, out=d_occ)[1],
            "ambient_occlusion": lambda: gpu.ambient_occlusion(d_p, d_n, samples, radius, mint=AO_MINT, out=d_ao)[1],
            "ao_map": lambda: gpu.ao_map(cam, w, h, mint, maxt, samples, radius, ao_mint=AO_MINT)[-1],
            "depth_map": lambda: gpu.depth_map(cam, w, h, mint, maxt, ids=True, normals=True)[-1],
        })
        # the answers: the fused floats are the yardstick's counts, ao_map's are the fused floats
        counts = d_occ.view(n_hit, samples).sum(dim=1, dtype=torch.int32).cpu().numpy()
        want = np.ones(len(p), F)
        want[hit] = (F(samples) - counts.astype(F)) * (F(1.0) / F(samples))
        got = d_ao.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "ambient_occlusion != the counts of scene_occluded"
        assert np.array_equal(gpu.ao_map(cam, w, h, mint, maxt, samples, radius, ao_mint=AO_MINT)[0].reshape(-1).view(np.uint32), want.view(np.uint32))
        y, f, m, dm = (res[k] for k in ("scene_occluded", "ambient_occlusion", "ao_map", "depth_map"))
        for k in ("segments", "sphere_tests", "node_tests", "quad_tests"):
            assert getattr(y[3], k) == getattr(f[3], k), (k, getattr(y[3], k), getattr(f[3], k))
        out.append(f"{name}, {w} x {h}, {samples} samples, radius {radius:.3g}: {n_hit} of {len(p)} pixels hit, {n_rays} AO rays, "
                   f"{float(counts.sum()) / n_rays:.1%} occluded, mean ao {float(got[hit].mean()):.3f}")
        for label, (med, lo, hi, st) in (("scene_occluded (stored rays)", y), ("ambient_occlusion (fused)", f)):
            out.append(f"  {label:<29} {med:9.3f} ms ({lo:.3f} - {hi:.3f})  {1e6 * med / n_rays:8.3f} ns/ray  sphere tests {st.sphere_tests / n_rays:8.2f}  "
                       f"node visits {st.node_tests / n_rays:8.2f}  quad + triangle tests {st.quad_tests / n_rays:8.2f} per ray")
        spread = y[2] - y[1]
        verdict = "not slower" if f[0] <= y[0] + spread else "SLOWER than the yardstick by more than its min-max spread"
        out.append(f"  fused / stored {f[0] / y[0]:.3f}  (the yardstick's spread {spread:.3f} ms: {verdict}); the stored rays are {n_rays * 24 / 2 ** 20:.0f} MiB "
                   f"read and {n_rays / 2 ** 20:.1f} MiB written, the fused call reads {len(p) * 24 / 2 ** 20:.1f} MiB and writes {len(p) * 4 / 2 ** 20:.1f} MiB")
        out.append(f"  ao_map (depth pass + AO)      {m[0]:9.3f} ms ({m[1]:.3f} - {m[2]:.3f});  depth_map alone {dm[0]:.3f} ms ({dm[1]:.3f} - {dm[2]:.3f});  "
                   f"ao_map - depth_map {m[0] - dm[0]:.3f} ms")
        del d_rays, d_occ, d_p, d_n, d_ao
        torch.cuda.empty_cache()
    return out


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else "acd"
    out = []
    if only == "acd" or only == "a":
        out.append(f"ambient occlusion, fused (rtw_ctx_ambient_occlusion) against rtw_ctx_scene_occluded over the same rays stored on the device (made by ao_rays; "
                   f"not timed), alternating in one process; warm-up + median of {RUNS} (min - max); kernel_ms")
    W, H = 1920, 1080
    with R.Renderer(0) as gpu:
        if "a" in only:
            scene = R.Scene.generate(R.SCENE_C2)
            gpu.set_scene(scene)
            cam = R.camera2_new(W / H, (13.0, 2.0, 3.0), (0.0, 1.0, 0.0), (-13.0, -2.0, -3.0), 20.0, 0.0)
            out += workload(gpu, "(a) Book-1 final scene, 485 spheres, BVH", cam, 1e-3, 1e3, 22.0)     # (the small spheres lie within -11 .. 11)
        if "c" in only:
            vtx, faces = R.mesh_terrain(317, seed=2)
            gpu.set_scene(R.Scene((), triangles=R.Triangle.from_mesh(vtx, faces)))
            blo, bhi = vtx.min(axis=0), vtx.max(axis=0)
            c, ext = (blo + bhi) / 2, float((bhi - blo).max())
            cam = R.camera2_new(W / H, (float(c[0]), float(c[1] + 0.6 * ext), float(c[2] - 0.9 * ext)), (0.0, 1.0, 0.0), (0.0, -0.55, 0.83), 50.0, 0.0)
            out += workload(gpu, f"(c) terrain, {len(faces)} triangles, BVH", cam, 1e-3, 1e4, ext)
        if "d" in only:
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
            out += workload(gpu, f"(d) {n} placements of the {len(faces)}-triangle terrain, top-level tree, BVH", cam, 1e-3, 1e4, reach)
            gpu.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)
    text = "\n".join(out) + "\n"
    print(text, end="")
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "profiles", "ao.log")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    open(dst, "w").write(text)


if __name__ == "__main__":
    main()
