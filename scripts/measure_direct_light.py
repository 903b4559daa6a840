#!/usr/bin/env python3
"""Direct lighting, fused, against the any-hit pass over stored rays, measured: writes profiles/direct_light.log.  One MI355X.

    python scripts/measure_direct_light.py [--only a|b|c] [--out FILE]

Without --only every workload runs in a process of its own under a time limit, in turn, and the first failure stops the rest; the log is
what they printed.  Each workload runs as direct_light_map's points at 1920 x 1080 with 16 samples and at 480 x 270 with 64.  The yardstick
is the code as it stood before the fused kernel: rtw_ctx_scene_occluded on the same rays, made beforehand by light_samples from the map's own
points and faced normals, the cast ones resident on the device (24 bytes per ray read, one byte per ray written; making and uploading the
rays is not timed).  Against it stands rtw_ctx_direct_light on the same points, device tensors in and out: the two calls alternate in one
process, a warm-up of each, then the median of RUNS with min - max; RtwStats.kernel_ms.  direct_light_map (both launches) and depth_map are
timed the same way beside them.  Every answer is checked: the fused kernel's vis is the count of the yardstick's free bytes per item, its
irr is light_reduce of the host weights under that mask, direct_light_map's are the same floats, and the counters are equal.

  (a) the golden light scene (tests/golden/rust2_light_scene.json): one sphere, six quads; a quad light and a sphere light
  (b) lights_common.sphere_field: the same with 60 small spheres on the floor of the box (61 spheres: the sphere tree), the same lights
  (c) the 200k-triangle terrain of scripts/measure_ao.py under one quad light"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

RUNS = 9
DEV = "cuda:0"
F = np.float32
SIZES = ((1920, 1080, 16), (480, 270, 64))
LO, HI = 1e-3, 1.0 - 1e-3
LIMIT_S = 360                            # per workload
STATS = ("segments", "sphere_tests", "node_tests", "quad_tests")


def workload(R, torch, gpu, name, scene, lights, cam, mint, maxt):
    from scripts.measure_ao import device, points_of, timed
    out = []
    nl = len(lights)
    for w, h, samples in SIZES:
        p, faced, hit = points_of(gpu, cam, w, h, mint, maxt)
        rays, wts = R.light_samples(scene, lights, p, faced, samples, 0)          # (sample [i][l][k] depends on i: made at the pixels' own indices)
        cast = np.any(rays[..., 3:] != 0.0, axis=-1)
        n_rays = int(cast.sum())
        d_rays = device(rays[cast])
        del rays
        d_p, d_n = device(p), device(faced)
        d_occ = torch.empty(n_rays, dtype=torch.uint8, device=DEV)
        d_vis = torch.empty((len(p), nl), dtype=torch.float32, device=DEV)
        d_irr = torch.empty((len(p), nl), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        res = timed({
            "scene_occluded": lambda: gpu.scene_occluded(d_rays, LO, HI, out=d_occ)[1],
            "direct_light": lambda: gpu.direct_light(d_p, d_n, samples, LO, HI, out_vis=d_vis, out_irr=d_irr)[-1],
            "direct_light_map": lambda: gpu.direct_light_map(cam, w, h, mint, maxt, samples, LO, HI)[-1],
            "depth_map": lambda: gpu.depth_map(cam, w, h, mint, maxt, ids=True, normals=True)[-1],
        })
        # the answers: the fused floats are the yardstick's bytes reduced on the host, direct_light_map's are the fused floats
        free = cast.copy()
        free[cast] = d_occ.cpu().numpy() == 0
        want_vis = (free.sum(axis=-1).astype(F) * (F(1.0) / F(samples))).astype(F)
        want_irr = R.light_reduce(np.where(free, wts, F(0.0)).astype(F))
        got_vis, got_irr = d_vis.cpu().numpy(), d_irr.cpu().numpy()
        assert np.array_equal(got_vis.view(np.uint32), want_vis.view(np.uint32)), "direct_light's vis != the counts of scene_occluded"
        assert np.array_equal(got_irr.view(np.uint32), want_irr.view(np.uint32)), "direct_light's irr != light_reduce under scene_occluded's mask"
        m_vis, m_irr, _ = gpu.direct_light_map(cam, w, h, mint, maxt, samples, LO, HI)
        assert np.array_equal(m_vis.reshape(-1, nl).view(np.uint32), want_vis.view(np.uint32))
        assert np.array_equal(m_irr.reshape(-1, nl).view(np.uint32), want_irr.view(np.uint32))
        y, f, m, dm = (res[k] for k in ("scene_occluded", "direct_light", "direct_light_map", "depth_map"))
        for k in STATS:
            assert getattr(y[3], k) == getattr(f[3], k), (k, getattr(y[3], k), getattr(f[3], k))
        n_items = int(hit.sum()) * nl
        out.append(f"{name}, {w} x {h}, {nl} light(s), {samples} samples: {int(hit.sum())} of {len(p)} pixels hit, {n_rays} of {n_items * samples} samples cast, "
                   f"{1.0 - float(free.sum()) / n_rays:.1%} of them blocked, mean vis {float(got_vis[hit].mean()):.3f}, mean irr {float(got_irr[hit].mean()):.4f}")
        for label, (med, lo, hi, st) in (("scene_occluded (stored rays)", y), ("direct_light (fused)", f)):
            out.append(f"  {label:<29} {med:9.3f} ms ({lo:.3f} - {hi:.3f})  {1e6 * med / n_rays:8.3f} ns/ray  sphere tests {st.sphere_tests / n_rays:8.2f}  "
                       f"node visits {st.node_tests / n_rays:8.2f}  quad + triangle tests {st.quad_tests / n_rays:8.2f} per ray")
        spread = y[2] - y[1]
        verdict = "not slower" if f[0] <= y[0] + spread else "SLOWER than the yardstick by more than its min-max spread"
        out.append(f"  fused / stored {f[0] / y[0]:.3f}  (the yardstick's spread {spread:.3f} ms: {verdict}); the stored rays are {n_rays * 24 / 2 ** 20:.0f} MiB "
                   f"read and {n_rays / 2 ** 20:.1f} MiB written, the fused call reads {len(p) * 24 / 2 ** 20:.1f} MiB and writes {len(p) * nl * 8 / 2 ** 20:.1f} MiB")
        out.append(f"  direct_light_map (depth pass + lights) {m[0]:9.3f} ms ({m[1]:.3f} - {m[2]:.3f});  depth_map alone {dm[0]:.3f} ms ({dm[1]:.3f} - {dm[2]:.3f});  "
                   f"the difference {m[0] - dm[0]:.3f} ms")
        del d_rays, d_occ, d_p, d_n, d_vis, d_irr, wts, cast, free
        torch.cuda.empty_cache()
    return out


def one(only):
    import torch
    import rtw_amd as R
    from tests import lights_common as LC
    W, H = 1920, 1080
    with R.Renderer(0) as gpu:
        if only in "ab":
            ls, g = LC.golden()
            if only == "b":
                ls = LC.LightScene(LC.sphere_field(g), g["quads"], ls.lights, g["background"])
            gpu.set_scene(ls.scene)
            gpu.set_lights(ls.lights)
            name = "(a) the golden light scene, 1 sphere, 6 quads" if only == "a" else f"(b) sphere_field, {ls.scene.n_spheres} spheres, 6 quads, BVH"
            return workload(R, torch, gpu, name, ls.scene, ls.lights, LC.camera(g, W, H), g["mint"], g["maxt"])
        vtx, faces = R.mesh_terrain(317, seed=2)
        blo, bhi = vtx.min(axis=0), vtx.max(axis=0)
        c, ext = (blo + bhi) / 2, float((bhi - blo).max())
        lamp = R.Quad.new((float(c[0] - 0.1 * ext), float(bhi[1] + 0.3 * ext), float(c[2] - 0.1 * ext)), (0.2 * ext, 0.0, 0.0), (0.0, 0.0, 0.2 * ext))
        scene = R.Scene((), quads=[lamp], triangles=R.Triangle.from_mesh(vtx, faces))
        lights = [(R.LIGHT_QUAD, 0)]
        gpu.set_scene(scene)
        gpu.set_lights(lights)
        cam = R.camera2_new(W / H, (float(c[0]), float(c[1] + 0.6 * ext), float(c[2] - 0.9 * ext)), (0.0, 1.0, 0.0), (0.0, -0.55, 0.83), 50.0, 0.0)
        return workload(R, torch, gpu, f"(c) terrain, {len(faces)} triangles under one quad light, BVH", scene, lights, cam, 1e-3, 1e4)


def main():
    if "--only" in sys.argv:
        print("\n".join(one(sys.argv[sys.argv.index("--only") + 1])))
        return 0
    text = (f"direct lighting, fused (rtw_ctx_direct_light) against rtw_ctx_scene_occluded over the same rays stored on the device (made by light_samples; "
            f"not timed), alternating in one process; warm-up + median of {RUNS} (min - max); kernel_ms\n")
    print(text, end="", flush=True)
    status = 0
    for only in "abc":                   # each workload in a process of its own, under a time limit; the first failure stops the rest
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", only], capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            text += f"workload ({only}): no answer within {LIMIT_S} s; stopped\n"
            status = 1
            break
        text += r.stdout
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            text += f"workload ({only}) failed with status {r.returncode}; stopped\n" + r.stderr[-2000:] + "\n"
            status = 1
            break
    if status:
        print(text.splitlines()[-1] if text else "", file=sys.stderr)
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "profiles", "direct_light.log")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    open(dst, "w").write(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
