#!/usr/bin/env python3
"""The refit of the triangle tree, measured: writes profiles/refit.log.

    python scripts/measure_refit.py                      speed and tree quality: everything but the launch table
    python scripts/measure_refit.py --refits-only        a warm-up and 20 refits per mesh and nothing else: the run to put under
                                                         rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/measure_refit.py --refits-only
    python scripts/measure_refit.py --trace DIR          the launch table from that trace, APPENDED to profiles/refit.log: run it last

Meshes: mesh_icosphere(5) (20 480 triangles) and mesh_terrain(317) (200 978).  The deformation is a wave along x, y += a sin(k x + phase),
its amplitude a third of the mesh's height.

Speed.  refit_triangles from a device tensor that already holds origin / u / v: wall time of the call (it ends with a stream synchronise)
and stream time between two events round it on the context's stream.  Beside it set_triangles of the same geometry from a host array that
is already built -- the parent's path, unchanged: prepare, build and three uploads; the copy of the vertices to the host that a caller
whose mesh lives in torch pays on top is not in it.  The two are interleaved, ALTERNATIONS times; median, min and max of each.
Then 20 refits back to back: a refit that directly follows a set_triangles is the first call to touch buffers just reserved, and its wall
time (not its stream time) carries that.

Tree quality.  The price of keeping the topology: the tree built for the rest shape and refitted to the wave against a tree built for
the wave, same camera, same frame (the images must be equal on the bits): RtwStats.kernel_ms and node visits per segment."""
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
LOG = os.path.join(HERE, "profiles", "refit.log")
ALTERNATIONS, RENDERS = 5, 5
W, H, SPP, DEPTH = 480, 270, 4, 6


def meshes(R):
    return [("icosphere(5)", R.mesh_icosphere(5), 0.3, 4.0), ("terrain(317)", R.mesh_terrain(317, seed=2), 0.6, 1.5)]


def wave(v, amp, k, phase=0.0):
    w = v.copy()
    w[:, 1] += (amp * np.sin(k * v[:, 0].astype(np.float64) + phase)).astype(np.float32)
    return w


def span(x):
    return f"{statistics.median(x):9.3f} ms ({min(x):.3f} - {max(x):.3f})"


def heights(nodes):
    h = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes) - 1, -1, -1):
        if not nodes["leaf"][i]:
            h[i] = 1 + max(h[i + 1], h[int(nodes["skip"][i + 1])])
    return h


def measure():
    import torch
    import rtw_amd as R
    out = [f"refit of the triangle tree: refit_triangles (device tensor) beside set_triangles (host array) of the same geometry, interleaved, "
           f"{ALTERNATIONS} alternations; median (min - max)"]
    dev = torch.device("cuda:0")
    S = torch.cuda.Stream(dev)
    scene = R.Scene([R.Sphere.new((0.0, -50.0, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M)], background=(0.6, 0.7, 0.9))
    for name, (v, f), amp, k in meshes(R):
        n = len(f)
        rest = R.Triangle.from_mesh(v, f)
        with R.Renderer(0) as gpu:
            gpu.set_scene(scene)
            gpu.set_triangles(rest)
            gpu.use_torch_stream(S)
            nodes = gpu.triangle_bvh_dump()
            hs = heights(nodes)
            shapes = [wave(v, amp, k, 0.7 * j) for j in range(ALTERNATIONS + 1)]
            tensors = [torch.from_numpy(R.mesh_ouv(w, f)).to(dev) for w in shapes]
            arrays = [R.Triangle.from_mesh(w, f) for w in shapes]
            torch.cuda.synchronize()
            gpu.refit_triangles(tensors[0])                    # warm-up of both paths
            gpu.set_triangles(arrays[0])
            wall_r, stream_r, wall_s = [], [], []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for j in range(1, ALTERNATIONS + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record(S)
                lw = gpu.refit_triangles(tensors[j])
                e1.record(S)
                wall_r.append((time.perf_counter() - t0) * 1e3)
                e1.synchronize()
                stream_r.append(e0.elapsed_time(e1))
                assert lw == 0
                t0 = time.perf_counter()
                gpu.set_triangles(arrays[j])
                wall_s.append((time.perf_counter() - t0) * 1e3)
            # ... and the refit alone, back to back: between two set_triangles above every refit is the first to touch buffers just reserved
            gpu.refit_triangles(tensors[0])
            wall_b = []
            for j in range(20):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gpu.refit_triangles(tensors[j % len(tensors)])
                wall_b.append((time.perf_counter() - t0) * 1e3)
            out.append(f"{name}: {n} triangles, {len(nodes)} nodes, {int((hs == 0).sum())} leaves, {int(hs.max())} inner launches per refit "
                       f"(nodes per launch from the leaves' parents up: {np.bincount(hs)[1:].tolist()})")
            out.append(f"  refit_triangles  wall   {span(wall_r)}")
            out.append(f"  refit_triangles  stream {span(stream_r)}")
            out.append(f"  refit_triangles  wall   {span(wall_b)}    20 calls back to back, no set_triangles between them")
            out.append(f"  set_triangles    wall   {span(wall_s)}    set / refit (medians) {statistics.median(wall_s) / statistics.median(wall_r):.0f} x")
            # tree quality: built for the rest shape and refitted to the wave, against built for the wave
            gpu.set_stream(None)
            w = shapes[1]
            lo, hi = w.min(axis=0), w.max(axis=0)
            c, ext = (lo + hi) / 2, float((hi - lo).max())
            cam = R.camera2_new(W / H, (float(c[0]), float(c[1] + 0.6 * ext), float(c[2] - 0.9 * ext)), (0.0, 1.0, 0.0), (0.0, -0.55, 0.83), 50.0, 0.0)
            p = R.RtwParams()
            p.width, p.height, p.samples, p.depth = W, H, SPP, DEPTH
            p.gamma, p.mint, p.maxt = 1.0, 1e-3, 1e4
            p.integrator, p.sampler, p.accel, p.seed = R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, R.ACCEL_BVH, 1
            p.row_block, p.part_index, p.part_count = 8, 0, 1
            res = {}
            for which in ("refitted", "rebuilt"):
                if which == "refitted":
                    gpu.set_triangles(rest)
                    assert gpu.refit_triangles(tensors[1]) == 0
                else:
                    gpu.set_triangles(arrays[1])
                gpu.render(cam, p)
                ms = []
                for _ in range(RENDERS):
                    img, st = gpu.render(cam, p)
                    ms.append(st.kernel_ms)
                res[which] = (ms, st, img)
            same = np.array_equal(res["refitted"][2].view(np.uint32), res["rebuilt"][2].view(np.uint32))
            for which in ("refitted", "rebuilt"):
                ms, st, _ = res[which]
                out.append(f"  render {W} x {H}, {SPP} spp, depth {DEPTH}, tree {which:<9} {span(ms)}  {st.node_tests / st.segments:8.2f} node visits  "
                           f"{st.quad_tests / st.segments:6.2f} triangle tests per segment ({st.segments} segments)")
            out.append(f"  refitted / rebuilt: kernel {statistics.median(res['refitted'][0]) / statistics.median(res['rebuilt'][0]):.3f}, node visits "
                       f"{res['refitted'][1].node_tests / res['rebuilt'][1].node_tests:.3f}; frames equal: {same}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    open(LOG, "w").write(text)


def refits_only():
    import torch
    import rtw_amd as R
    scene = R.Scene([R.Sphere.new((0.0, -50.0, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M)])
    for name, (v, f), amp, k in meshes(R):
        with R.Renderer(0) as gpu:
            gpu.set_scene(scene)
            gpu.set_triangles(R.Triangle.from_mesh(v, f))
            t = torch.from_numpy(R.mesh_ouv(wave(v, amp, k), f)).to("cuda:0")
            torch.cuda.synchronize()
            for _ in range(21):
                gpu.refit_triangles(t)


def trace(d):
    """Per refit (a leaf-pass dispatch and the inner dispatches behind it): the kernels' own time and the span from the first start to the
    last end, gaps between launches included."""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    assert files, "no kernel trace under " + d
    rows = [r for r in csv.DictReader(open(files[-1])) if "tri_refit_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    refits = []
    for r in rows:
        a, b = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if "leaves" in r["Kernel_Name"]:
            refits.append(dict(grid=int(r.get("Grid_Size") or r["Grid_Size_X"]), leaf=b - a, inner=[], start=a, end=b))
        elif refits:
            refits[-1]["inner"].append(b - a)
            refits[-1]["end"] = b
    out = ["launches of a refit (rocprofv3 --kernel-trace of --refits-only; the first refit of each mesh dropped; medians over the rest, microseconds)"]
    for grid in sorted({r["grid"] for r in refits}):
        g = [r for r in refits if r["grid"] == grid][1:]
        leaf = statistics.median(r["leaf"] for r in g) / 1e3
        inner = statistics.median(sum(r["inner"]) for r in g) / 1e3
        whole = statistics.median(r["end"] - r["start"] for r in g) / 1e3
        out.append(f"  leaf pass of {grid:6d} threads: {leaf:8.1f} us;  {len(g[0]['inner']):2d} inner launches: {inner:7.1f} us in the kernels;  first start to last end "
                   f"{whole:8.1f} us -> the inner launches and the gaps round them are {100.0 * (whole - leaf) / whole:.0f} % of the refit's device time  ({len(g)} refits)")
    text = "\n".join(out) + "\n"
    print(text, end="")
    open(LOG, "a").write(text)


if __name__ == "__main__":
    if "--refits-only" in sys.argv:
        refits_only()
    elif "--trace" in sys.argv:
        trace(sys.argv[sys.argv.index("--trace") + 1])
    else:
        measure()
