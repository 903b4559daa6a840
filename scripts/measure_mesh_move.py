#!/usr/bin/env python3
"""Moving mesh placements on the GPU, measured: writes profiles/mesh_move.log.

    python scripts/measure_mesh_move.py

The setup of scripts/measure_mesh_top.py: the 20k terrain placed on a square grid, 480 x 270, 4 spp, depth 6,
RTW_INTEGRATOR_RUST2, RTW_ACCEL_BVH.  Every comparison alternates its two sides in one process after a warm-up of both and reports the
median with min - max.

1. Move against set.  move_mesh_instances(poses) from a device tensor -- stream time between two events round the call on the context's
   stream, and wall time of the call (it ends with a stream synchronise) -- against rtw_ctx_set_mesh_instances of the same poses from a host
   array that is already built (the parent's path: validate, rows, boxes, binned SAH, uploads; the copy of the poses to the host that a
   caller whose poses live in torch pays on top is not in it).  64, 1024, 4096 and 65 536 placements.
2. Poses and mesh.  The same with ouv as well (a wave over the terrain), against clear + refit_triangles + set_mesh_instances.
3. The climb, A/B.  RTW_OPT_MESH_CLIMB = 1 (one launch of the triangle refit's inner kernel per height) against 2 (one launch of one
   workgroup): stream time of the move at 64, 1024, 4096, 16 384 and 65 536 placements, the two alternating call by call.
4. Tree quality.  At 1024 and 4096 placements the frame of 4.11 through the MOVED tree against a tree BUILT for the same poses, for (a)
   every placement turned by a random quaternion and shifted by a third of the grid pitch and (b) the poses permuted at random among the
   placements: RtwStats.kernel_ms and node visits per segment; the frames must be equal on the bits."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
LOG = os.path.join(HERE, "profiles", "mesh_move.log")
W, H, SPP, DEPTH = 480, 270, 4, 6
SIDE, SIZE = 100, 20.0                                           # 2 * 100^2 = 20k triangles over 20 x 20
ALTERNATIONS, CLIMBS, RENDERS = 7, 15, 7
COUNTS = (64, 1024, 4096, 65536)


def span(x, unit="ms"):
    return f"{statistics.median(x):9.3f} {unit} ({min(x):.3f} - {max(x):.3f})"


def grid(n):
    """[n][7] float32: the square grid of measure_mesh_top.py, identity quaternions."""
    side = int(round(n ** 0.5))
    out = np.zeros((side * side, 7), np.float32)
    j, i = np.divmod(np.arange(side * side), side)
    out[:, 0], out[:, 2], out[:, 3] = SIZE * (i - (side - 1) / 2), SIZE * (j - (side - 1) / 2), 1.0
    return out


def turned(poses, seed):
    """(a): every placement turned by a random quaternion and shifted by a third of the grid pitch."""
    rng = np.random.default_rng(seed)
    out = poses.copy()
    d = rng.normal(size=(len(out), 3))
    out[:, :3] += ((SIZE / 3.0) * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    out[:, 3:] = rng.normal(size=(len(out), 4)).astype(np.float32)
    return out


def permuted(poses, seed):
    """(b): the poses permuted at random among the placements."""
    return poses[np.random.default_rng(seed).permutation(len(poses))].copy()


def pods(R, poses):
    arr = (R.RtwMeshInstance * len(poses))()
    C.memmove(arr, np.ascontiguousarray(poses, np.float32).ctypes.data, poses.nbytes)
    return arr


def camera(R, n):
    reach = SIZE * max(1.0, n ** 0.5)
    return R.camera2_new(W / H, (0.0, 0.45 * reach, -0.75 * reach), (0.0, 1.0, 0.0), (0.0, -0.5, 1.0), 50.0, 0.0)


def params(R):
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth = W, H, SPP, DEPTH
    p.gamma, p.mint, p.maxt = 1.0, 1e-3, 1e4
    p.integrator, p.sampler, p.accel = R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, R.ACCEL_BVH
    p.seed = 1
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    return p


def main():
    import torch
    import rtw_amd as R
    L = R.lib()
    dev = torch.device("cuda:0")
    S = torch.cuda.Stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = [f"moving mesh placements: the 20k terrain on a square grid; warm-up, then the two sides of every comparison in turn; median (min - max)"]
    vtx, faces = R.mesh_terrain(SIDE, SIZE, 1.0, seed=3)
    tris = R.Triangle.from_mesh(vtx, faces)
    wave = vtx.copy()
    wave[:, 1] += (0.3 * np.sin(1.5 * vtx[:, 0].astype(np.float64))).astype(np.float32)
    ouv_wave, ouv_rest = R.mesh_ouv(wave, faces), R.mesh_ouv(vtx, faces)
    scene = R.Scene([R.Sphere.new((0.0, 3.0, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M)], background=(0.6, 0.7, 0.9))

    def stream_and_wall(gpu, call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(S)
        lw = call()
        e1.record(S)
        wall = (time.perf_counter() - t0) * 1e3
        e1.synchronize()
        assert lw == 0, lw
        return e0.elapsed_time(e1), wall

    with R.Renderer(0) as gpu:
        gpu.set_scene(scene)
        gpu.set_triangles(tris)
        gpu.use_torch_stream(S)
        t_wave, t_rest = torch.from_numpy(ouv_wave).to(dev), torch.from_numpy(ouv_rest).to(dev)
        # ---- 1 and 2: move against set ------------------------------------------------------------------------------------------------------
        for n in COUNTS:
            base = grid(n)
            lists = [turned(base, 100 + j) for j in range(ALTERNATIONS + 1)]
            tensors = [torch.from_numpy(a).to(dev) for a in lists]
            arrays = [pods(R, a) for a in lists]
            torch.cuda.synchronize()
            assert L.rtw_ctx_set_mesh_instances(gpu._h, arrays[0], n) == 0
            nodes, _ = gpu.mesh_top_dump()
            gpu.move_mesh_instances(tensors[0])                                   # warm-up of both paths
            ms, mw, sw = [], [], []
            for j in range(1, ALTERNATIONS + 1):
                s, w = stream_and_wall(gpu, lambda: gpu.move_mesh_instances(tensors[j]))
                ms.append(s)
                mw.append(w)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert L.rtw_ctx_set_mesh_instances(gpu._h, arrays[j], n) == 0
                sw.append((time.perf_counter() - t0) * 1e3)
            gpu.move_mesh_instances(tensors[0])
            back = []
            for j in range(20):                                                   # ... and back to back, no set between them
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gpu.move_mesh_instances(tensors[j % len(tensors)])
                back.append((time.perf_counter() - t0) * 1e3)
            out.append(f"{n:6d} placements, {len(nodes)} top-level nodes")
            out.append(f"  move_mesh_instances(poses)       stream {span(ms)}")
            out.append(f"  move_mesh_instances(poses)       wall   {span(mw)}    each behind a set_mesh_instances")
            out.append(f"  move_mesh_instances(poses)       wall   {span(back)}    20 calls back to back")
            out.append(f"  set_mesh_instances               wall   {span(sw)}    set / move back to back (medians) {statistics.median(sw) / statistics.median(back):.0f} x")
            # poses and mesh against clear + refit_triangles + set
            both_s, both_w, three = [], [], []
            gpu.move_mesh_instances(tensors[0], t_wave)
            for j in range(1, ALTERNATIONS + 1):
                t_mesh = t_wave if j % 2 else t_rest
                s, w = stream_and_wall(gpu, lambda: gpu.move_mesh_instances(tensors[j], t_mesh))
                both_s.append(s)
                both_w.append(w)
                t_mesh = t_rest if j % 2 else t_wave
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert L.rtw_ctx_set_mesh_instances(gpu._h, None, 0) == 0
                assert gpu.refit_triangles(t_mesh) == 0
                assert L.rtw_ctx_set_mesh_instances(gpu._h, arrays[j], n) == 0
                three.append((time.perf_counter() - t0) * 1e3)
            out.append(f"  move_mesh_instances(poses, ouv)  stream {span(both_s)}")
            out.append(f"  move_mesh_instances(poses, ouv)  wall   {span(both_w)}")
            out.append(f"  clear + refit_triangles + set    wall   {span(three)}    three calls / move (medians) {statistics.median(three) / statistics.median(both_w):.0f} x")
            gpu.move_mesh_instances(None, t_rest)
        # ---- 3: the climb, A/B ----------------------------------------------------------------------------------------------------------------
        out.append(f"the climb, A/B: stream time of move_mesh_instances(poses), RTW_OPT_MESH_CLIMB 1 (a launch per height) and 2 (one workgroup) call by call, {CLIMBS} each")
        for n in (64, 1024, 4096, 16384, 65536):
            base = grid(n)
            tensors = [torch.from_numpy(turned(base, 200 + j)).to(dev) for j in range(2)]
            assert L.rtw_ctx_set_mesh_instances(gpu._h, pods(R, base), n) == 0
            nodes, _ = gpu.mesh_top_dump()
            ms = {1: [], 2: []}
            for j in range(CLIMBS + 1):
                for climb in (1, 2):
                    gpu.set_option(R.OPT_MESH_CLIMB, climb)
                    s, _ = stream_and_wall(gpu, lambda: gpu.move_mesh_instances(tensors[j % 2]))
                    if j:                                                         # (the first round is the warm-up)
                        ms[climb].append(s)
            gpu.set_option(R.OPT_MESH_CLIMB, 0)
            out.append(f"  {n:6d} placements, {len(nodes):6d} nodes:  per height {span([1e3 * x for x in ms[1]], 'us')}   one workgroup {span([1e3 * x for x in ms[2]], 'us')}"
                       f"   one workgroup / per height (medians) {statistics.median(ms[2]) / statistics.median(ms[1]):.3f}")
        # ---- 4: tree quality --------------------------------------------------------------------------------------------------------------------
        gpu.set_stream(None)
        gpu.set_option(R.OPT_MESH_LIST_MAX, 0)
        p = params(R)
        for n in (1024, 4096):
            base, cam = grid(n), camera(R, n)
            for name, moved in (("(a) turned and shifted", turned(base, 7)), ("(b) permuted", permuted(turned(base, 7), 8))):
                start = base if name.startswith("(a)") else turned(base, 7)
                res = {}
                for which in ("moved", "built"):
                    if which == "moved":
                        assert L.rtw_ctx_set_mesh_instances(gpu._h, pods(R, start), n) == 0
                        assert gpu.move_mesh_instances(moved) == 0
                    else:
                        assert L.rtw_ctx_set_mesh_instances(gpu._h, pods(R, moved), n) == 0
                    gpu.render(cam, p)
                    ms = []
                    for _ in range(RENDERS):
                        img, st = gpu.render(cam, p)
                        ms.append(st.kernel_ms)
                    res[which] = (ms, st, img)
                same = np.array_equal(res["moved"][2].view(np.uint32), res["built"][2].view(np.uint32))
                for which in ("moved", "built"):
                    ms, st, _ = res[which]
                    out.append(f"  {n:5d} placements {name:<24} tree {which:<6} {span(ms)}  {st.node_tests / st.segments:9.2f} node visits per segment ({st.segments} segments)")
                out.append(f"  {n:5d} placements {name:<24} moved / built: kernel {statistics.median(res['moved'][0]) / statistics.median(res['built'][0]):.3f}, node visits "
                           f"{res['moved'][1].node_tests / res['built'][1].node_tests:.3f}; frames equal: {same}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else LOG
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    open(dst, "w").write(text)


if __name__ == "__main__":
    main()
