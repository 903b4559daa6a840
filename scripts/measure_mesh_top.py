#!/usr/bin/env python3
"""The top-level tree over mesh placements, measured: writes profiles/mesh_top_tree.log.

    python scripts/measure_mesh_top.py                        this tree: everything below
    python scripts/measure_mesh_top.py --parent --tree DIR    a checkout of the parent commit in DIR (built): its list order at N = 1 .. 64,
                                                              APPENDED to profiles/mesh_top_tree.log of THIS tree: run it second
(The parent's rows come from a checkout of its own, package and library, not from scripts/gpu_ab_libs.sh: this tree's package binds
rtw_mesh_top_dump and its kin when it loads a library, and the parent's library does not have them.)

The setup of scripts/measure_mesh_instances.py: the 20k terrain, 480 x 270, 4 spp, depth 6, RTW_INTEGRATOR_RUST2,
RTW_ACCEL_BVH; RtwStats.kernel_ms, one warm-up render per variant, then the median of RUNS with min - max.  At each N the list order
(RTW_OPT_MESH_LIST_MAX = 4294967295) and the top-level tree (0) are rendered in turn, run by run, in one process; the frames must be equal
on the bits.  N <= 64: the same world geometry flattened into one triangle list (SPEC 8) beside them.
The scene holds one sphere, so those rows run render_brute<false, 12, true>.  Two more blocks, on this tree and on the parent, time the LIST
order through the kernels that lost occupancy to the second walk: render_bvh<false, global nodes, 12, true> (two far spheres added, the
sphere tree forced by RTW_OPT_LIST_WALK_MAX = 0 and RTW_FLAG_GLOBAL_NODES) at N = 1 .. 64, and rtw_ctx_depth_map (1920 x 1080, ids and
normals) at N = 16 and 64."""
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = "--parent" in sys.argv
ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, ROOT)
import rtw_amd as R  # noqa: E402

W, H, SPP, DEPTH, RUNS = 480, 270, 4, 6, 9
SIDE, SIZE = 100, 20.0                                           # 2 * 100^2 = 20k triangles over 20 x 20
NEVER = 4294967295
COUNTS = (1, 4, 16, 64) if PARENT else (1, 4, 16, 64, 256, 1024, 4096)


def params():
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth = W, H, SPP, DEPTH
    p.gamma, p.mint, p.maxt = 1.0, 1e-3, 1e4
    p.integrator, p.sampler, p.accel = R.INTEGRATOR_RUST2, R.SAMPLER_CENTRES, R.ACCEL_BVH
    p.seed = 1
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    return p


def grid(n):
    side = int(round(n ** 0.5))
    return [((SIZE * (i - (side - 1) / 2), 0.0, SIZE * (j - (side - 1) / 2)), (1.0, 0.0, 0.0, 0.0)) for j in range(side) for i in range(side)]


def camera(n):
    reach = SIZE * max(1.0, n ** 0.5)
    return R.camera2_new(W / H, (0.0, 0.45 * reach, -0.75 * reach), (0.0, 1.0, 0.0), (0.0, -0.5, 1.0), 50.0, 0.0)


def timed(gpu, cam, p, options=(None,)):
    """One warm-up render per option, then RUNS rounds with the options in turn: {option: (median, min, max, stats, image)}."""
    def render(o):
        if o is not None:
            gpu.set_option(R.OPT_MESH_LIST_MAX, o)
        return gpu.render(cam, p)
    for o in options:
        render(o)
    ms, last = {o: [] for o in options}, {}
    for _ in range(RUNS):
        for o in options:
            img, st = render(o)
            ms[o].append(st.kernel_ms)
            last[o] = (st, img)
    return {o: (statistics.median(ms[o]), min(ms[o]), max(ms[o])) + last[o] for o in options}


def line(name, r):
    med, lo, hi, st = r[:4]
    return (f"{name:<44} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {1e6 * med / st.segments:8.3f} ns/segment  {st.segments:9d} segments  "
            f"{st.node_tests / st.segments:9.2f} node visits  {st.quad_tests / st.segments:7.2f} triangle tests per segment")


def main():
    out = [f"top-level tree over mesh placements: {W} x {H}, {SPP} spp, depth {DEPTH}, RUST2, BVH; warm-up + median of {RUNS} (min - max); kernel_ms"
           + ("  [PARENT COMMIT: list order]" if PARENT else "")]
    vtx, faces = R.mesh_terrain(SIDE, SIZE, 1.0, seed=3)
    scene = R.Scene([R.Sphere.new((0.0, 3.0, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M)], background=(0.6, 0.7, 0.9))
    p = params()
    with R.Renderer(0) as gpu:
        gpu.set_scene(scene)
        tris = R.Triangle.from_mesh(vtx, faces)
        for n in COUNTS:
            gpu.set_triangles(tris)
            gpu.set_mesh_instances(grid(n))
            if PARENT:
                out.append(line(f"placed {n:4d} x, list order (parent)", timed(gpu, camera(n), p)[None]))
                continue
            r = timed(gpu, camera(n), p, (NEVER, 0))
            same = np.array_equal(r[NEVER][4].view(np.uint32), r[0][4].view(np.uint32))
            out.append(line(f"placed {n:4d} x, list order", r[NEVER]))
            out.append(line(f"placed {n:4d} x, top-level tree", r[0]) + f"  tree / list {r[0][0] / r[NEVER][0]:.3f}  frames equal: {same}")
        # the list order through render_bvh<false, global nodes, 12, true> and through the query kernel, here and on the parent
        if not PARENT:
            gpu.set_option(R.OPT_MESH_LIST_MAX, NEVER)
        far = [R.Sphere.new((0.0, -5e3, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M), R.Sphere.new((9.0, -5e3, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M)]
        gpu.set_scene(R.Scene([R.Sphere.new((0.0, 3.0, 0.0), 1.0, (0.8, 0.8, 0.8), R.SCATTER_M)] + far, background=(0.6, 0.7, 0.9)))
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        pg = params()
        pg.flags |= R.FLAG_GLOBAL_NODES
        who = " (parent)" if PARENT else ""
        for n in (1, 4, 16, 64):
            gpu.set_triangles(tris)
            gpu.set_mesh_instances(grid(n))
            r = timed(gpu, camera(n), pg)[None]
            out.append(line(f"placed {n:4d} x, list order, {gpu.last_render_build()}{who}", r))
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
        for n in (16, 64):
            gpu.set_triangles(tris)
            gpu.set_mesh_instances(grid(n))
            cam = R.camera2_new(1920 / 1080, (0.0, 0.45 * SIZE * n ** 0.5, -0.75 * SIZE * n ** 0.5), (0.0, 1.0, 0.0), (0.0, -0.5145, 0.8575), 50.0, 0.0)
            ms = [gpu.depth_map(cam, 1920, 1080, 1e-3, 1e4, ids=True, normals=True)[-1].kernel_ms for _ in range(RUNS + 1)][1:]
            out.append(f"depth_map 1920 x 1080, ids + normals, placed {n:2d} x, list order{who}: {statistics.median(ms):.3f} ms ({min(ms):.3f} - {max(ms):.3f})")
        gpu.set_scene(scene)
        if not PARENT:
            gpu.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)
            for n in (1, 4, 16, 64):
                flat = np.concatenate([vtx + np.asarray(pos, np.float32)[None] for pos, _ in grid(n)])
                ff = np.concatenate([faces + k * len(vtx) for k in range(n)])
                gpu.set_triangles(R.Triangle.from_mesh(flat, ff))
                out.append(line(f"flattened {n:2d} x = {len(ff)} triangles (SPEC 8)", timed(gpu, camera(n), p)[None]))
    text = "\n".join(out) + "\n"
    print(text, end="")
    dst = os.path.join(HERE, "profiles", "mesh_top_tree.log")
    if "--out" in sys.argv:
        dst = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    open(dst, "a" if PARENT else "w").write(text)


if __name__ == "__main__":
    main()
