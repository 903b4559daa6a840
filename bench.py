#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json's config, on N MI355X of one node.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

Workload (all N): config 3 of BASELINE.json -- the Book-1 final random-spheres scene (485 spheres, scene
seed 42), 1920 x 1080, 500 spp (render_row sampler), depth 50, gradient sky, render seed 1.  A "step" is
one full frame: every rank renders its interleaved 8-row blocks into HBM, one RCCL gather puts the frame
on rank 0.  The frame is a fixed amount of work split over N GPUs, hence "scaling": "strong".
value = (closest-hit queries == "rays x bounces" of all ranks, counted exactly by the kernel) / wall time.

The JSON line also carries
  roofline      for the render kernel (+ its resolve pass): ALGORITHMIC f32 flop (DESIGN.md "Roofline": 50/node visit,
                17/exact sphere test, 120/segment) / mean kernel time (HIP events on the launch stream,
                taken inside rtw_ctx_render) against the 157.3 TFLOP/s f32 vector peak.  The path is
                VALU-bound by construction (12 B of HBM per pixel per frame); `hbm` gives the achieved
                framebuffer GB/s for completeness.
  cpu_baseline  (--full only) the CPU oracle (a port: the reference's Rust cannot be built offline) timed on this
                host's cores on a bounded sample of the SAME frame (every 17th 8-row block, fewer spp).

A plain run sets up, warms up, times the --steps frames and prints the line; --full adds the CPU baseline.
--dump-outputs DIR writes what the last timed step computed: DIR/frame.npy (the [H][W][3] f32 frame on rank 0,
the array a caller of the render path receives) and DIR/counters.npy (f64 [camera_rays, segments] of that frame,
all ranks).  The scene, camera and seeds are fixed, so the same arguments give the same inputs on every run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F_NODE, F_SPHERE, F_SEGMENT = 50.0, 17.0, 120.0     # algorithmic f32 flop per unit (DESIGN.md "Roofline")
PEAK_TFLOPS = 157.3                                 # MI355X f32 vector peak (MI355X_MICROARCH.md)


def cpu_baseline(R, scene, cam, p):
    """Oracle on the host cores, ~10-20 s, on a subset of the same frame."""
    import ctypes as C
    from tests import oracle_binding as O
    # the GPU box gives one GPU's share of the host: 16 cores (os.cpu_count() reports the whole machine)
    threads = min(len(os.sched_getaffinity(0)), 16)
    q = R.RtwParams.from_buffer_copy(p)
    q.accel = R.ACCEL_BRUTE                     # the oracle has one closest-hit: the list-order loop
    q.row_block, q.part_index, q.part_count = 8, 0, 17      # 8 of the 135 row blocks, spread over the frame
    q.samples = 2
    _, st = O.render(cam, scene, q, threads)    # calibration
    rate = st.segments / max(st.total_ms, 1e-3) * 1e3
    target_s = 12.0
    q.samples = int(max(2, min(p.samples, round(2 * target_s * rate / max(st.segments, 1)))))
    _, st = O.render(cam, scene, q, threads)
    sec = st.total_ms / 1e3
    extra = {}
    if O.have_ref():
        # the reference's own C++ objects (oracle/_ref: Sphere::collisionNormal -> Material::onHit), serial like
        # C++/src/viewport.cpp, 1 core, on a much smaller slice (it is ~30x slower than the 16-thread port)
        r = R.RtwParams.from_buffer_copy(p)
        r.width, r.height, r.samples, r.part_count = p.width // 8, p.height // 8, 4, 1
        cam_s = R.RtwCamera.from_buffer_copy(cam)
        for k in range(3):
            cam_s.pixel00[k] = cam.pixel00[k] - 0.5 * (cam.delta_u[k] + cam.delta_v[k]) + 4.0 * (cam.delta_u[k] + cam.delta_v[k])
            cam_s.delta_u[k] = cam.delta_u[k] * 8
            cam_s.delta_v[k] = cam.delta_v[k] * 8
        _, seg_ref, sec_ref = O.ref_render(cam_s, scene, r, rand_seed=1)
        extra = {"reference_cpp_objects_1core": {"value": round(seg_ref / sec_ref / 1e6, 4), "unit": "Msamples/s", "cores": 1,
                                                 "sample": f"{r.width}x{r.height}x{r.samples} spp of the same view, {seg_ref} segments in {sec_ref:.2f} s"}}
    return {**extra, "value": round(st.segments / sec / 1e6, 4), "unit": "Msamples/s", "cores": threads, "kind": "port",
            "sample": f"oracle/rtw_oracle.c (f32 restatement of the Rust path, one task per row), rows of every 17th 8-row block "
                      f"({st.rows} rows) x {q.width} px x {q.samples} spp of the same frame, {st.segments} segments in {sec:.2f} s",
            "camera_msamples_per_s": round(st.camera_rays / sec / 1e6, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--accel", choices=["bvh", "brute"], default="bvh")
    ap.add_argument("--config", choices=["c3", "c2", "c4", "c5"], default="c3",
                    help="c3 = BASELINE.json's metric config (default); the others exist to profile their kernels and are NOT the headline")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write the last step's frame and counters as DIR/<name>.npy")
    ap.add_argument("--global-nodes", action="store_true", help="A/B: BVH nodes in global memory (f32) instead of LDS (f16)")
    ap.add_argument("--spp", type=int, default=0, help="override samples per pixel (INVALID as a benchmark; for smoke runs)")
    ap.add_argument("--chunk-sums", action="store_true", help="RTW_FLAG_CHUNK_SUMS: bank one partial sum per 4 samples (A/B; not the default association)")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE",
                    help="rtw_ctx_set_option, e.g. --opt 4=5 (RTW_OPT_BLOCKS_PER_CU = 5) or --opt 6=1 (one path per lane); A/B runs")
    ap.add_argument("--devices", default="", help="single-process rtw_mgpu over these HIP ordinals, e.g. 0,0,0 = three contexts on one GPU "
                                                  "(a rehearsal of the N-GPU path on a 1-GPU box: INVALID as a benchmark)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # dmabuf IPC only on this pool: must be in the environment BEFORE anything initialises HIP / HSA (torch.cuda, librtw_hip)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    import importlib
    import rtw_amd as R
    par = importlib.import_module("raytracing-in-a-weekend_amd.parallel")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus or world == 1, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available() and R.device_count() > 0, "bench.py needs the MI355X: there is no CPU path"
    backend = os.environ.get("RTW_BENCH_BACKEND", "nccl")       # "gloo": rehearse the N > 1 path on a 1-GPU box (tests only)
    if os.environ.get("RTW_BENCH_SINGLE_DEVICE"):               # ... with every rank on cuda:0
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)      # RCCL over xGMI
        else:
            dist.init_process_group(backend)

    if args.config == "c3":
        scene = R.Scene.generate(R.SCENE_C2, 42)
        cam, p = R.default_view(R.SCENE_C5)          # 1920 x 1080 x 500 spp x depth 50 framing
        cam.shutter = 0.0                            # config 3 is the static Book-1 scene
        workload = "BASELINE configs[2]: Book-1 final random-spheres scene (485 spheres, scene seed 42)"
    else:
        which = {"c2": R.SCENE_C2, "c4": R.SCENE_C4, "c5": R.SCENE_C5}[args.config]
        scene = R.Scene.generate(which, 42)
        cam, p = R.default_view(which)
        workload = {"c2": "BASELINE configs[1]: Book-1 final random-spheres scene", "c4": "BASELINE configs[3]: dielectric-heavy scene (183 spheres)",
                    "c5": "BASELINE configs[4]: Book-2 motion blur + image-textured ground (485 spheres)"}[args.config] + " -- NOT the headline config"
    p.accel = R.ACCEL_BVH if args.accel == "bvh" else R.ACCEL_BRUTE
    if args.global_nodes:
        p.flags |= 4          # RTW_FLAG_GLOBAL_NODES
    if args.chunk_sums:
        p.flags |= 16         # RTW_FLAG_CHUNK_SUMS
    if args.spp:
        p.samples = args.spp
    H, W = p.height, p.width

    single_process_multi = world == 1 and (args.gpus > 1 or bool(args.devices))   # one process drives all GPUs through the C ABI's rtw_mgpu
    if single_process_multi:
        devices = [int(x) for x in args.devices.split(",")] if args.devices else list(range(args.gpus))
        assert R.device_count() > max(devices), f"devices {devices} but only {R.device_count()} HIP devices are visible"
        args.gpus = len(devices)
        r = R.MultiRenderer(devices)              # fork / ordered join of viewport.rs:236-244 over GPUs, no torch.distributed
        r.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
        for kv in args.opt:
            r.set_option(int(kv.split("=")[0]), float(kv.split("=")[1]))
        frame_buf = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)

        def step():
            _, tot, _ = r.render(cam, p, out=frame_buf.data_ptr())     # every device copies its row blocks straight into GPU 0's frame
            return frame_buf, tot
    else:
        r = R.Renderer(local_rank)                                  # one rtw_ctx per process == per GPU
        r.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        r.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
        for kv in args.opt:
            r.set_option(int(kv.split("=")[0]), float(kv.split("=")[1]))
        local = torch.zeros((par.max_rows(H, world), W, 3), dtype=torch.float32, device=dev)

        def render_rows(row_block, idx, cnt, out):
            q = R.RtwParams.from_buffer_copy(p)
            q.row_block, q.part_index, q.part_count = row_block, idx, cnt
            return r.render(cam, q, out=out.data_ptr())[1]

        def step():
            frame, st = par.render_frame(render_rows, H, W, rank, world, dev, local=local)
            return frame, st

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    seg = rays = nodes = tests = 0
    steps3, lanes3 = [0] * 5, [0] * 5
    kernel_ms = 0.0
    frame = None
    for _ in range(args.steps):
        frame, st = step()
        last = (st.camera_rays, st.segments)
        seg += st.segments; rays += st.camera_rays; nodes += st.node_tests; tests += st.sphere_tests
        kernel_ms += st.kernel_ms
        for k in range(5):
            steps3[k] += st.phase_steps[k]; lanes3[k] += st.phase_lanes[k]
    fence()
    elapsed = time.perf_counter() - t0
    elapsed = par.max_over_ranks(elapsed, world, dev)
    seg, rays, nodes, tests = par.reduce_counters([seg, rays, nodes, tests], world, dev)
    kernel_ms_max = par.max_over_ranks(kernel_ms, world, dev)
    if args.dump_outputs:
        last = par.reduce_counters(list(last), world, dev)        # collective: every rank takes part

    if single_process_multi:
        world = args.gpus                                           # per-GPU figures below divide by the GPUs that shared the frame
    if rank == 0:
        k_s = kernel_ms_max / 1e3 / args.steps                      # mean kernel time per launch (slowest rank)
        flop = (nodes * F_NODE + tests * F_SPHERE + seg * F_SEGMENT) / args.steps / world   # per launch, per GPU
        achieved = flop / k_s / 1e12
        # Counter evidence for this same command, from the committed rocprofv3 --pmc passes (scripts/profile_bench.sh +
        # scripts/summarise_profile.py): NOT measured in this run -- the source file is named in the line.
        traffic, traffic_source, executed, stale = None, None, None, None
        if world == 1 and not args.spp and args.accel == "bvh" and args.config == "c3" and not args.opt and not args.chunk_sums:
            import glob
            cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_rocprofv3_summary.json")))
            if cands:
                prof = json.load(open(cands[-1]))
                rel = os.path.relpath(cands[-1], ROOT)
                pmc, der = prof.get("pmc", {}), prof.get("derived", {})
                # The profile must be OF THIS KERNEL: its rocprofv3 kernel time (render + resolve) has to agree with this run's HIP-event time
                # within 3 %, else the counters belong to another build and are not quoted.
                prof_ms = der.get("render_kernel_avg_ms", 0.0) + der.get("resolve_kernel_avg_ms", 0.0)
                stale = {"stale_profile": True, "profile": rel, "profile_kernel_ms": round(prof_ms, 3), "this_run_kernel_ms": round(k_s * 1e3, 3),
                         "note": "the committed profile's kernel time differs from this run's by more than 3 %: traffic / executed_valu are not quoted"} \
                    if not (prof_ms > 0.0 and abs(prof_ms - k_s * 1e3) <= 0.03 * k_s * 1e3) else None
                if stale:
                    der, pmc = {}, {}
                if "hbm_bytes_per_step" in der:
                    traffic = der["hbm_bytes_per_step"]
                    traffic_source = f"{rel}: FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE, render + resolve, separate --pmc passes of this command"
                if "SQ_INSTS_VALU" in pmc and "render_kernel_avg_ms" in der:
                    insts = pmc["SQ_INSTS_VALU"]["mean_per_dispatch"]
                    clock = der.get("shader_clock_GHz", 2.4)
                    lane_peak = der["render_kernel_avg_ms"] * 1e-3 * clock * 1e9 * 1024 * 32      # 1024 SIMDs x 32 lanes per clock
                    executed = {"source": f"{rel} (rocprofv3 --pmc passes of this command; kernel {der['render_kernel_avg_ms']:.2f} ms under the profiler)",
                                "SQ_INSTS_VALU": insts, "lane_slots": insts * 64,
                                "lane_utilisation": round(der.get("valu_lane_utilisation", 0.0), 4),
                                "issue_fraction_of_lane_peak": round(insts * 64 / lane_peak, 4),
                                "live_lane_fraction_of_lane_peak": round(insts * 64 * der.get("valu_lane_utilisation", 0.0) / lane_peak, 4),
                                "valu_issues_per_cycle_per_simd": round(der.get("valu_issues_per_cycle_per_simd", 0.0), 4)}
        out = {
            "metric": "Msamples/s (rays x bounces) at 1920x1080x500spp",
            "value": round(seg / elapsed / 1e6, 3), "unit": "Msamples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload + ", "
                                   f"{W}x{H}, {p.samples} spp (render_row sampler), depth {p.depth}, gradient sky, render seed 1; "
                                   "rows in interleaved 8-row blocks per GPU + " +
                                   ("rtw_mgpu (one process, strided peer copies into GPU 0's frame)" if single_process_multi else "one RCCL gather"),
                       "accel": args.accel, "camera_msamples_per_s": round(rays / elapsed / 1e6, 3),
                       "segments_per_camera_ray": round(seg / max(rays, 1), 4)},
            "roofline": {"bound": "valu", "achieved": round(achieved, 4), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(achieved / PEAK_TFLOPS, 5), "traffic": traffic, "traffic_source": traffic_source,
                         "executed_valu": executed, **({"stale_profile": stale} if stale else {}),
                         "kernel": "rtw::render_%s + rtw::resolve_kernel (timed together: HIP events around both)" % args.accel,
                         "kernel_ms": round(k_s * 1e3, 3),
                         "algorithmic_flop_per_launch": flop,
                         "scheduler_census_rank0": {n: {"wave_steps": steps3[k] // args.steps,
                                                            "simd_efficiency": round(lanes3[k] / max(1, 64 * steps3[k]), 4)}
                                                        for k, n in enumerate(("traverse", "leaf", "shade", "switch", "new_path")) if steps3[k]},
                         "units_per_launch": {"segments": seg / args.steps / world, "node_visits": nodes / args.steps / world,
                                              "sphere_tests": tests / args.steps / world},
                         "hbm": {"achieved": round((H * W * 12 + rays / args.steps * 24) / world / k_s / 1e9, 3), "peak": 8000.0, "unit": "GB/s",
                                 "framebuffer_bytes": H * W * 12 / world,
                                 "sample_bank_bytes": rays / args.steps * 24 / world,
                                 "note": "algorithmic bytes per launch: framebuffer 12 B/pixel (what SURVEY 8d counts) + the builder's own per-sample "
                                         "bank, 12 B per camera ray written by the render kernel and read back by the in-order resolve; "
                                         "the path is not HBM-bound"}},
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(R, scene, cam, p)
        assert frame is not None and bool(torch.isfinite(frame).all())
        if args.dump_outputs:
            import numpy as np
            os.makedirs(args.dump_outputs, exist_ok=True)
            np.save(os.path.join(args.dump_outputs, "frame.npy"), frame.cpu().numpy().astype(np.float32))
            np.save(os.path.join(args.dump_outputs, "counters.npy"), np.array(last, dtype=np.float64))
        print(json.dumps(out), flush=True)
    r.close()
    if world > 1 and not single_process_multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
