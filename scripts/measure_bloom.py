#!/usr/bin/env python3
"""Bloom's numbers for DESIGN.md 8k and profiles/bloom.log.  Needs the GPU (but for --from-trace).

  (a) filter_ms (hipEvent, first launch to last) of Renderer.bloom at 1920 x 1080 for levels 1, 3, 6 and 8 under RTW_OPT_ATROUS_LAYOUT 0 (as
      shipped), 1 (LDS tiles) and 2 (global memory), device tensors, alternated in one process with Renderer.display (sRGB, RGB8) and one
      a-trous level as yardsticks: per variant the median of the rounds' medians and the range of all calls.
  (b) "a frame on the device to bytes on the host": DisplayTransform.step with bloom against without (host clock around the blocking calls),
      and the path a user had before: the f32 frame copied to the host, the numpy restatement of the same pyramid there
      (tests/bloom_common.py), and display.
  (c) the host form's largest |f32 - float64| beside its bound (tests/bloom_common.py), on the CPU tests' frames.
  (d) per launch, from a kernel trace taken in a run of its own:
          rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/measure_bloom.py --trace-workload
          python scripts/measure_bloom.py --from-trace DIR --out profiles/bloom.log --append
      the workload makes CALLS calls at 8 levels under layout 1, then under layout 2; --from-trace finds the bloom launches in the trace,
      takes them in the order of a call (8 down, 7 up, the composite) and prints per launch the median time from the tile and from global
      memory beside the HBM time of the launch's bytes, the share of the two full-size launches, and what the 2 n - 2 small ones cost.

    python scripts/measure_bloom.py [rounds] [--out profiles/bloom.log]
"""
import csv
import glob
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
HBM_GBS = 8000.0                                       # MI355X peak HBM3E bandwidth, GB/s, as the other sections use
CALLS = 20                                             # calls a round
TRACE_LEVELS = 8
LINES = []
LAYOUT_NAMES = {0: "as shipped", 1: "tile", 2: "global"}


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def save(out, append=False):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a" if append else "w") as f:
            f.write("\n".join(LINES) + "\n")


def alternate(variants, rounds, calls=CALLS):
    """variants: {name: call returning ms}.  `rounds` rounds, each running every variant in turn for `calls` calls after a warm-up call.
    {name: (median of the rounds' medians, min of all calls, max of all calls)}."""
    meds, lo, hi = {k: [] for k in variants}, {}, {}
    for _ in range(rounds):
        for k, call in variants.items():
            call()
            ms = [call() for _ in range(calls)]
            meds[k].append(float(np.median(ms)))
            lo[k], hi[k] = min(lo.get(k, ms[0]), min(ms)), max(hi.get(k, ms[0]), max(ms))
    return {k: (float(np.median(meds[k])), lo[k], hi[k]) for k in variants}


def fmt(t):
    return f"{t[0]:7.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


def hbm_ms(n_bytes):
    return n_bytes / (HBM_GBS * 1e9) * 1e3


def test_frame():
    """A 1080p frame over 22 stops with emitters 40 times their surroundings (tests/bloom_common.noise)."""
    from tests.bloom_common import noise
    return noise(W, H)


def launch_bytes(w, h, levels):
    """[(name, output pixels, bytes read + written)] of a call's launches in their order."""
    import rtw_amd as R
    sizes = [(w, h)] + R.bloom_levels(w, h, levels)
    px = [a * b for a, b in sizes]
    n = len(sizes) - 1
    rows = [(f"down {l} -> {l + 1} ({sizes[l + 1][0]} x {sizes[l + 1][1]})", px[l + 1], 12 * (px[l] + px[l + 1])) for l in range(n)]
    rows += [(f"up {l + 1} -> {l} ({sizes[l][0]} x {sizes[l][1]})", px[l], 12 * (px[l + 1] + 2 * px[l])) for l in range(n - 1, 0, -1)]
    rows.append((f"composite ({w} x {h})", px[0], 12 * (px[1] + 2 * px[0])))
    return rows


def call_rows(gpu, torch, R, frame, rounds):
    dev = torch.device("cuda:0")
    t = torch.from_numpy(frame).to(dev)
    out, out8 = torch.empty_like(t), torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    log(f"# (a) bloom filter_ms at {W} x {H}, device tensors, BLOOM_DEFAULTS but for levels: median of {rounds} rounds' medians of {CALLS} calls, "
        f"variants alternated (min .. max of all calls)")

    def bloom_ms(layout, levels):
        gpu.set_option(R.OPT_ATROUS_LAYOUT, layout)
        return gpu.bloom(t, out=out, levels=levels)[2].filter_ms

    def atrous_ms():
        gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)
        return gpu.atrous_filter(t, levels=1, out=out)[1].filter_ms

    variants = {("bloom", la, lv): (lambda la=la, lv=lv: bloom_ms(la, lv)) for lv in (1, 3, 6, 8) for la in (0, 1, 2)}
    variants[("display",)] = lambda: gpu.display(t, out=out8, transfer=R.TRANSFER_SRGB, out_format=R.DISPLAY_RGB8)[1].filter_ms
    variants[("atrous",)] = atrous_ms
    want = {lv: R.bloom(frame, levels=lv)[0] for lv in (1, 8)}
    for la in (0, 1, 2):
        for lv in (1, 8):
            bloom_ms(la, lv)
            assert np.array_equal(out.cpu().numpy(), want[lv]), (la, lv)         # the bytes of the host form under every layout
    res = alternate(variants, rounds)
    for lv in (1, 3, 6, 8):
        rows = launch_bytes(W, H, lv)
        floor = hbm_ms(sum(b for _, _, b in rows))
        log(f"  levels {lv} ({len(rows)} launches)   " + "   ".join(f"{LAYOUT_NAMES[la]} {fmt(res[('bloom', la, lv)])}" for la in (0, 1, 2))
            + f"   HBM time of all launches' bytes {floor:.4f} ms = {100 * floor / res[('bloom', 0, lv)][0]:4.1f} % of the shipped")
    log(f"  Renderer.display, sRGB, RGB8             {fmt(res[('display',)])}")
    log(f"  Renderer.atrous_filter, one level        {fmt(res[('atrous',)])}")
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)


def end_to_end(gpu, torch, R, frame, rounds):
    from tests.bloom_common import restate_bloom
    dev = torch.device("cuda:0")
    t = torch.from_numpy(frame).to(dev)
    out = np.empty((H, W, 3), np.uint8)
    log(f"# (b) a frame on the device to bytes on the host, {W} x {H}, host clock, median of {rounds} rounds' medians of {CALLS} calls (min .. max)")
    plain, bloomed = R.DisplayTransform(gpu), R.DisplayTransform(gpu, bloom={})

    def step(dt):
        t0 = time.perf_counter()
        dt.step(t, out=out)
        return (time.perf_counter() - t0) * 1e3

    res = alternate({"plain": lambda: step(plain), "bloom": lambda: step(bloomed)}, rounds)
    log(f"  DisplayTransform.step (histogram, metering, display)             {fmt(res['plain'])}")
    log(f"  DisplayTransform(bloom=BLOOM_DEFAULTS).step                      {fmt(res['bloom'])}   the bloom adds {res['bloom'][0] - res['plain'][0]:.4f} ms")
    e = np.float32(bloomed.exposure)
    prm = dict(R.BLOOM_DEFAULTS, threshold=float(np.float32(1.0) / e), knee=float(np.float32(0.5) / e))
    parts = {}

    def old_path():
        t0 = time.perf_counter()
        host = t.cpu().numpy()
        t1 = time.perf_counter()
        b = restate_bloom(host, **prm)[0]
        t2 = time.perf_counter()
        old_path.bytes = R.display(b, exposure=float(e))[0]
        t3 = time.perf_counter()
        for k, v in (("copy", t1 - t0), ("numpy pyramid", t2 - t1), ("display (host form)", t3 - t2)):
            parts.setdefault(k, []).append(v * 1e3)
        return (t3 - t0) * 1e3

    old = [old_path() for _ in range(3)]
    log(f"  f32 copy to the host, the pyramid in numpy, display (3 calls)    {np.median(old):9.1f} ms ({min(old):.1f} .. {max(old):.1f})   of which, medians: "
        + ", ".join(f"{k} {np.median(v):.1f} ms" for k, v in parts.items()))
    log(f"  ratio of the medians: {np.median(old) / res['bloom'][0]:.0f} x;  bytes that differ between the two: {int((out != old_path.bytes).sum())}")


def f64_rows():
    import rtw_amd as R
    from tests.bloom_common import PARAM_SETS, bloom_bound, noise
    log("# (c) the host form against the float64 rule, noise frames of tests/bloom_common.py, 8 levels: largest |f32 - f64| of out and of the layer, the "
        "bound at that pixel, and the largest error / bound over all pixels")
    for size in ((5, 3), (33, 33), (65, 35), (64, 48)):
        frame = noise(*size)
        for ps in PARAM_SETS:
            prm = dict(levels=8, spread=0.5, intensity=0.25, **ps)
            out, layer, _ = R.bloom(frame, layer=True, **prm)
            o64, l64, bo, bl = bloom_bound(frame, **prm)
            eo, el = np.abs(out - o64), np.abs(layer - l64)
            with np.errstate(all="ignore"):
                ratio = max(np.nanmax(np.where(bo > 0, eo / bo, 0.0)), np.nanmax(np.where(bl > 0, el / bl, 0.0)))
            log(f"  {size[0]:>3} x {size[1]:<3} karis {int(ps['karis'])} threshold {ps['threshold']:<5} knee {ps['knee']:<5} out {eo.max():.3e} (bound {bo.flat[eo.argmax()]:.3e})   "
                f"layer {el.max():.3e} (bound {bl.flat[el.argmax()]:.3e})   largest error / bound {ratio:.3f}")


def trace_workload():
    import torch
    import rtw_amd as R
    frame = test_frame()
    with R.Renderer(0) as gpu:
        t = torch.from_numpy(frame).to("cuda:0")
        out = torch.empty_like(t)
        for layout in (1, 2):
            gpu.set_option(R.OPT_ATROUS_LAYOUT, layout)
            for _ in range(CALLS + 2):
                gpu.bloom(t, out=out, levels=TRACE_LEVELS)


def from_trace(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {trace_dir}"
    rows = []
    for name in files:
        with open(name, newline="") as f:
            for r in csv.DictReader(f):
                m = re.search(r"bloom_(down|up)_kernel<\s*(true|false)\s*,\s*(true|false)\s*>", r["Kernel_Name"])
                if m:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(1), m.group(2) == "true", m.group(3) == "true"))
    rows.sort()
    plan = launch_bytes(W, H, TRACE_LEVELS)
    per_call = len(plan)
    assert rows and len(rows) % per_call == 0, (len(rows), per_call)
    times = {True: [[] for _ in plan], False: [[] for _ in plan]}             # by tile, by launch of the call
    gaps = {True: [], False: []}
    for c in range(len(rows) // per_call):
        call = rows[c * per_call:(c + 1) * per_call]
        tile = call[0][4]
        assert all(r[4] == tile for r in call) and [r[2] for r in call] == ["down"] * TRACE_LEVELS + ["up"] * TRACE_LEVELS, c
        assert call[0][3] and call[-1][3] and not any(r[3] for r in call[1:-1]), c     # FIRST, ..., COMPOSITE
        for k, r in enumerate(call):
            times[tile][k].append((r[1] - r[0]) * 1e-6)
        gaps[tile].append(((call[-1][1] - call[0][0]) - sum(r[1] - r[0] for r in call)) * 1e-6)
    med = {tile: [float(np.median(v[2:])) for v in times[tile]] for tile in (True, False)}     # (the first two calls of a layout warm up)
    log(f"# (d) per launch at {W} x {H}, {TRACE_LEVELS} levels, from a kernel trace ({len(times[True][0]) - 2} + {len(times[False][0]) - 2} calls): median kernel time "
        f"from the LDS tile and from global memory, and the HBM time of the launch's bytes at {HBM_GBS:.0f} GB/s")
    for k, (name, px, nb) in enumerate(plan):
        a, b = med[True][k], med[False][k]
        log(f"  {name:<34}{px:>9} px   tile {a:.4f} ms   global {b:.4f} ms   {'tile' if a < b else 'global'} ahead by {100 * abs(a - b) / max(a, b):4.1f} %   "
            f"HBM {hbm_ms(nb):.5f} ms = {100 * hbm_ms(nb) / min(a, b):4.1f} % of the faster")
    for tile in (True, False):
        m = med[tile]
        big, small = m[0] + m[-1], sum(m[1:-1])
        floor = hbm_ms(plan[0][2] + plan[-1][2])
        log(f"  {'tile' if tile else 'global'}: the first down step and the composite {big:.4f} ms (HBM time of their bytes {floor:.4f} ms = {100 * floor / big:.1f} %), "
            f"the {per_call - 2} small launches {small:.4f} ms, all kernels {big + small:.4f} ms; between the kernels of a call (median) {np.median(gaps[tile][2:]):.4f} ms")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if "--trace-workload" in sys.argv:
        return trace_workload()
    if "--from-trace" in sys.argv:
        from_trace(sys.argv[sys.argv.index("--from-trace") + 1])
        return save(out, append="--append" in sys.argv)
    args = [a for a in args if a != out]
    rounds = max(5, int(args[0])) if args else 5
    import torch                                       # before the first rtw call: the library then shares the HIP runtime torch loaded (tests/conftest.py)
    import rtw_amd as R
    assert R.device_count() > 0, "measure_bloom.py needs the MI355X"
    frame = test_frame()
    with R.Renderer(0) as gpu:
        log(f"# bloom, {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} compute units; one thread an output pixel, "
            f"workgroups of 16 x 16")
        call_rows(gpu, torch, R, frame, rounds)
        save(out)
        end_to_end(gpu, torch, R, frame, rounds)
        save(out)
    f64_rows()
    save(out)


if __name__ == "__main__":
    main()
