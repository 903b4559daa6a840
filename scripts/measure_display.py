#!/usr/bin/env python3
"""The display stage's numbers for DESIGN.md 8j and profiles/display.log.  Needs the GPU.

  (a) filter_ms (hipEvent) of luminance_histogram at 1920 x 1080 on white noise, a constant frame and the Book-1 4-spp frame under
      RTW_OPT_HISTOGRAM_COUNT 1 (plain LDS atomics), 2 (a histogram a wave) and 3 (ballot), alternated in one process: per variant the
      median of the rounds' medians and the range of all calls, beside the time of the frame's bytes at the peak HBM rate.
  (b) filter_ms of display per out_format and per tone curve, dither off and on (sRGB, RUST), and for the transfer alone (gamma 1, gamma
      2.2, sRGB without a curve); beside the HBM time of the bytes read and written.
  (c) "a filtered frame on the device to bytes on the host": Renderer.display of a device tensor into a numpy array (host clock around the
      blocking call) against the path before it: the f32 frame copied to the host, np.power(np.maximum(x, 0), 1 / gamma), quantize_u8;
      the same frame, the same gamma, the same process.  The two give the same bytes but where pow_plain and numpy's power round apart.
  (d) the largest |F32 output - float64 reference| per curve and transfer with its bound (tests/test_display_cpu.py), on the host form.

    python scripts/measure_display.py [rounds] [--out profiles/display.log]
"""
import os
import sys
import time

import numpy as np

import torch                                           # before the first rtw call: the library then shares the HIP runtime torch loaded (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtw_amd as R                                    # noqa: E402

W, H = 1920, 1080
HBM_GBS = 8000.0                                       # MI355X peak HBM3E bandwidth, GB/s
CALLS = 20                                             # calls a round
LINES = []
COUNT_NAMES = {1: "plain", 2: "per wave", 3: "ballot"}
TONE_NAMES = {R.TONE_NONE: "none", R.TONE_REINHARD: "reinhard", R.TONE_REINHARD_LUMA: "reinhard luma", R.TONE_ACES_FIT: "aces fit"}
FORMAT_NAMES = {R.DISPLAY_RGB8: "rgb8", R.DISPLAY_RGBA8: "rgba8", R.DISPLAY_F32: "f32"}
OUT_BYTES = {R.DISPLAY_RGB8: 3, R.DISPLAY_RGBA8: 4, R.DISPLAY_F32: 12}


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def save(out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


def alternate(variants, rounds):
    """variants: {name: call returning ms}.  `rounds` rounds, each running every variant in turn for CALLS calls after a warm-up call.
    {name: (median of the rounds' medians, min of all calls, max of all calls)}."""
    meds, lo, hi = {k: [] for k in variants}, {}, {}
    for _ in range(rounds):
        for k, call in variants.items():
            call()
            ms = [call() for _ in range(CALLS)]
            meds[k].append(float(np.median(ms)))
            lo[k], hi[k] = min(lo.get(k, ms[0]), min(ms)), max(hi.get(k, ms[0]), max(ms))
    return {k: (float(np.median(meds[k])), lo[k], hi[k]) for k in variants}


def fmt(t):
    return f"{t[0]:7.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


def book1_frame(gpu):
    from tests.test_oracle_golden import small_view
    scene, cam, p = small_view(R.SCENE_C2, W, H, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    return gpu.render(cam, p)[0]


def histogram_rows(gpu, frames, rounds):
    dev = torch.device("cuda:0")
    floor_ms = 12 * W * H / (HBM_GBS * 1e9) * 1e3
    log(f"# (a) luminance_histogram filter_ms at {W} x {H}, device tensors: median of {rounds} rounds' medians of {CALLS} calls, variants alternated (min .. max of all calls)")
    log(f"#     HBM time of the frame's {12 * W * H / 1e6:.1f} MB at {HBM_GBS:.0f} GB/s: {floor_ms:.4f} ms")
    wins = {}
    for name, frame in frames.items():
        t = torch.from_numpy(frame).to(dev)
        hist = torch.zeros(256, dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        want = R.luminance_histogram(frame)

        def call(v):
            gpu.set_option(R.OPT_HISTOGRAM_COUNT, v)
            return gpu.luminance_histogram(t, out_hist=hist, out_counts=counts)[2].filter_ms

        for v in COUNT_NAMES:
            call(v)
            assert np.array_equal(hist.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(counts.cpu().numpy().view(np.uint32), want[1]), (name, v)
        res = alternate({v: (lambda v=v: call(v)) for v in COUNT_NAMES}, rounds)
        best = min(res, key=lambda v: res[v][0])
        wins[name] = best
        log(f"  {name:<14}" + "   ".join(f"{COUNT_NAMES[v]} {fmt(res[v])}" for v in COUNT_NAMES)
            + f"   HBM {100 * floor_ms / res[best][0]:4.1f} % of the fastest ({COUNT_NAMES[best]}); occupied bins {int(np.count_nonzero(want[0]))}")
    gpu.set_option(R.OPT_HISTOGRAM_COUNT, 0)
    log(f"#     fastest by frame: " + ", ".join(f"{k}: {COUNT_NAMES[v]}" for k, v in wins.items()))


def display_rows(gpu, frame, rounds):
    dev = torch.device("cuda:0")
    t = torch.from_numpy(frame).to(dev)
    log(f"# (b) display filter_ms at {W} x {H} on the Book-1 frame, device tensors, sRGB, RUST, exposure 1: median of {rounds} rounds' medians of {CALLS} calls (min .. max)")
    log(f"#     HBM = the time of the bytes read (12 a pixel) and written (3, 4 or 12 a pixel) at {HBM_GBS:.0f} GB/s")
    outs = {R.DISPLAY_RGB8: torch.empty((H, W, 3), dtype=torch.uint8, device=dev), R.DISPLAY_RGBA8: torch.empty((H, W, 4), dtype=torch.uint8, device=dev),
            R.DISPLAY_F32: torch.empty((H, W, 3), dtype=torch.float32, device=dev)}
    for f, out in outs.items():
        floor_ms = (12 + OUT_BYTES[f]) * W * H / (HBM_GBS * 1e9) * 1e3
        variants = {}
        for tone in TONE_NAMES:
            for dither in ((False,) if f == R.DISPLAY_F32 else (False, True)):
                prm = dict(tone=tone, white=4.0, transfer=R.TRANSFER_SRGB, quantise=R.QUANTISE_RUST, dither=dither, out_format=f)
                variants[(tone, dither)] = lambda prm=prm, out=out: gpu.display(t, out=out, **prm)[1].filter_ms
        res = alternate(variants, rounds)
        for (tone, dither), r in res.items():
            log(f"  {FORMAT_NAMES[f]:<6}{TONE_NAMES[tone]:<14}{'dither' if dither else 'no dither':<10}{fmt(r)}   HBM {floor_ms:.4f} ms = {100 * floor_ms / r[0]:4.1f} %")
    out = outs[R.DISPLAY_RGB8]
    floor_ms = 15 * W * H / (HBM_GBS * 1e9) * 1e3
    variants = {name: (lambda prm=prm: gpu.display(t, out=out, tone=R.TONE_NONE, out_format=R.DISPLAY_RGB8, **prm)[1].filter_ms)
                for name, prm in (("gamma 1 (no pow_plain)", dict(transfer=R.TRANSFER_GAMMA, gamma=1.0)), ("gamma 2.2", dict(transfer=R.TRANSFER_GAMMA, gamma=2.2)),
                                  ("sRGB", dict(transfer=R.TRANSFER_SRGB)))}
    for name, r in alternate(variants, rounds).items():
        log(f"  rgb8  none, {name:<24}{fmt(r)}   HBM {floor_ms:.4f} ms = {100 * floor_ms / r[0]:4.1f} %")
    # the scalar path: the same frame one pixel into an allocation (12 bytes off 16-byte alignment), and an RGB8 output one byte in
    base = torch.zeros(frame.size + 3, dtype=torch.float32, device=dev)
    off = base[3:].view(H, W, 3)
    off.copy_(t)
    odd = torch.zeros(H * W * 3 + 1, dtype=torch.uint8, device=dev)[1:].view(H, W, 3)
    prm = dict(tone=R.TONE_ACES_FIT, transfer=R.TRANSFER_SRGB, out_format=R.DISPLAY_RGB8)
    res = alternate({"aligned (four pixels a thread)": lambda: gpu.display(t, out=out, **prm)[1].filter_ms,
                     "in 12 bytes off (a pixel a thread)": lambda: gpu.display(off, out=out, **prm)[1].filter_ms,
                     "out 1 byte off (a pixel a thread)": lambda: gpu.display(t, out=odd, **prm)[1].filter_ms}, rounds)
    for name, r in res.items():
        log(f"  rgb8  aces fit, {name:<36}{fmt(r)}")
    gpu.set_option(R.OPT_HISTOGRAM_COUNT, 0)
    hist = torch.zeros(256, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    res = alternate({"aligned": lambda: gpu.luminance_histogram(t, out_hist=hist, out_counts=counts)[2].filter_ms,
                     "in 12 bytes off": lambda: gpu.luminance_histogram(off, out_hist=hist, out_counts=counts)[2].filter_ms}, rounds)
    for name, r in res.items():
        log(f"  luminance_histogram (the shipped choice), {name:<18}{fmt(r)}")


def end_to_end(gpu, frame, rounds):
    dev = torch.device("cuda:0")
    t = torch.from_numpy(frame).to(dev)
    gamma = 2.0
    log(f"# (c) a filtered frame on the device to bytes on the host, {W} x {H}, gamma {gamma}, host clock, median of {rounds} rounds' medians of {CALLS} calls (min .. max)")
    out = np.empty((H, W, 3), np.uint8)

    def new_path():
        t0 = time.perf_counter()
        gpu.display(t, out=out, tone=R.TONE_NONE, transfer=R.TRANSFER_GAMMA, gamma=gamma, quantise=R.QUANTISE_RUST, out_format=R.DISPLAY_RGB8)
        return (time.perf_counter() - t0) * 1e3

    parts = {}

    def old_path():
        t0 = time.perf_counter()
        host = t.cpu().numpy()
        t1 = time.perf_counter()
        g = np.power(np.maximum(host, np.float32(0.0)), np.float32(1.0 / gamma)).astype(np.float32)
        t2 = time.perf_counter()
        old_path.bytes = R.quantize_u8(g)
        t3 = time.perf_counter()
        for k, v in (("copy", t1 - t0), ("np.power", t2 - t1), ("quantize_u8", t3 - t2)):
            parts.setdefault(k, []).append(v * 1e3)
        return (t3 - t0) * 1e3

    res = alternate({"new": new_path, "old": old_path}, rounds)
    log(f"  Renderer.display (device tensor -> numpy uint8 [h][w][3])        {fmt(res['new'])}")
    log(f"  f32 copy to the host, np.power, quantize_u8 (the path before)    {fmt(res['old'])}   of which, medians: "
        + ", ".join(f"{k} {np.median(v):.3f} ms" for k, v in parts.items()))
    log(f"  ratio of the medians: {res['old'][0] / res['new'][0]:.1f} x")
    diff = np.abs(out.astype(np.int16) - old_path.bytes.astype(np.int16))
    log(f"  bytes that differ between the two (pow_plain against numpy's power): {int((diff != 0).sum())} of {diff.size}, largest difference {int(diff.max())}")


def f64_rows():
    from tests.test_display_cpu import observed_f64_errors
    log("# (d) the host form's F32 output against the float64 reference, noise frames of tests/display_common.py: largest |f32 - f64| and the bound")
    for (tone, transfer, gamma), (worst, bound) in observed_f64_errors().items():
        log(f"  {TONE_NAMES[tone]:<14}{'sRGB' if transfer == R.TRANSFER_SRGB else f'gamma {gamma}':<10}  {worst:.3e}   bound {bound:.3e}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = max(5, int(args[0])) if args else 5
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    assert R.device_count() > 0, "measure_display.py needs the MI355X"
    rng = np.random.default_rng(1)
    with R.Renderer(0) as gpu:
        book1 = book1_frame(gpu)
        frames = {"white noise": np.exp2(rng.uniform(-16.0, 16.0, (H, W, 3))).astype(np.float32),
                  "constant 0.18": np.full((H, W, 3), 0.18, np.float32), "Book-1 4 spp": book1}
        log(f"# display stage, {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} compute units; "
            f"histogram grid at most {R.HISTOGRAM_BLOCKS_PER_CU} workgroups of 256 threads a unit")
        histogram_rows(gpu, frames, rounds)
        save(out)
        display_rows(gpu, book1, rounds)
        save(out)
        end_to_end(gpu, book1, rounds)
        save(out)
    f64_rows()
    save(out)


if __name__ == "__main__":
    main()
