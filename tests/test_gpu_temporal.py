"""Temporal accumulation on the GPU (rtw_ctx_temporal_accumulate, csrc/rtw_temporal.hip) against the host form, bit for bit (as
tests/temporal_common.py defines it: the same bits, or NaN on both sides): the CPU tests' cases at their four sizes -- 33 x 17 and 67 x 35
cross the 32 x 8 workgroup in both directions -- with numpy arrays and with torch tensors in place, out_color == cur, two sizes in a row on
one context, the refusals, and two rendered sequences: a static camera, whose accumulation is the running mean of its frames bit for bit,
and a small orbit through TemporalDenoiser.  The host form itself is held to a numpy restatement by tests/test_temporal_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.temporal_common import (CASE_NAMES, F, OFFSET, OUT_KEYS, SENTINEL, SHAPES, assert_same_runs, cases, host_answer, mismatch, orbit, raw_call,
                                   refusal_calls, run, same_bits)
from tests.test_gpu_stream_order import torch  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
shape_ids = lambda s: f"{s[1]}x{s[0]}"


# ---- 1. the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_device_equals_host_numpy(gpu, shape):
    h, w = shape
    for name in CASE_NAMES:
        frames, params = cases(h, w)[name]
        assert_same_runs(run(gpu.temporal_accumulate, frames, params), host_answer(h, w, name), name)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_ids)
def test_device_equals_host_tensors_in_place(gpu, torch, shape):
    """Every buffer a tensor on the context's device: read in place, results written straight into new tensors."""
    h, w = shape
    wrap = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
    for name in CASE_NAMES:
        frames, params = cases(h, w)[name]
        assert_same_runs(run(gpu.temporal_accumulate, frames, params, wrap=wrap), host_answer(h, w, name), name)


def test_tensors_passed_as_history_are_unchanged(gpu, torch):
    h, w = 35, 67
    frames, params = cases(h, w)["terms-all"]
    wrap = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
    f0, f1 = frames
    hist, _, _ = gpu.temporal_accumulate(wrap(f0["cur"]), f0["cam"], depth=wrap(f0["depth"]), normal=wrap(f0["normal"]), ids=wrap(f0["idx"]),
                                         offset=OFFSET, **params)
    assert all(hasattr(hist[k], "data_ptr") for k in ("color", "moments", "len"))
    before = {k: v.clone() for k, v in hist.items() if k != "cam"}
    cur = wrap(f1["cur"])
    new, var, st = gpu.temporal_accumulate(cur, f1["cam"], depth=wrap(f1["depth"]), normal=wrap(f1["normal"]), ids=wrap(f1["idx"]), history=hist,
                                           offset=OFFSET, **params)
    for k, v in before.items():
        assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v, hist[k].view(torch.int32) if v.dtype == torch.float32 else hist[k]), k
    assert same_bits(cur.cpu().numpy(), f1["cur"])                                   # (cur is only read, too)
    want = host_answer(h, w, "terms-all")[1]
    assert same_bits(new["color"].cpu().numpy(), want["color"]) and same_bits(var.cpu().numpy(), want["variance"])
    assert st.filter_ms > 0.0 and st.taps == 4 * h * w


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_out_color_may_be_cur(gpu, torch, device):
    h, w = 35, 67
    frames, params = cases(h, w)["turned"]
    want = host_answer(h, w, "turned")
    wrap = (lambda a: torch.from_numpy(np.array(a)).to("cuda:0")) if device else (lambda a: a)
    hist = None
    for fr, x in zip(frames, want):
        cur = wrap(fr["cur"].copy())
        hist, var, _ = gpu.temporal_accumulate(cur, fr["cam"], depth=wrap(fr["depth"]), normal=wrap(fr["normal"]), ids=wrap(fr["idx"]), history=hist,
                                               out_color=cur, offset=OFFSET, **params)
        assert hist["color"] is cur
        got = cur.cpu().numpy() if device else cur
        assert same_bits(got, x["color"]), mismatch(got, x["color"])


def test_two_sizes_in_a_row_on_one_context():
    """The scratch grown by the larger frame serves the smaller one, and grows again."""
    with R.Renderer(0) as other:
        for h, w in ((17, 33), (35, 67), (3, 5), (35, 67)):
            frames, params = cases(h, w)["terms-all"]
            assert_same_runs(run(other.temporal_accumulate, frames, params), host_answer(h, w, "terms-all"), (h, w))


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_unwritten(gpu):
    call = R.lib().rtw_ctx_temporal_accumulate
    for name, change in refusal_calls():
        rc, outs, _ = raw_call(call, (gpu._h,), **change)
        assert rc == -1, name
        assert all(np.all(o == SENTINEL) for o in outs), name
    rc, outs, _ = raw_call(call, (None,))
    assert rc == -1 and all(np.all(o == SENTINEL) for o in outs)
    rc, outs, _ = raw_call(call, (gpu._h,))                                          # the call they all start from is accepted
    want = raw_call(R.lib().rtw_temporal_accumulate)[1]
    assert rc == 0 and all(same_bits(a, b) for a, b in zip(outs, want))
    rc, outs, _ = raw_call(call, (gpu._h,), out_variance=None)
    assert rc == 0 and np.all(outs[3] == SENTINEL) and same_bits(outs[0], want[0])


# ---- 3. rendered sequences ---------------------------------------------------------------------------------------------------------------
W, H = 64, 36


@pytest.fixture(scope="module")
def book1(gpu):
    from tests.test_oracle_golden import small_view
    scene, cam, p = small_view(R.SCENE_C2, W, H, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    return scene, cam, p


def test_rendered_static_accumulation_is_the_running_mean(gpu, book1):
    """8 frames of 4 spp with distinct seeds under a static camera, alpha 0, max_history 8: the accumulated frame is the numpy running mean
    of the 8 frames bit for bit, and -- the mean of 8 independent frames -- closer to a 1024-spp render than the first frame alone.
    The depth and id tests are on and pass everywhere (a pixel meets its own guides); the normal test is off: a miss has the normal
    (0, 0, 0), whose product with itself is below any normal_cos, so with that test on the background starts again in every frame
     -- asserted at the end."""
    _, cam, p = book1
    p.samples, p.seed = 1024, 99
    truth = gpu.render(cam, p)[0].astype(np.float64)
    p.samples = 4
    g = gpu.surface_map(cam, W, H, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, OFFSET)
    hist, mean, first = None, None, None
    for n in range(1, 9):
        p.seed = n
        cur = gpu.render(cam, p)[0]
        assert np.all(np.isfinite(cur))
        hist, var, _ = gpu.temporal_accumulate(cur, cam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist, alpha=0.0,
                                               alpha_moments=0.0, max_history=8, depth_tol=0.05, normal_cos=0.0, same_object=1, offset=OFFSET)
        mean = cur if n == 1 else mean + (cur - mean) * (F(1) / F(n))
        first = cur if n == 1 else first
        assert same_bits(hist["color"], mean), (n, mismatch(hist["color"], mean))
        assert np.all(hist["len"] == n)
    one, acc = float(((first - truth) ** 2).mean()), float(((hist["color"] - truth) ** 2).mean())
    print(f"\n[temporal, static] MSE of frame 1 {one:.6f}, of 8 accumulated {acc:.6f}, ratio {acc / one:.3f}")
    assert acc < one, (one, acc)
    again = gpu.temporal_accumulate(cur, cam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist, alpha=0.0, alpha_moments=0.0,
                                    max_history=8, depth_tol=0.05, normal_cos=0.9, same_object=1, offset=OFFSET)[0]
    miss = g["idx"] < 0
    assert miss.any() and np.all(again["len"][miss] == 1) and np.all(again["len"][~miss & (np.abs(g["normal"]).sum(-1) > 0.99)] == 8)


def test_rendered_camera_move_through_the_denoiser(gpu, book1):
    """Three cameras along a small orbit through TemporalDenoiser.step: after a move some pixels keep their history and some lose it, and
    every output equals the host form run on the same rendered inputs."""
    _, cam, p = book1
    p.samples, p.seed = 4, 20
    den = R.TemporalDenoiser(gpu, alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1)
    hist_host = None
    for k, deg in enumerate((0.0, 1.0, 2.0)):
        c = orbit(cam, deg)
        frame, acc, var, st = den.step(c, p)
        assert p.seed == 21 + k and p.gamma == 1.0
        g = st["guides"]
        hist_host, var_host, _ = R.temporal_accumulate(st["cur"], c, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist_host,
                                                       alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1,
                                                       offset=OFFSET)
        for key in ("color", "moments", "len"):
            assert same_bits(den.history[key], hist_host[key]), (k, key, mismatch(den.history[key], hist_host[key]))
        assert same_bits(var, var_host) and acc is den.history["color"]
        cover = float((den.history["len"] > 1).mean())
        assert st["coverage"] == cover
        if k == 0:
            assert cover == 0.0
        else:
            assert 0.0 < cover < 1.0, (k, cover)
        want = gpu.atrous_filter(acc, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"])[0]
        assert same_bits(frame, want) and frame.shape == (H, W, 3)
    den.reset()
    assert den.history is None
    assert den.step(cam, p)[3]["coverage"] == 0.0
