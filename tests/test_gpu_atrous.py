"""The a-trous filter on the GPU (rtw_ctx_atrous_filter, csrc/rtw_atrous.hip) against the host form, bit for bit (as
tests/atrous_common.py defines it: the same bits, or NaN on both sides): the CPU tests' matrix under every RTW_OPT_ATROUS_LAYOUT, strips
259 pixels long whose taps at levels 7 and 8 land inside the frame, frames
around the workgroup's 32 x 16 tile, host and device memory mixed per argument, out == in, torch tensors behind use_torch_stream, a second
context, the refusals, and the one thing asserted about quality.  The host form itself is held to a numpy restatement by
tests/test_atrous_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.atrous_common import (DEEP_LEVELS, DEEP_SHAPES, DEEP_TERM_SETS, F, FLOOR, LEVELS, SHAPES, TERM_SETS, call_kwargs, deep_answer, deep_frame,
                                 host_answer, inputs, mismatch, same_bits)
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

LAYOUTS = [0, 1, 2]                                        # the measured choice, LDS tile wherever it fits, global memory
TILE_W, TILE_H = 32, 16                                    # the kernel's workgroup (csrc/rtw_atrous.hip ABX, ABY)


@pytest.fixture()
def layout(gpu, request):
    gpu.set_option(R.OPT_ATROUS_LAYOUT, request.param)
    yield request.param
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)


# ---- 1. the matrix -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_equals_host(gpu, shape, levels, layout):
    h, w = shape
    for terms in TERM_SETS:
        got, st = gpu.atrous_filter(inputs(h, w)["frame"], **call_kwargs(h, w, terms, levels))
        want = host_answer(h, w, terms, levels)
        assert same_bits(got, want), (terms, mismatch(got, want))
        assert st.taps == R.atrous_filter(np.zeros((h, w, 3), F), levels=levels)[1].taps and st.filter_ms > 0.0


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("levels", DEEP_LEVELS)
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_equals_host_with_taps_at_levels_7_and_8(gpu, shape, levels, layout):
    """259 pixels long, so that the taps of step 64 and step 128 land inside the frame and count (tests/test_atrous_cpu.py asserts that they
    do): 1 << i, 2^-i, the choice between tile and direct reads and the parity of the two buffers at the last levels."""
    h, w = shape
    for terms in DEEP_TERM_SETS:
        got, st = gpu.atrous_filter(deep_frame(h, w), **call_kwargs(h, w, terms, levels))
        want, taps = deep_answer(h, w, terms, levels)
        assert same_bits(got, want), (terms, mismatch(got, want))
        assert st.taps == taps


# ---- 2. around the tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("h", [TILE_H - 1, TILE_H, TILE_H + 1])
@pytest.mark.parametrize("w", [TILE_W - 1, TILE_W, TILE_W + 1])
def test_frames_around_the_tile(gpu, w, h, layout):
    for terms, levels in (("all+albedo+emitted", 4), ("color", 2), ("all", 5)):
        got = gpu.atrous_filter(inputs(h, w)["frame"], **call_kwargs(h, w, terms, levels))[0]
        want = host_answer(h, w, terms, levels)
        assert same_bits(got, want), (terms, levels, mismatch(got, want))


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_many_tiles(gpu, layout):
    """3 x 5 workgroups with ragged edges; five levels: the halo of the later ones spans several neighbours, and the last does not fit a tile."""
    h, w = 4 * TILE_H + 3, 2 * TILE_W + 7
    got = gpu.atrous_filter(inputs(h, w)["frame"], **call_kwargs(h, w, "all+albedo+emitted", 5))[0]
    want = host_answer(h, w, "all+albedo+emitted", 5)
    assert same_bits(got, want), mismatch(got, want)


def test_layout_option_is_checked(gpu):
    for bad in (3, -1, 0.5, float("nan")):
        with pytest.raises(R.RtwError):
            gpu.set_option(R.OPT_ATROUS_LAYOUT, bad)


# ---- 3. memory kinds ---------------------------------------------------------------------------------------------------------------------
NAMES = ["frame", "depth", "normal", "ids", "albedo", "emitted", "out"]


@pytest.mark.parametrize("on_device", [0b0000000, 0b1111111, 0b0101010, 0b1010101, 0b1000001, 0b0111110],
                         ids=lambda m: "".join(n[0] if m >> i & 1 else "-" for i, n in enumerate(NAMES)))
def test_host_and_device_memory_mixed(gpu, torch, on_device):
    """Each argument independently a numpy array (staged) or a torch tensor (in place)."""
    h, w = 35, 67
    g = inputs(h, w)
    kw = call_kwargs(h, w, "all+albedo+emitted", 4)
    dev = torch.device("cuda:0")
    for i, name in enumerate(NAMES[:-1]):
        if on_device >> i & 1:
            t = torch.from_numpy(np.array(g[name])).to(dev)
            if name == "frame":
                frame = t
            else:
                kw[name] = t
        elif name == "frame":
            frame = g["frame"]
    out = torch.full((h, w, 3), 7.0, device=dev) if on_device >> 6 & 1 else np.full((h, w, 3), 7.0, F)
    got, _ = gpu.atrous_filter(frame, **kw, out=out)
    assert got is out
    got = out.cpu().numpy() if hasattr(out, "cpu") else out
    want = host_answer(h, w, "all+albedo+emitted", 4)
    assert same_bits(got, want), mismatch(got, want)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_out_may_be_in(gpu, torch, device):
    h, w = 35, 67
    for terms, levels in (("all+albedo+emitted", 3), ("color", 1)):
        frame = np.array(inputs(h, w)["frame"])
        if device:
            frame = torch.from_numpy(frame).to("cuda:0")
        out, _ = gpu.atrous_filter(frame, **call_kwargs(h, w, terms, levels), out=frame)
        assert out is frame
        got = frame.cpu().numpy() if device else frame
        assert same_bits(got, host_answer(h, w, terms, levels)), (terms, mismatch(got, host_answer(h, w, terms, levels)))


# ---- 4. stream order and contexts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_tensors_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """Every buffer a tensor whose producer is still pending on the caller's stream when the call is made (tests/test_gpu_stream_order.py)."""
    h, w = 35, 67
    g = inputs(h, w)
    kw = call_kwargs(h, w, "all+albedo+emitted", 4)
    want = host_answer(h, w, "all+albedo+emitted", 4)
    assert same_bits(ctx.atrous_filter(g["frame"], **kw)[0], want)       # own stream, host buffers: the scratch is as large as it gets
    hz = Hazard(torch, cycles_per_ms)
    t_frame = hz.input(g["frame"])
    t_kw = {k: (hz.input(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    t_out = hz.output((h, w, 3), torch.float32, 3.0, 5.0)
    (got,), _ = hz.run(ctx, kind, lambda: ctx.atrous_filter(t_frame, **t_kw, out=t_out))
    assert same_bits(got, want), mismatch(got, want)
    assert not same_bits(R.atrous_filter(np.zeros_like(g["frame"]), **kw)[0], want)          # (the stale frame's answer is another)


def test_second_context_gives_the_same_bytes(gpu):
    h, w = 35, 67
    kw = call_kwargs(h, w, "all+albedo+emitted", 5)
    first = gpu.atrous_filter(inputs(h, w)["frame"], **kw)[0]
    with R.Renderer(0) as other:
        second = other.atrous_filter(inputs(h, w)["frame"], **kw)[0]
        small = other.atrous_filter(inputs(9, 17)["frame"], **call_kwargs(9, 17, "all", 3))[0]      # (a smaller frame on the grown scratch)
    assert same_bits(first, second) and same_bits(first, host_answer(h, w, "all+albedo+emitted", 5))
    assert same_bits(small, host_answer(9, 17, "all", 3))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_error_paths_device(gpu):
    g = inputs(9, 17)
    frame = g["frame"].copy()
    out = np.full_like(frame, 7.0)
    ip, op = C.c_void_p(frame.ctypes.data), C.c_void_p(out.ctypes.data)
    dp, np_, xp, ap, ep = (C.c_void_p(g[k].ctypes.data) for k in ("depth", "normal", "ids", "albedo", "emitted"))
    call = R.lib().rtw_ctx_atrous_filter
    hnd = gpu._h

    def prm(levels=3, sc=0.5, sd=0.5, sn=0.5, same=1, floor=FLOOR):
        return C.byref(R.RtwAtrous(levels, sc, sd, sn, same, floor))

    def refused(*args):
        assert call(*args) == -1
        assert (out == 7.0).all()

    refused(None, ip, 17, 9, dp, np_, xp, ap, ep, prm(), op, None)
    refused(hnd, None, 17, 9, dp, np_, xp, ap, ep, prm(), op, None)
    refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(), None, None)
    refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, None, op, None)
    refused(hnd, ip, 0, 9, dp, np_, xp, ap, ep, prm(), op, None)
    refused(hnd, ip, 17, 0, dp, np_, xp, ap, ep, prm(), op, None)
    refused(hnd, ip, 65536, 65536, dp, np_, xp, ap, ep, prm(), op, None)
    refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=0), op, None)
    refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=R.ATROUS_MAX_LEVELS + 1), op, None)
    for v in (-1.0, float("nan"), float("inf"), 1e-30):
        refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(sc=v), op, None)
        refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(sd=v), op, None)
        refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(sn=v), op, None)
    refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=8, sc=1e-18), op, None)
    refused(hnd, ip, 17, 9, None, np_, xp, ap, ep, prm(), op, None)
    refused(hnd, ip, 17, 9, dp, None, xp, ap, ep, prm(), op, None)
    refused(hnd, ip, 17, 9, dp, np_, None, ap, ep, prm(), op, None)
    refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(same=2), op, None)
    for v in (0.0, -0.5, float("nan"), float("inf")):
        refused(hnd, ip, 17, 9, dp, np_, xp, ap, ep, prm(floor=v), op, None)
    assert call(hnd, ip, 17, 9, None, None, None, None, None, prm(sd=0.0, sn=0.0, same=0, floor=0.0), op, None) == 0      # off terms: NULL guides
    assert same_bits(out, R.atrous_filter(frame, levels=3, sigma_color=0.5)[0])


# ---- 6. quality: the one assertion ---------------------------------------------------------------------------------------------------------
def test_the_defaults_lower_the_error_of_the_4spp_book1_frame(gpu):
    """The Book-1 view of small_view(SCENE_C2, 400, 225, 4) under SAMPLER_ROW at gamma 1, guides, albedo and emission from surface_map at the
    pixel centres, the Python defaults, against a 4096-spp render of the same view: the filtered MSE is below the unfiltered one.  Measured
    (scripts/measure_atrous.py, profiles/atrous.log): ratio 0.269 on the sweep's frame and 0.264 .. 0.273 over 8 other seeds -- below the
    0.5 that DESIGN.md 8c asks of a ratio before it is asserted at 1, a margin of two over a spread of 0.01."""
    from tests.test_oracle_golden import small_view
    w, h = 400, 225
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    p.samples, p.seed = 4096, 1
    truth = gpu.render(cam, p)[0].astype(np.float64)
    p.samples, p.seed = 4, 7
    frame = gpu.render(cam, p)[0]
    g = gpu.surface_map(cam, w, h, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, (0.5, 0.5))
    out = gpu.atrous_filter(frame, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"])[0]
    before, after = float(((frame - truth) ** 2).mean()), float(((out - truth) ** 2).mean())
    print(f"\n[a-trous quality] unfiltered MSE {before:.6f}, filtered {after:.6f}, ratio {after / before:.3f}")
    assert after < before, (before, after)
    den, _ = gpu.render_denoised(cam, p)                           # the same chain behind one call (gamma 1: no power applied)
    assert same_bits(den, out)
