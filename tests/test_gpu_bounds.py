"""The neighbourhood colour bounds and the bounded temporal accumulation on the GPU (rtw_ctx_colour_bounds,
rtw_ctx_temporal_accumulate_bounded, csrc/rtw_bounds.hip, csrc/rtw_temporal.hip) against their host forms, bit for bit
(tests/atrous_common.py's same_bits): the CPU tests' matrix under every RTW_OPT_ATROUS_LAYOUT, frames around the workgroup's 32 x 16 tile,
many ragged tiles, every edge value on a tile's first and last row and column and in its halo, host and device memory mixed per argument,
torch tensors behind use_torch_stream, a second context, the refusals, the bounded accumulation over the CPU cases, and the two denoisers'
steps with firefly and history_clamp against the hand-chained calls.  The host forms themselves are held to numpy restatements by
tests/test_bounds_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.bounds_common import (BOUNDED_CASES, BOUNDED_KEYS, F, FLAGS, KS, MANY_TILES, RADII, SHAPES, TILE_SHAPES, assert_same_outputs, bounded_case,
                                 case_bounds, check_bounded_refusals, check_bounds, check_bounds_refusals, edge_pixels, host_bounded, host_bounds,
                                 inputs, lighting_step, mismatch, raw_null_bounds_vs_points, run_bounded, same_bits, small_places, tile_places)
from tests.temporal_common import OFFSET
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

LAYOUTS = [0, 1, 2]                                        # the measured choice, LDS tile, global memory
SHAPE_IDS = lambda s: f"{s[1]}x{s[0]}"
EDGE_IDS = ["nan", "+inf", "-inf", "3e38", "denormal", "-0"]


@pytest.fixture()
def layout(gpu, request):
    gpu.set_option(R.OPT_ATROUS_LAYOUT, request.param)
    yield request.param
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)


# ---- 1. the matrix -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_bounds_device_equals_host(gpu, shape, layout):
    h, w = shape
    for radius in RADII:
        for k in KS:
            for same, excl in FLAGS:
                st = check_bounds(gpu.colour_bounds, h, w, radius, k, same, excl)
                assert st.filter_ms > 0.0


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("which", range(len(edge_pixels())), ids=EDGE_IDS)
def test_edge_values_in_small_frames(gpu, which, layout):
    for h, w in ((4, 5), (9, 3)):
        for places in small_places(h, w):
            for radius in (1, 3):
                for same, excl in FLAGS:
                    check_bounds(gpu.colour_bounds, h, w, radius, 1.0, same, excl, (places, which))


# ---- 2. around the tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("shape", TILE_SHAPES, ids=SHAPE_IDS)
def test_frames_around_the_tile(gpu, shape, layout):
    """Halo entries outside the frame and the pixels a ragged last tile does not have must not count as taps."""
    h, w = shape
    for radius in RADII:
        for same, excl in FLAGS:
            check_bounds(gpu.colour_bounds, h, w, radius, 1.0, same, excl)


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_many_tiles(gpu, layout):
    h, w = MANY_TILES
    for radius, k, same, excl in ((3, 2.0, True, False), (1, 0.5, False, True), (2, 1.0, True, True)):
        check_bounds(gpu.colour_bounds, h, w, radius, k, same, excl)


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("which", range(len(edge_pixels())), ids=EDGE_IDS)
def test_edge_values_on_the_tiles_edges_and_in_their_halos(gpu, which, layout):
    """65 x 33 pixels are 3 x 3 workgroups: the value sits on the first and last row and column of the middle tile, on the rows and columns
    next to them (its halo, the neighbours' edges) and in the frame's corners."""
    h, w = 33, 65
    places = tile_places(h, w)
    for radius, same, excl in ((3, True, False), (1, False, True), (2, False, False)):
        check_bounds(gpu.colour_bounds, h, w, radius, 1.0, same, excl, (places, which))


# ---- 3. memory kinds ---------------------------------------------------------------------------------------------------------------------
B_NAMES = ["frame", "ids", "out_lo", "out_hi", "out_clamped"]
mask_id = lambda names: (lambda m: "".join(n.split("_")[-1][0] if m >> i & 1 else "-" for i, n in enumerate(names)))


@pytest.mark.parametrize("on_device", [0b00000, 0b11111, 0b01010, 0b10101, 0b00011, 0b11100, 0b10000], ids=mask_id(B_NAMES))
def test_bounds_host_and_device_memory_mixed(gpu, torch, on_device):
    """Each argument independently a numpy array (staged) or a torch tensor (in place)."""
    h, w = 35, 67
    fr, ids = inputs(h, w)
    dev = torch.device("cuda:0")
    t = lambda a, i: torch.from_numpy(np.array(a)).to(dev) if on_device >> i & 1 else np.array(a)
    outs = [torch.full((h, w, 3), 7.0, device=dev) if on_device >> i & 1 else np.full((h, w, 3), 7.0, F) for i in (2, 3, 4)]
    lo, hi, cl, _ = gpu.colour_bounds(t(fr, 0), ids=t(ids, 1), radius=3, k=1.5, same_object=True, out_lo=outs[0], out_hi=outs[1], out_clamped=outs[2])
    assert lo is outs[0] and hi is outs[1] and cl is outs[2]
    want = R.colour_bounds(fr, ids=ids, radius=3, k=1.5, same_object=True, out_clamped=True)
    for g, x in zip(outs, want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert same_bits(g, x), mismatch(g, x)


# ---- 4. stream order and contexts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_tensors_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """Every buffer a tensor whose producer is still pending on the caller's stream when the call is made (tests/test_gpu_stream_order.py)."""
    h, w = 35, 67
    fr, ids = (np.array(a) for a in inputs(h, w))
    want = R.colour_bounds(fr, ids=ids, radius=3, k=1.5, same_object=True, out_clamped=True)
    got = ctx.colour_bounds(fr, ids=ids, radius=3, k=1.5, same_object=True, out_clamped=True)       # own stream, host buffers: the scratch is grown
    assert all(same_bits(g, x) for g, x in zip(got[:3], want[:3]))

    hz = Hazard(torch, cycles_per_ms)
    t_fr, t_ids = hz.input(fr), hz.input(ids, stale=np.full((h, w), 3, np.int32))
    t_out = [hz.output((h, w, 3), torch.float32, 3.0, 5.0) for _ in range(3)]
    got, _ = hz.run(ctx, kind, lambda: ctx.colour_bounds(t_fr, ids=t_ids, radius=3, k=1.5, same_object=True, out_lo=t_out[0], out_hi=t_out[1],
                                                         out_clamped=t_out[2]))
    for g, x in zip(got, want):
        assert same_bits(g, x), mismatch(g, x)
    assert not same_bits(R.colour_bounds(np.zeros_like(fr), radius=3, k=1.5)[0], want[0])          # (the stale answer is another)

    # the bounded accumulation likewise: the bounds and out_clipped behind the stream
    frames, params, _ = bounded_case("moved")
    f0, f1 = frames
    want = host_bounded("moved", "box")
    lo, hi = case_bounds(f1, "box")
    first = ctx.temporal_accumulate(f0["cur"], f0["cam"], depth=f0["depth"], normal=f0["normal"], ids=f0["idx"], offset=OFFSET, **params)[0]
    hz = Hazard(torch, cycles_per_ms)
    t_cur, t_lo, t_hi = hz.input(f1["cur"]), hz.input(lo), hz.input(hi, stale=np.full_like(hi, -1.0))
    t_color, t_clipped = hz.output(f1["cur"].shape, torch.float32, 3.0, 5.0), hz.output(f1["depth"].shape, torch.float32, 3.0, 5.0)
    (color, clipped), _ = hz.run(ctx, kind, lambda: ctx.temporal_accumulate(t_cur, f1["cam"], depth=f1["depth"], normal=f1["normal"], ids=f1["idx"],
                                                                            history=first, hist_lo=t_lo, hist_hi=t_hi, out_color=t_color,
                                                                            out_clipped=t_clipped, offset=OFFSET, **params))
    assert same_bits(color, want["color"]), mismatch(color, want["color"])
    assert same_bits(clipped, want["clipped"]), mismatch(clipped, want["clipped"])


def test_second_context_gives_the_same_bytes(gpu):
    h, w = 35, 67
    first = check_bounds(gpu.colour_bounds, h, w, 3, 1.0, True, False)
    with R.Renderer(0) as other:
        check_bounds(other.colour_bounds, h, w, 3, 1.0, True, False)
        check_bounds(other.colour_bounds, 4, 5, 2, 0.5, False, True)            # (a smaller frame on the grown scratch)
        check_bounds(other.colour_bounds, *MANY_TILES, 3, 2.0, True, False)     # (and a larger one, which grows it again)
        got = run_bounded(other.temporal_accumulate, "moved", "box")
        assert_same_outputs(got, host_bounded("moved", "box"), "second context")
    assert first.taps == host_bounds(h, w, 3, 1.0, True, False)[3]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_error_paths_device(gpu):
    check_bounds_refusals(R.lib().rtw_ctx_colour_bounds, (gpu._h,))
    check_bounded_refusals(R.lib().rtw_ctx_temporal_accumulate_bounded, (gpu._h,))
    fr, _ = inputs(4, 5)
    out = [np.full((4, 5, 3), 7.0, F) for _ in range(3)]
    P = lambda a: R.C.c_void_p(a.ctypes.data)
    assert R.lib().rtw_ctx_colour_bounds(None, P(np.array(fr)), 5, 4, None, R.C.byref(R.RtwColourBounds(1, 1.0, 0, 0)), *(P(a) for a in out), None) == -1
    assert all((a == 7.0).all() for a in out)                                   # no context


# ---- 6. the bounded accumulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BOUNDED_CASES)
def test_bounded_device_equals_host(gpu, torch, name):
    """The CPU cases, host buffers and device tensors; with all three new arguments None the call is the _points call on the same inputs."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    for kind in ("box", "open", "nan", "cur"):
        want = host_bounded(name, kind)
        assert_same_outputs(run_bounded(gpu.temporal_accumulate, name, kind), want, (name, kind, "host buffers"))
        assert_same_outputs(run_bounded(gpu.temporal_accumulate, name, kind, wrap=dev), want, (name, kind, "device tensors"))
    plain = run_bounded(gpu.temporal_accumulate, name, None, clipped=False)
    assert "clipped" not in plain
    want = run_bounded(R.temporal_accumulate, name, None, clipped=False)
    assert_same_outputs(plain, want, (name, "all None"))
    assert_same_outputs({k: host_bounded(name, "open")[k] for k in want}, want, (name, "open is the _points call"))
    only_clipped = run_bounded(gpu.temporal_accumulate, name, None)                       # out_clipped alone: the fourth kernel, no box
    assert_same_outputs(only_clipped, dict(want, clipped=np.zeros_like(want["len"])), (name, "out_clipped alone"))


@pytest.mark.parametrize("name", BOUNDED_CASES)
def test_the_c_call_with_the_three_new_pointers_null_is_the_points_call(gpu, name):
    """rtw_ctx_temporal_accumulate_bounded itself, through ctypes, hist_lo = hist_hi = out_clipped = NULL, against
    rtw_ctx_temporal_accumulate_points on the same inputs, and both against the host entry points: the five outputs byte for byte."""
    L = R.lib()
    got, want = raw_null_bounds_vs_points(L.rtw_ctx_temporal_accumulate_bounded, L.rtw_ctx_temporal_accumulate_points, (gpu._h,), name)
    host, _ = raw_null_bounds_vs_points(L.rtw_temporal_accumulate_bounded, L.rtw_temporal_accumulate_points, (), name)
    for k, (g, x, y) in enumerate(zip(got, want, host)):
        assert same_bits(g, x), (name, k, mismatch(g, x))
        assert same_bits(g, y), (name, k, "host", mismatch(g, y))


def test_a_lighting_step_is_followed_at_once(gpu, torch):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    for wrap in (None, dev):
        plain, bounded, clipped = lighting_step(gpu.temporal_accumulate, gpu.colour_bounds, radius=2, k=1.0, wrap=wrap)
        want = lighting_step(R.temporal_accumulate, R.colour_bounds, radius=2, k=1.0)
        assert same_bits(plain, want[0]) and (bounded == F(0.75)).all() and (clipped == F(1.5)).all()


# ---- 7. the sequence drivers -------------------------------------------------------------------------------------------------------------
def _view(gpu):
    from tests.test_oracle_golden import small_view
    w, h = 67, 35
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    p.samples = 4
    return cam, p


TKW = dict(alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1)


@pytest.mark.parametrize("which", ["firefly", "history_clamp", "both"])
def test_the_denoisers_are_the_hand_chained_calls(gpu, which):
    """TemporalDenoiser.step and SvgfDenoiser.step over three frames of a moved camera at 67 x 35 with firefly and / or history_clamp: the
    accumulated colour, the moments, the length and out_clipped are those of the calls chained by hand on the same rendered frame and
    guides through the host forms of the two new passes, and the filtered frame that of the filter's host form on them."""
    from tests.temporal_common import orbit
    cam, p = _view(gpu)
    firefly = dict(radius=2, k=2.0) if which != "history_clamp" else None
    clamp = dict(radius=1, k=1.0, same_object=True) if which != "firefly" else None
    skw = dict(levels=2, sigma_luminance=2.0, epsilon=1e-6, prefilter=True, sigma_depth=0.25, sigma_normal=0.3)
    akw = dict(levels=2, sigma_color=1.0, sigma_depth=0.25, sigma_normal=0.3)
    for cls in (R.TemporalDenoiser, R.SvgfDenoiser):
        den, plain = cls(gpu, **TKW), cls(gpu, **TKW)
        hist = None
        p.seed = 40
        moved = 0
        for k, deg in enumerate((0.0, 1.0, 2.0)):
            c = orbit(cam, deg)
            kw = skw if cls is R.SvgfDenoiser else akw
            frame, acc, var, st = den.step(c, p, firefly=firefly, history_clamp=clamp, **kw)
            p.seed -= 1
            raw = plain.step(c, p, **kw)[3]["cur"]                               # the rendered frame, before any clamp
            g = st["guides"]
            guides = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
            cur = raw
            if firefly:
                cur = R.colour_bounds(raw, exclude_centre=True, out_clamped=True, **firefly)[2]
                assert st["firefly"].filter_ms > 0.0
            assert same_bits(st["cur"], cur), (cls.__name__, k, mismatch(st["cur"], cur))
            bounds = {}
            if clamp:
                lo, hi, _, _ = R.colour_bounds(cur, ids=g["idx"], **clamp)
                bounds = dict(hist_lo=lo, hist_hi=hi, out_clipped=True)
                assert st["history_clamp"].filter_ms > 0.0
            hist, _, _ = R.temporal_accumulate(cur, c, **guides, history=hist, offset=OFFSET, **bounds, **TKW)
            for key in ("color", "moments", "len") + (("clipped",) if clamp else ()):
                assert same_bits(den.history[key], hist[key]), (cls.__name__, k, key, mismatch(den.history[key], hist[key]))
            if clamp:
                moved += int((hist["clipped"] > 0).sum())
            if cls is R.SvgfDenoiser:
                v = R.variance_estimate(hist["moments"], hist["len"], **guides, sigma_depth=0.25, sigma_normal=0.3)[0]
                want = R.svgf_filter(hist["color"], v, **guides, albedo=g["albedo"], emitted=g["emitted"], **skw)[0]
            else:
                want = R.atrous_filter(hist["color"], **guides, albedo=g["albedo"], emitted=g["emitted"], **akw)[0]
            assert same_bits(frame, want), (cls.__name__, k, mismatch(frame, want))
        assert not clamp or moved > 0                                            # the clamp was at work


def test_the_denoisers_without_the_new_arguments_write_their_present_bytes(gpu):
    """firefly=None, history_clamp=None: both steps make the calls they made, whose outputs are those of the calls the existing tests chain
    by hand -- render, surface_map, temporal_accumulate, the filter -- and the history has no "clipped"."""
    from tests.temporal_common import orbit
    cam, p = _view(gpu)
    for cls in (R.TemporalDenoiser, R.SvgfDenoiser):
        den, same = cls(gpu, **TKW), cls(gpu, **TKW)
        hist = None
        p.seed = 60
        for k, deg in enumerate((0.0, 1.0)):
            c = orbit(cam, deg)
            frame, acc, var, st = den.step(c, p, firefly=None, history_clamp=None)
            p.seed -= 1
            frame2, acc2, var2, _ = same.step(c, p)
            assert same_bits(frame, frame2) and same_bits(acc, acc2) and same_bits(var, var2)
            assert "clipped" not in den.history and "firefly" not in st and "history_clamp" not in st
            g = st["guides"]
            guides = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
            hist, hvar, _ = R.temporal_accumulate(st["cur"], c, **guides, history=hist, offset=OFFSET, **TKW)
            for key in ("color", "moments", "len"):
                assert same_bits(den.history[key], hist[key]), (cls.__name__, k, key)
            if cls is R.SvgfDenoiser:
                v = R.variance_estimate(hist["moments"], hist["len"], **guides)[0]
                want = R.svgf_filter(hist["color"], v, **guides, albedo=g["albedo"], emitted=g["emitted"])[0]
            else:
                want = R.atrous_filter(hist["color"], **guides, albedo=g["albedo"], emitted=g["emitted"])[0]
            assert same_bits(frame, want), (cls.__name__, k, mismatch(frame, want))
