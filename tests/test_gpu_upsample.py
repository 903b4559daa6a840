"""The guide-steered upsampling on the GPU (rtw_ctx_upsample_filter, csrc/rtw_upsample.hip) against its host form, bit for
bit (tests/atrous_common.py's same_bits): the CPU tests' matrix under every RTW_OPT_ATROUS_LAYOUT, output sizes around the workgroup's
32 x 16 pixels with ragged low sizes, every edge value on the first and last row and column of the middle workgroup's low window, in its
halo and in the low frame's corners, fallback pixels on a tile's edge, host and device memory mixed per argument, torch tensors behind
use_torch_stream, a second context, the refusals, render_upsampled and the two denoisers' steps against the hand-chained calls.  The host
form itself is held to numpy restatements by tests/test_upsample_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.upsample_common import (EDGE_IDS, F, FLOOR, RADII, SCALES, SIZES, TERMS, TILE_SCALES, TILE_SIZES, check_upsample, check_upsample_refusals,
                                   edge_pixels, guides_for, host_upsample, inputs, lo_size, mismatch, same_bits, term_kw, window_places)
from tests.temporal_common import OFFSET
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

LAYOUTS = [0, 1, 2]                                        # the measured choice, LDS tile, global memory
SIZE_IDS = lambda s: f"{s[0]}x{s[1]}"
ALL, NONE = TERMS[-1], TERMS[0]
SOME = [ALL, NONE, (True, False, False, True), (False, True, True, False)]


@pytest.fixture()
def layout(gpu, request):
    gpu.set_option(R.OPT_ATROUS_LAYOUT, request.param)
    yield request.param
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)


# ---- 1. the matrix -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_upsample_device_equals_host(gpu, size, layout):
    w, h = size
    for scale in SCALES:
        for radius in RADII:
            for terms in TERMS:
                st = check_upsample(gpu.upsample_filter, w, h, scale, radius, terms)
                assert st.filter_ms > 0.0


# ---- 2. around the tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("size", TILE_SIZES, ids=SIZE_IDS)
def test_sizes_around_the_tile(gpu, size, layout):
    """Window entries outside the low frame and the pixels a ragged last workgroup does not have; 65 x 33 at scale 2 has a 33 x 17 low
    frame, at scale 3 a 22 x 11 one whose last low pixel covers one output column."""
    w, h = size
    for scale in TILE_SCALES:
        for radius in RADII:
            for terms in SOME:
                check_upsample(gpu.upsample_filter, w, h, scale, radius, terms)


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_many_workgroups_at_scale_1_and_8(gpu, layout):
    for scale, radius in ((1, 2), (8, 1), (8, 2)):
        check_upsample(gpu.upsample_filter, 70, 50, scale, radius, ALL)


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("which", range(len(edge_pixels())), ids=EDGE_IDS)
def test_edge_values_on_the_windows_edges_and_in_its_halo(gpu, which, layout):
    """97 x 49 output pixels are 4 x 4 workgroups (the last ragged): the value sits in low pixels on the first and last row and column of the
    window of the workgroup at (32, 16), in the entries next to them and in the low frame's corners."""
    w, h = 97, 49
    for scale in TILE_SCALES:
        for radius in RADII:
            places = window_places(w, h, scale, radius)
            for terms in (ALL, NONE):
                check_upsample(gpu.upsample_filter, w, h, scale, radius, terms, (places, which))


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_fallback_pixels_on_a_tiles_edge(gpu, layout):
    """Output pixels whose id no low pixel has, on the first and last row and column of the workgroup at (32, 16) and of its neighbours:
    each takes its covering low pixel from the window, and wsum is 0 exactly there."""
    w, h = 97, 49
    lonely = [(j, i) for j in (15, 16, 31, 32, 0, h - 1) for i in (31, 32, 63, 64, 0, w - 1)]
    for scale in TILE_SCALES:
        fr, g_lo, g_hi = inputs(w, h, scale)
        ids = np.zeros((h, w), np.int32)
        for n, (j, i) in enumerate(lonely):
            ids[j, i] = 1000 + n
        lo, hi = dict(g_lo, idx=np.zeros_like(g_lo["idx"])), dict(g_hi, idx=ids)
        for radius in RADII:
            kw = dict(scale=scale, radius=radius, sigma_depth=0.0, sigma_normal=0.0, same_object=True, albedo_floor=FLOOR, out_wsum=True)
            out, ws, _ = gpu.upsample_filter(fr, (w, h), lo=lo, hi=hi, **kw)
            want, wws, _ = R.upsample_filter(fr, (w, h), lo=lo, hi=hi, **kw)
            assert same_bits(out, want), (scale, radius, mismatch(out, want))
            assert same_bits(ws, wws)
            zero = np.zeros((h, w), bool)
            zero[tuple(np.array(lonely).T)] = True
            assert np.array_equal(ws == 0.0, zero)


# ---- 3. memory kinds ---------------------------------------------------------------------------------------------------------------------
NAMES = ["frame", "lo", "hi", "out", "wsum"]
mask_id = lambda m: "".join(n[0] if m >> i & 1 else "-" for i, n in enumerate(NAMES))


@pytest.mark.parametrize("on_device", [0b00000, 0b11111, 0b01010, 0b10101, 0b00011, 0b11100, 0b10000], ids=mask_id)
def test_host_and_device_memory_mixed(gpu, torch, on_device):
    """Each argument independently a numpy array (staged) or a torch tensor (in place); within a guide dict the kinds alternate too."""
    w, h, s = 67, 35, 3
    w_lo, h_lo = lo_size(w, h, s)
    fr, g_lo, g_hi = inputs(w, h, s)
    dev = torch.device("cuda:0")
    t = lambda a, on: torch.from_numpy(np.array(a)).to(dev) if on else np.array(a)
    lo = {k: t(v, (on_device >> 1 & 1) ^ (n & 1)) for n, (k, v) in enumerate(g_lo.items())}
    hi = {k: t(v, (on_device >> 2 & 1) ^ (n & 1)) for n, (k, v) in enumerate(g_hi.items())}
    out = torch.full((h, w, 3), 7.0, device=dev) if on_device >> 3 & 1 else np.full((h, w, 3), 7.0, F)
    ws = torch.full((h, w), 7.0, device=dev) if on_device >> 4 & 1 else np.full((h, w), 7.0, F)
    got, gws, _ = gpu.upsample_filter(t(fr, on_device & 1), (w, h), lo=lo, hi=hi, scale=s, radius=2, out=out, out_wsum=ws, **term_kw(ALL))
    assert got is out and gws is ws
    want = host_upsample(w, h, s, 2, ALL)
    for g, x in zip((out, ws), want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert same_bits(g, x), mismatch(g, x)


# ---- 4. stream order and contexts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_tensors_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """The low frame, a guide of each side and both outputs are tensors whose producers are still pending on the caller's stream when the
    call is made (tests/test_gpu_stream_order.py): the pass reads the new frame."""
    w, h, s = 67, 35, 2
    fr, g_lo, g_hi = inputs(w, h, s)
    want = host_upsample(w, h, s, 1, ALL)
    kw = dict(scale=s, radius=1, **term_kw(ALL))
    got = ctx.upsample_filter(fr, (w, h), lo=g_lo, hi=g_hi, out_wsum=True, **kw)         # own stream, host buffers: the scratch is grown
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])

    hz = Hazard(torch, cycles_per_ms)
    t_fr = hz.input(fr)
    t_lo = dict(g_lo, depth=hz.input(g_lo["depth"]), albedo=hz.input(g_lo["albedo"], stale=np.ones_like(g_lo["albedo"])))
    t_hi = dict(g_hi, idx=hz.input(g_hi["idx"], stale=np.full((h, w), 3, np.int32)), emitted=hz.input(g_hi["emitted"]))
    t_out, t_ws = hz.output((h, w, 3), torch.float32, 3.0, 5.0), hz.output((h, w), torch.float32, 3.0, 5.0)
    got, _ = hz.run(ctx, kind, lambda: ctx.upsample_filter(t_fr, (w, h), lo=t_lo, hi=t_hi, out=t_out, out_wsum=t_ws, **kw))
    for g, x in zip(got, want):
        assert same_bits(g, x), mismatch(g, x)
    stale = R.upsample_filter(np.zeros_like(fr), (w, h), lo=g_lo, hi=g_hi, **kw)[0]
    assert not same_bits(stale, want[0])                                                 # (the stale answer is another)


def test_second_context_gives_the_same_bytes(gpu):
    first = check_upsample(gpu.upsample_filter, 65, 33, 2, 2, ALL)
    with R.Renderer(0) as other:
        check_upsample(other.upsample_filter, 65, 33, 2, 2, ALL)
        check_upsample(other.upsample_filter, 5, 4, 3, 1, NONE)                          # (a smaller frame on the grown scratch)
        check_upsample(other.upsample_filter, 97, 49, 4, 2, ALL)                         # (and a larger one, which grows it again)
    assert first.taps == host_upsample(65, 33, 2, 2, ALL)[2]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_error_paths_device(gpu):
    check_upsample_refusals(R.lib().rtw_ctx_upsample_filter, (gpu._h,))
    fr = np.array(inputs(5, 4, 2)[0])
    out = np.full((4, 5, 3), 7.0, F)
    P = lambda a: R.C.c_void_p(a.ctypes.data)
    prm = R.RtwUpsample(2, 1, 0.0, 0.0, 0, FLOOR)
    assert R.lib().rtw_ctx_upsample_filter(None, P(fr), 3, 2, None, 5, 4, None, R.C.byref(prm), P(out), None, None) == -1
    assert (out == 7.0).all()                                                            # no context


# ---- 6. the drivers ------------------------------------------------------------------------------------------------------------------------
def _view(gpu, w, h, spp=4):
    from tests.test_oracle_golden import small_view
    scene, cam, p = small_view(R.SCENE_C2, w, h, spp)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 2.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    p.samples = spp
    return cam, p


def _surf(gpu, cam, p):
    return gpu.surface_map(cam, p.width, p.height, p.mint, p.maxt, p.integrator, R.RAYS_PIXEL, (0.5, 0.5), accel=p.accel)


def _gamma(a, gamma):
    return np.power(np.maximum(a, np.float32(0.0)), np.float32(1.0 / gamma)).astype(np.float32)


def _low(cam, p, scale):
    lp = R.RtwParams.from_buffer_copy(p)
    lp.width, lp.height = lo_size(p.width, p.height, scale)
    lp.gamma = 1.0
    return R.camera_scaled(cam, scale), lp


@pytest.mark.parametrize("size", [(64, 48), (50, 37)], ids=SIZE_IDS)
def test_render_upsampled_is_the_hand_chained_calls(gpu, size):
    """render at the low size with camera_scaled at gamma 1, surface_map there, (atrous_filter), surface_map at the output size,
    upsample_filter, gamma; the two filters through their host forms.  50 x 37 has ceiling sizes at scales 3 and 4."""
    w, h = size
    cam, p = _view(gpu, w, h)
    for scale, atrous, ukw in ((2, None, {}), (3, dict(levels=2), dict(radius=2)), (4, dict(levels=1, sigma_color=0.5), dict(sigma_depth=0.5, same_object=False))):
        p.seed = 7
        got, st = gpu.render_upsampled(cam, p, scale, atrous=atrous, **ukw)
        lcam, lp = _low(cam, p, scale)
        frame, st2 = gpu.render(lcam, lp)
        assert frame.shape == (lp.height, lp.width, 3) and st.segments == st2.segments
        g, hi = _surf(gpu, lcam, lp), _surf(gpu, cam, p)
        if atrous is not None:
            frame = R.atrous_filter(frame, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"], **atrous)[0]
        want = _gamma(R.upsample_filter(frame, (w, h), lo=g, hi=hi, scale=scale, **ukw)[0], 2.0)
        assert got.shape == (h, w, 3) and same_bits(got, want), (size, scale, mismatch(got, want))
        assert p.gamma == 2.0 and (p.width, p.height) == (w, h)


TKW = dict(alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1)
SKW = dict(levels=2, sigma_luminance=2.0, epsilon=1e-6, prefilter=True, sigma_depth=0.25, sigma_normal=0.3)
AKW = dict(levels=2, sigma_color=1.0, sigma_depth=0.25, sigma_normal=0.3)


def _filtered(cls, hist, g):
    guides = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
    if cls is R.SvgfDenoiser:
        v = R.variance_estimate(hist["moments"], hist["len"], **guides, sigma_depth=0.25, sigma_normal=0.3)[0]
        return R.svgf_filter(hist["color"], v, **guides, albedo=g["albedo"], emitted=g["emitted"], **SKW)[0]
    return R.atrous_filter(hist["color"], **guides, albedo=g["albedo"], emitted=g["emitted"], **AKW)[0]


@pytest.mark.parametrize("cls", [R.TemporalDenoiser, R.SvgfDenoiser], ids=["temporal", "svgf"])
def test_the_denoisers_at_scale_2_are_the_hand_chained_calls(gpu, cls):
    """Three steps of a moved camera at 64 x 48: the history lives at 32 x 24 and is that of temporal_accumulate's host form on the low
    render and low guides with the scaled cameras; the frame is upsample_filter's host form of the filter's host form, then gamma."""
    from tests.temporal_common import orbit
    w, h, scale = 64, 48, 2
    cam, p = _view(gpu, w, h)
    ukw = dict(radius=2, sigma_depth=0.5)
    den = cls(gpu, scale=scale, upsample=ukw, **TKW)
    kw = SKW if cls is R.SvgfDenoiser else AKW
    hist = None
    p.seed = 40
    for k, deg in enumerate((0.0, 1.0, 2.0)):
        c = orbit(cam, deg)
        frame, acc, var, st = den.step(c, p, **kw)
        lcam, lp = _low(c, p, scale)                                             # (p.seed is the step's)
        cur = gpu.render(lcam, lp)[0]
        assert same_bits(st["cur"], cur) and cur.shape == (h // 2, w // 2, 3)
        g, hi = st["guides"], st["guides_hi"]
        for key, x in _surf(gpu, lcam, lp).items():
            assert key == "stats" or same_bits(np.asarray(g[key], F), np.asarray(x, F)), (k, key)
        for key, x in _surf(gpu, c, p).items():
            assert key == "stats" or same_bits(np.asarray(hi[key], F), np.asarray(x, F)), (k, key)
        hist, _, _ = R.temporal_accumulate(cur, lcam, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist, offset=OFFSET, **TKW)
        for key in ("color", "moments", "len"):
            assert same_bits(den.history[key], hist[key]), (cls.__name__, k, key, mismatch(den.history[key], hist[key]))
        assert same_bits(acc, hist["color"]) and acc.shape == cur.shape
        low = _filtered(cls, hist, g)
        up, ws, _ = R.upsample_filter(low, (w, h), lo=g, hi=hi, scale=scale, out_wsum=True, **ukw)
        assert same_bits(frame, _gamma(up, 2.0)), (cls.__name__, k, mismatch(frame, _gamma(up, 2.0)))
        assert same_bits(st["wsum"], ws) and st["upsample"].filter_ms > 0.0
    assert (den.history["len"] > 1).mean() > 0.5                                  # the scaled previous camera reprojects


@pytest.mark.parametrize("cls", [R.TemporalDenoiser, R.SvgfDenoiser], ids=["temporal", "svgf"])
def test_the_denoisers_at_scale_1_write_their_present_bytes(gpu, cls):
    """scale=1: the steps make the calls they made -- render, surface_map, temporal_accumulate, the filter at params' size -- whose outputs
    are those of the calls chained by hand as tests/test_gpu_bounds.py chains them, and no upsampling enters."""
    from tests.temporal_common import orbit
    w, h = 64, 48
    cam, p = _view(gpu, w, h)
    den, plain = cls(gpu, scale=1, **TKW), cls(gpu, **TKW)
    kw = SKW if cls is R.SvgfDenoiser else AKW
    hist = None
    p.seed = 60
    for k, deg in enumerate((0.0, 1.0, 2.0)):
        c = orbit(cam, deg)
        frame, acc, var, st = den.step(c, p, **kw)
        p.seed -= 1
        frame2, acc2, var2, st2 = plain.step(c, p, **kw)
        assert same_bits(frame, frame2) and same_bits(acc, acc2) and same_bits(var, var2)
        assert not {"upsample", "guides_hi", "wsum"} & set(st) and frame.shape == (h, w, 3) and acc.shape == (h, w, 3)
        cur = gpu.render(c, _low(c, p, 1)[1])[0]
        assert same_bits(st["cur"], cur)
        g = st["guides"]
        hist, _, _ = R.temporal_accumulate(cur, c, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist, offset=OFFSET, **TKW)
        for key in ("color", "moments", "len"):
            assert same_bits(den.history[key], hist[key]), (cls.__name__, k, key)
        assert same_bits(frame, _gamma(_filtered(cls, hist, g), 2.0)), (cls.__name__, k)
