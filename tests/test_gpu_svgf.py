"""The variance estimate and the variance-steered a-trous filter on the GPU (rtw_ctx_variance_estimate, rtw_ctx_svgf_filter,
csrc/rtw_svgf.hip) against their host forms, bit for bit (tests/atrous_common.py's same_bits): the CPU tests' matrix under
every RTW_OPT_ATROUS_LAYOUT, strips 259 pixels long whose taps at levels 7 and 8 land inside the frame, frames around the workgroup's 32 x 16 tile, many ragged tiles, host and device memory mixed per argument,
out == in, torch tensors behind use_torch_stream, a second context, the refusals, the a-trous filter on the scratch these calls grew, and
SvgfDenoiser against the hand-chained calls.  The host forms themselves are held to numpy restatements by tests/test_svgf_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.atrous_common import TERM_SETS, call_kwargs, host_answer
from tests.svgf_common import (DEEP_LEVELS, DEEP_SHAPES, SVGF_DEEP_TERM_SETS, deep_filter, deep_frame, deep_variance, F, LEVELS, MANY_TILES, MIN_HISTORIES, RADII, SHAPES, SVGF_TERM_SETS, TILE_SHAPES, VARIANCE_TERM_SETS,
                               check_refusals, filter_inputs, filter_kwargs, history, host_filter, host_variance, inputs, mismatch, same_bits,
                               variance_kwargs)
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

LAYOUTS = [0, 1, 2]                                        # the measured choice, LDS tile wherever it fits, global memory
SHAPE_IDS = lambda s: f"{s[1]}x{s[0]}"
FULL = "var+all+albedo+emitted"


@pytest.fixture()
def layout(gpu, request):
    gpu.set_option(R.OPT_ATROUS_LAYOUT, request.param)
    yield request.param
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)


def check_variance(r, h, w, terms, min_history, radius):
    moments, length = history(h, w)
    got, st = r.variance_estimate(moments, length, **variance_kwargs(h, w, terms, min_history, radius))
    want = host_variance(h, w, terms, min_history, radius)
    assert same_bits(got, want), (terms, min_history, radius, mismatch(got, want))
    return st


def check_filter(r, h, w, terms, levels, prefilter):
    frame, variance = filter_inputs(h, w)
    got, got_v, st = r.svgf_filter(frame, variance, **filter_kwargs(h, w, terms, levels, prefilter))
    want, want_v = host_filter(h, w, terms, levels, prefilter)
    assert same_bits(got, want), (terms, levels, prefilter, mismatch(got, want))
    assert same_bits(got_v, want_v), (terms, levels, prefilter, mismatch(got_v, want_v))
    return st


# ---- 1. the matrix -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_variance_device_equals_host(gpu, shape, radius, layout):
    h, w = shape
    for min_history in MIN_HISTORIES:
        for terms in VARIANCE_TERM_SETS:
            st = check_variance(gpu, h, w, terms, min_history, radius)
            assert st.filter_ms > 0.0 and st.taps == R.variance_estimate(np.zeros((h, w, 2), F), np.ones((h, w), F), radius=radius)[1].taps


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_filter_device_equals_host(gpu, shape, levels, layout):
    h, w = shape
    for terms in SVGF_TERM_SETS:
        for prefilter in (0, 1):
            st = check_filter(gpu, h, w, terms, levels, prefilter)
            assert st.taps == R.atrous_filter(np.zeros((h, w, 3), F), levels=levels)[1].taps and st.filter_ms > 0.0


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("levels", DEEP_LEVELS)
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=SHAPE_IDS)
def test_filter_device_equals_host_with_taps_at_levels_7_and_8(gpu, shape, levels, layout):
    """259 pixels long, so that the taps of step 64 and step 128 land inside the frame and count (tests/test_svgf_cpu.py asserts that they
    do): 1 << i, 2^-i, the choice between tile and direct reads and the parity of the buffers at the last levels."""
    h, w = shape
    for terms in SVGF_DEEP_TERM_SETS:
        for prefilter in (0, 1):
            got, got_v, st = gpu.svgf_filter(deep_frame(h, w), deep_variance(h, w), **filter_kwargs(h, w, terms, levels, prefilter))
            want, want_v, taps = deep_filter(h, w, terms, levels, prefilter)
            assert same_bits(got, want), (terms, prefilter, mismatch(got, want))
            assert same_bits(got_v, want_v), (terms, prefilter, mismatch(got_v, want_v))
            assert st.taps == taps


# ---- 2. around the tile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("shape", TILE_SHAPES, ids=SHAPE_IDS)
def test_frames_around_the_tile(gpu, shape, layout):
    h, w = shape
    for terms, min_history, radius in (("all", 4, 3), ("none", 4, 1), ("all", 1, 2)):
        check_variance(gpu, h, w, terms, min_history, radius)
    for terms, levels, prefilter in ((FULL, 4, 1), ("var", 2, 0), ("var+guides+albedo+emitted", 5, 1)):
        check_filter(gpu, h, w, terms, levels, prefilter)


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_many_tiles(gpu, layout):
    """3 x 5 workgroups with ragged edges; five levels: the halo of the later ones spans several neighbours, and the last does not fit a tile."""
    h, w = MANY_TILES
    check_variance(gpu, h, w, "all", 4, 3)
    check_filter(gpu, h, w, FULL, 5, 1)
    check_filter(gpu, h, w, "var", 5, 0)


def test_a_workgroup_without_short_histories_skips_its_window(gpu):
    """The tile kernel fills its tile only where a pixel of the workgroup needs the window: a frame whose every history is long, and one with
    a single short pixel in one workgroup, under every layout."""
    h, w = MANY_TILES
    moments = history(h, w)[0]
    for poke in (None, (40, 50)):
        length = np.full((h, w), 9.0, F)
        if poke:
            length[poke] = 2.0
        kw = variance_kwargs(h, w, "all", 4, 3)
        want = R.variance_estimate(moments, length, **kw)[0]
        for lay in LAYOUTS:
            gpu.set_option(R.OPT_ATROUS_LAYOUT, lay)
            try:
                got = gpu.variance_estimate(moments, length, **kw)[0]
            finally:
                gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)
            assert same_bits(got, want), (poke, lay, mismatch(got, want))


# ---- 3. memory kinds ---------------------------------------------------------------------------------------------------------------------
V_NAMES = ["moments", "length", "depth", "normal", "ids", "out"]
F_NAMES = ["frame", "variance", "depth", "normal", "ids", "albedo", "emitted", "out", "out_variance"]
mask_id = lambda names: (lambda m: "".join(n[0] if m >> i & 1 else "-" for i, n in enumerate(names)))


@pytest.mark.parametrize("on_device", [0b000000, 0b111111, 0b010101, 0b101010, 0b100001, 0b011110], ids=mask_id(V_NAMES))
def test_variance_host_and_device_memory_mixed(gpu, torch, on_device):
    """Each argument independently a numpy array (staged) or a torch tensor (in place)."""
    h, w = 35, 67
    moments, length = history(h, w)
    kw = dict(variance_kwargs(h, w, "all", 4, 3), moments=moments, length=length)
    dev = torch.device("cuda:0")
    for i, name in enumerate(V_NAMES[:-1]):
        if on_device >> i & 1:
            kw[name] = torch.from_numpy(np.array(kw[name])).to(dev)
    out = torch.full((h, w), 7.0, device=dev) if on_device >> 5 & 1 else np.full((h, w), 7.0, F)
    got, _ = gpu.variance_estimate(**kw, out=out)
    assert got is out
    got = out.cpu().numpy() if hasattr(out, "cpu") else out
    want = host_variance(h, w, "all", 4, 3)
    assert same_bits(got, want), mismatch(got, want)


@pytest.mark.parametrize("on_device", [0b000000000, 0b111111111, 0b010101010, 0b101010101, 0b100000001, 0b011111110, 0b100000010, 0b010000001],
                         ids=mask_id(F_NAMES))
def test_filter_host_and_device_memory_mixed(gpu, torch, on_device):
    h, w = 35, 67
    frame, variance = filter_inputs(h, w)
    kw = dict(filter_kwargs(h, w, FULL, 4, 1), frame=frame, variance=variance)
    dev = torch.device("cuda:0")
    for i, name in enumerate(F_NAMES[:-2]):
        if on_device >> i & 1:
            kw[name] = torch.from_numpy(np.array(kw[name])).to(dev)
    out = torch.full((h, w, 3), 7.0, device=dev) if on_device >> 7 & 1 else np.full((h, w, 3), 7.0, F)
    out_v = torch.full((h, w), 7.0, device=dev) if on_device >> 8 & 1 else np.full((h, w), 7.0, F)
    got, got_v, _ = gpu.svgf_filter(**kw, out=out, out_variance=out_v)
    assert got is out and got_v is out_v
    got, got_v = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (out, out_v))
    want, want_v = host_filter(h, w, FULL, 4, 1)
    assert same_bits(got, want), mismatch(got, want)
    assert same_bits(got_v, want_v), mismatch(got_v, want_v)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_out_may_be_in(gpu, torch, device):
    h, w = 35, 67
    for terms, levels in ((FULL, 3), ("var", 1)):
        frame, variance = filter_inputs(h, w)
        frame = np.array(frame)
        if device:
            frame = torch.from_numpy(frame).to("cuda:0")
        out, out_v, _ = gpu.svgf_filter(frame, variance, **filter_kwargs(h, w, terms, levels, 1), out=frame)
        assert out is frame
        got = frame.cpu().numpy() if device else frame
        got_v = out_v.cpu().numpy() if device else out_v
        want, want_v = host_filter(h, w, terms, levels, 1)
        assert same_bits(got, want), (terms, mismatch(got, want))
        assert same_bits(got_v, want_v), (terms, mismatch(got_v, want_v))


# ---- 4. stream order and contexts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_tensors_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """Every buffer a tensor whose producer is still pending on the caller's stream when the call is made (tests/test_gpu_stream_order.py)."""
    h, w = 35, 67
    moments, length = history(h, w)
    frame, variance = filter_inputs(h, w)
    vkw, fkw = variance_kwargs(h, w, "all", 4, 3), filter_kwargs(h, w, FULL, 4, 1)
    want_e = host_variance(h, w, "all", 4, 3)
    want, want_v = host_filter(h, w, FULL, 4, 1)
    assert same_bits(ctx.variance_estimate(moments, length, **vkw)[0], want_e)       # own stream, host buffers: the scratch is as large as it gets
    assert same_bits(ctx.svgf_filter(frame, variance, **fkw)[0], want)
    on = lambda hz, kw: {k: (hz.input(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}

    hz = Hazard(torch, cycles_per_ms)
    t_moments, t_length, t_kw = hz.input(moments), hz.input(length, stale=np.ones((h, w), F)), on(hz, vkw)
    t_out = hz.output((h, w), torch.float32, 3.0, 5.0)
    (got,), _ = hz.run(ctx, kind, lambda: ctx.variance_estimate(t_moments, t_length, **t_kw, out=t_out))
    assert same_bits(got, want_e), mismatch(got, want_e)
    assert not same_bits(R.variance_estimate(np.zeros_like(moments), np.ones((h, w), F), **vkw)[0], want_e)      # (the stale answer is another)

    hz = Hazard(torch, cycles_per_ms)
    t_frame, t_variance, t_kw = hz.input(frame), hz.input(variance), on(hz, fkw)
    t_out, t_out_v = hz.output((h, w, 3), torch.float32, 3.0, 5.0), hz.output((h, w), torch.float32, 3.0, 5.0)
    (got, got_v), _ = hz.run(ctx, kind, lambda: ctx.svgf_filter(t_frame, t_variance, **t_kw, out=t_out, out_variance=t_out_v))
    assert same_bits(got, want), mismatch(got, want)
    assert same_bits(got_v, want_v), mismatch(got_v, want_v)
    assert not same_bits(R.svgf_filter(np.zeros_like(frame), np.zeros_like(variance), **fkw)[0], want)


def test_second_context_gives_the_same_bytes(gpu):
    h, w = 35, 67
    frame, variance = filter_inputs(h, w)
    first = gpu.svgf_filter(frame, variance, **filter_kwargs(h, w, FULL, 5, 1))
    with R.Renderer(0) as other:
        second = other.svgf_filter(frame, variance, **filter_kwargs(h, w, FULL, 5, 1))
        check_variance(other, h, w, "all", 4, 3)
        check_filter(other, 9, 17, "var+color", 3, 0)                      # (smaller frames on the grown scratch)
        check_variance(other, 9, 17, "all", 4, 3)
        check_filter(other, *MANY_TILES, FULL, 5, 1)                       # (and a larger one, which grows it again)
        check_filter(other, h, w, FULL, 5, 1)
    want, want_v = host_filter(h, w, FULL, 5, 1)
    for a, b in zip(first[:2], second[:2]):
        assert same_bits(a, b)
    assert same_bits(first[0], want) and same_bits(first[1], want_v)


def test_atrous_filter_on_the_scratch_these_calls_grew():
    """rtw_ctx_atrous_filter shares its scratch with the two new passes: it still writes the host form's bytes after they have grown it, on
    a smaller and on a larger frame, and between them."""
    with R.Renderer(0) as r:
        check_filter(r, 35, 67, FULL, 5, 1)
        check_variance(r, 35, 67, "all", 4, 3)
        for (h, w), terms, levels in (((35, 67), "all+albedo+emitted", 5), ((9, 17), "all", 3), ((35, 67), "color", 3)):
            got = r.atrous_filter(inputs(h, w)["frame"], **call_kwargs(h, w, terms, levels))[0]
            assert same_bits(got, host_answer(h, w, terms, levels)), (h, w, terms, mismatch(got, host_answer(h, w, terms, levels)))
        check_filter(r, 9, 17, "var", 3, 1)
        for terms in TERM_SETS:
            got = r.atrous_filter(inputs(35, 67)["frame"], **call_kwargs(35, 67, terms, 3))[0]
            assert same_bits(got, host_answer(35, 67, terms, 3)), (terms, mismatch(got, host_answer(35, 67, terms, 3)))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_error_paths_device(gpu):
    check_refusals(R.lib().rtw_ctx_variance_estimate, R.lib().rtw_ctx_svgf_filter, (gpu._h,))
    moments, length = history(9, 17)
    frame, variance = filter_inputs(9, 17)
    out = np.full((9, 17), 7.0, F)
    prm = R.C.byref(R.RtwVarianceEstimate(4, 3, 0.0, 0.0, 0))
    P = lambda a: R.C.c_void_p(a.ctypes.data)
    assert R.lib().rtw_ctx_variance_estimate(None, P(moments), P(length), 17, 9, None, None, None, prm, P(out), None) == -1      # no context
    assert R.lib().rtw_ctx_svgf_filter(None, P(frame), P(variance), 17, 9, None, None, None, None, None, R.C.byref(R.RtwAtrous(3, 0, 0, 0, 0, 0)),
                                       R.C.byref(R.RtwSvgf(1.0, 1e-6, 1)), P(np.empty((9, 17, 3), F)), P(out), None) == -1
    assert (out == 7.0).all()


# ---- 6. the sequence driver --------------------------------------------------------------------------------------------------------------
def test_the_denoiser_is_the_hand_chained_calls(gpu):
    """SvgfDenoiser.step over three frames of a moved camera at 67 x 35: every output is that of the calls chained by hand on the same
    rendered frame and guides, the filter stage through the host forms."""
    from tests.temporal_common import OFFSET, orbit
    from tests.test_oracle_golden import small_view
    w, h = 67, 35
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    p.samples, p.seed = 4, 30
    tkw = dict(alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1)
    skw = dict(levels=3, sigma_luminance=2.0, epsilon=1e-6, prefilter=True, sigma_depth=0.25, sigma_normal=0.3)
    den = R.SvgfDenoiser(gpu, **tkw)
    hist = None
    short = 0
    for k, deg in enumerate((0.0, 1.0, 2.0)):
        c = orbit(cam, deg)
        frame, acc, var, st = den.step(c, p, min_history=3, radius=2, **skw)
        assert p.seed == 31 + k and p.gamma == 1.0 and acc is den.history["color"]
        g = st["guides"]
        guides = dict(depth=g["depth"], normal=g["normal"], ids=g["idx"])
        hist, _, _ = gpu.temporal_accumulate(st["cur"], c, **guides, history=hist, offset=OFFSET, **tkw)
        for key in ("color", "moments", "len"):
            assert same_bits(den.history[key], hist[key]), (k, key)
        want_var = R.variance_estimate(hist["moments"], hist["len"], **guides, min_history=3, radius=2, sigma_depth=0.25, sigma_normal=0.3)[0]
        assert same_bits(var, want_var), (k, mismatch(var, want_var))
        want, want_fv, _ = R.svgf_filter(hist["color"], want_var, **guides, albedo=g["albedo"], emitted=g["emitted"], **skw)
        assert same_bits(frame, want), (k, mismatch(frame, want))
        assert same_bits(st["filtered_variance"], want_fv), (k, mismatch(st["filtered_variance"], want_fv))
        assert st["variance"].filter_ms > 0.0 and st["svgf"].filter_ms > 0.0 and st["temporal"].filter_ms > 0.0
        short += int((hist["len"] < 3).sum())
        assert (var > 0).mean() > 0.5, k                                    # (frame 0: the spatial estimate carries every pixel)
    assert short > w * h                                                    # both branches of the estimate were taken
    p.gamma = 2.0                                                           # the gamma is applied behind the filter, as render_denoised does
    frame2 = den.step(orbit(cam, 3.0), p, min_history=3, radius=2, **skw)[0]
    assert p.gamma == 2.0 and np.all(frame2[np.isfinite(frame2)] >= 0.0)


# ---- 7. quality: the one assertion -------------------------------------------------------------------------------------------------------
def test_the_defaults_beat_the_fixed_filter_on_the_accumulated_book1_orbit(gpu):
    """The Book-1 view of small_view(SCENE_C2, 400, 225, 4) under SAMPLER_ROW at gamma 1 along DESIGN.md 8d's orbit (0.25 degrees a frame):
    on frames 8 .. 11 the summed MSE against 4096-spp renders of SvgfDenoiser's frames (SVGF_DEFAULTS) is below that of TemporalDenoiser's
    (the fixed a-trous filter at ATROUS_DEFAULTS over the same accumulated frames).  Measured (scripts/measure_svgf.py, profiles/svgf.log):
    the ratio is 0.586 .. 0.591 over 8 sets of seeds -- the worst below 1 by 0.41, seventy times the spread of 0.006, where the rule for
    asserting it asks for twice."""
    from tests.temporal_common import orbit
    from tests.test_oracle_golden import small_view
    w, h = 400, 225
    scene, cam, p = small_view(R.SCENE_C2, w, h, 4)
    p.sampler, p.gamma, p.accel = R.SAMPLER_ROW, 1.0, R.ACCEL_BVH
    gpu.set_scene(scene)
    steered, fixed = R.SvgfDenoiser(gpu), R.TemporalDenoiser(gpu)
    new = old = 0.0
    for k in range(12):
        c = orbit(cam, 0.25 * k)
        p.samples, p.seed = 4, 500 + k
        a = steered.step(c, p)[0]
        p.seed = 500 + k                                                     # (step advances it: both chains see the same frame)
        b, acc = fixed.step(c, p)[:2]
        assert same_bits(acc, steered.history["color"])
        if k >= 8:
            p.samples, p.seed = 4096, 1
            truth = gpu.render(c, p)[0].astype(np.float64)
            new += float(((a - truth) ** 2).mean())
            old += float(((b - truth) ** 2).mean())
    print(f"\n[svgf quality] frames 8 .. 11: steered MSE {new / 4:.6f}, fixed {old / 4:.6f}, ratio {new / old:.3f}")
    assert new < old, (new, old)
