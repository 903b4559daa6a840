"""Bloom on the GPU (rtw_ctx_bloom, csrc/rtw_bloom.hip) against its host form, bit for bit: at the sizes of the CPU tests under
every RTW_OPT_ATROUS_LAYOUT, levels 1, 2 and 8, the Karis weight on and off, with the layer and in place; a frame of more than 16 tiles a
side that uses all 8 levels and one whose chain stops at 1 x 1; the special values and the known answers on the device; numpy and torch
memory, a tensor 12 bytes off 16-byte alignment, kinds mixed per argument; calls in a row over a pyramid that is regrown; a torch producer
still pending on the stream, a second context, a scene left alone; DisplayTransform(bloom=...) against the hand-chained calls; the refusals.
The host form itself is held to numpy restatements by tests/test_bloom_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.bloom_common import F, PARAM_SETS, SIZE_IDS, SIZES, noise, same_bits, special_frame
from tests.test_bloom_cpu import check_bloom_refusals
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

LAYOUTS = [0, 1, 2]                                        # the measured choice, LDS tiles, global memory
_HOST = {}


def host(frame, **prm):
    """The host form's (out, layer, taps) of a frame, computed once per frame and parameters."""
    key = (frame.shape, frame.tobytes(), tuple(sorted(prm.items())))
    if key not in _HOST:
        out, layer, st = R.bloom(frame, layer=True, **prm)
        out.setflags(write=False)
        layer.setflags(write=False)
        _HOST[key] = (out, layer, st.taps)
    return _HOST[key]


@pytest.fixture()
def layout(gpu, request):
    gpu.set_option(R.OPT_ATROUS_LAYOUT, request.param)
    yield request.param
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def check_bloom(r, frame, dev_frame=None, out=None, layer=True, **prm):
    """r.bloom of `dev_frame` (the frame itself unless given) against the host form of `frame`."""
    want_out, want_layer, taps = host(frame, **prm)
    got, lay, st = r.bloom(frame if dev_frame is None else dev_frame, out=out, layer=layer, **prm)
    got = numpy_of(got)
    assert same_bits(got, want_out), (prm, np.argwhere(got != want_out)[:4])
    if lay is not None:
        lay = numpy_of(lay)
        assert same_bits(lay, want_layer), (prm, np.argwhere(lay != want_layer)[:4])
    assert st.taps == taps and st.filter_ms > 0.0
    return st


# ---- 1. kernel against host form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_device_equals_host(gpu, size, layout):
    frame = noise(*size)
    for levels in (1, 2, 8):
        for ps in PARAM_SETS[3::4]:                                             # the ordinary knee, Karis off and on
            check_bloom(gpu, frame, levels=levels, **ps)
    for ps in PARAM_SETS:
        check_bloom(gpu, frame, layer=False, levels=3, **ps)
    buf = frame.copy()                                                          # out is in
    check_bloom(gpu, frame, dev_frame=buf, out=buf, levels=8)
    assert same_bits(buf, host(frame, levels=8)[0])


@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
@pytest.mark.parametrize("size", [(530, 275), (40, 24)], ids=SIZE_IDS)
def test_larger_frames(gpu, size, layout):
    w, h = size
    sizes = R.bloom_levels(w, h, 8)
    if size == (530, 275):
        assert len(sizes) == 8 and sizes[-1] != (1, 1)                          # all eight levels used
        assert sizes[0][0] > 16 * 16 and sizes[0][0] % 16 and sizes[0][1] % 16  # more than 16 tiles across, no multiple of a tile
    else:
        assert len(sizes) < 8 and sizes[-1] == (1, 1)                           # the early stop
    frame = noise(w, h)
    check_bloom(gpu, frame, levels=8)
    check_bloom(gpu, frame, levels=8, karis=False, threshold=0.0, knee=0.0, spread=1.0)


# ---- 2. special values and known answers on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_special_values_and_known_answers(gpu, layout):
    frame = special_frame()
    for ps in PARAM_SETS:
        check_bloom(gpu, frame, levels=3, **ps)
    big = np.full((5, 7, 3), 3e38, F)
    big[2, 3] = 1.0
    check_bloom(gpu, big, levels=2)
    constant = np.full((48, 64, 3), 0.75, F)
    n = len(R.bloom_levels(64, 48, 8))
    out, layer, _ = gpu.bloom(constant, layer=True, levels=8, threshold=0.0, knee=0.0, karis=False, spread=0.5, intensity=0.25)
    want = F(0.75 * (2.0 - 2.0 ** (1 - n)))
    assert (layer == want).all() and (out == F(0.75) + F(0.25) * want).all()
    dim = noise(65, 35, top=0.4)
    out, layer, _ = gpu.bloom(dim, layer=True, threshold=1.0, knee=0.5, intensity=7.0)
    assert not layer.any() and same_bits(out, dim)                              # wholly below threshold - knee: out == in
    out, layer, _ = gpu.bloom(np.full((7, 33, 3), np.nan, F), layer=True)
    assert not layer.any() and np.isnan(out).all()


# ---- 3. memory kinds ---------------------------------------------------------------------------------------------------------------------------
def shifted(torch, frame, floats):
    """`frame` on the device in a tensor that starts `floats` floats into its allocation."""
    base = torch.zeros(frame.size + floats, dtype=torch.float32, device="cuda:0")
    t = base[floats:].view(*frame.shape)
    t.copy_(torch.from_numpy(frame))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 * floats) % 16
    return t


@pytest.mark.parametrize("size", [(5, 3), (65, 35)], ids=SIZE_IDS)
def test_memory_kinds(gpu, torch, size):
    w, h = size
    frame = noise(w, h)
    dev = torch.from_numpy(frame).to("cuda:0")
    off = shifted(torch, frame, 3)                                              # one pixel in: 12 bytes off 16-byte alignment
    new_t = lambda: torch.full((h, w, 3), 9.0, dtype=torch.float32, device="cuda:0")
    new_n = lambda: np.full((h, w, 3), 9.0, F)
    for f in (frame, dev, off):
        check_bloom(gpu, frame, f)                                              # out=None: like the frame
        check_bloom(gpu, frame, f, layer=False)
    out, layer, _ = gpu.bloom(dev, layer=True)
    assert hasattr(out, "data_ptr") and hasattr(layer, "data_ptr")
    out, layer, _ = gpu.bloom(frame, layer=True)
    assert isinstance(out, np.ndarray) and isinstance(layer, np.ndarray)
    # kinds mixed between in, out and layer_out
    for f, o, l in ((dev, new_n(), new_t()), (frame, new_t(), new_n()), (off, new_t(), new_t()), (dev, new_n(), new_n()), (frame, new_n(), new_t()),
                    (dev, shifted(torch, frame, 1), shifted(torch, frame, 2))):
        check_bloom(gpu, frame, f, out=o, layer=l)
    in_place = dev.clone()
    check_bloom(gpu, frame, in_place, out=in_place)
    assert same_bits(in_place.cpu().numpy(), host(frame)[0])
    assert same_bits(dev.cpu().numpy(), frame) and same_bits(off.cpu().numpy(), frame)   # the inputs are read only


# ---- 4. calls in a row ---------------------------------------------------------------------------------------------------------------------------
def test_calls_in_a_row(gpu):
    large, small, larger = noise(65, 35), noise(5, 3), noise(130, 70)
    with R.Renderer(0) as r:                                                    # a context whose pyramid starts empty
        for frame in (large, small, larger, small, large, large):
            check_bloom(r, frame, levels=8)
            check_bloom(r, frame, levels=2, karis=False)


# ---- 5. stream order and contexts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_tensors_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """The frame and the outputs are tensors whose producers are still pending on the caller's stream when the call is made
    (tests/test_gpu_stream_order.py): every step reads the new frame."""
    frame = noise(67, 35)
    want_out, want_layer, _ = host(frame)
    check_bloom(ctx, frame)                                                     # own stream, host buffers: the scratch is grown
    hz = Hazard(torch, cycles_per_ms)
    t_frame = hz.input(frame)
    t_out, t_layer = hz.output((35, 67, 3), torch.float32, 3.0, 5.0), hz.output((35, 67, 3), torch.float32, 3.0, 5.0)
    got, _ = hz.run(ctx, kind, lambda: ctx.bloom(t_frame, out=t_out, layer=t_layer))
    assert same_bits(got[0], want_out) and same_bits(got[1], want_layer)
    assert not same_bits(R.bloom(np.zeros_like(frame))[0], want_out)            # (the stale answer is another)


def test_second_context_gives_the_same_bytes(gpu):
    frame = noise(64, 48)
    check_bloom(gpu, frame)
    with R.Renderer(0) as other:
        check_bloom(other, frame)
        check_bloom(other, noise(5, 3))                                         # (a smaller frame on the grown scratch)
        check_bloom(other, noise(257, 3), levels=8)
    check_bloom(gpu, frame)


def test_the_scene_is_left_alone(gpu):
    from tests.test_oracle_golden import small_view
    scene, cam, p = small_view(R.SCENE_C2, 64, 48, 4)
    p.accel = R.ACCEL_BVH
    gpu.set_scene(scene)
    before = gpu.render(cam, p)[0]
    check_bloom(gpu, before, threshold=0.5, knee=0.25)
    check_bloom(gpu, before, levels=8, karis=False, threshold=0.0, knee=0.0)
    assert np.array_equal(gpu.render(cam, p)[0], before)


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------------------
def test_display_transform_with_bloom(gpu):
    frames = [noise(64, 48, seed=k, top=t) for k, t in ((0, 256.0), (1, 4096.0), (2, 16.0))]
    prm = dict(tone=R.TONE_REINHARD_LUMA, white=3.0, dither=True)
    met = dict(rate=0.5, low_permille=100, high_permille=20, key=0.25)
    blm = dict(levels=4, threshold=0.8, knee=0.4, intensity=0.5)
    with_bloom, without = R.DisplayTransform(gpu, bloom=blm, **prm, **met), R.DisplayTransform(gpu, **prm, **met)
    level, exposure = None, 1.0
    for frame in frames:
        out, lv, ex, stats = with_bloom.step(frame)
        hist, counts, _ = gpu.luminance_histogram(frame)                        # the calls, chained by hand
        level, exposure = R.exposure_from_histogram(hist, prev_level=level, prev_exposure=exposure, **met)
        e = F(exposure)
        bloomed = gpu.bloom(frame, **dict(blm, threshold=float(F(0.8) / e), knee=float(F(0.4) / e)))[0]
        assert not same_bits(bloomed, frame)                                    # (the bloom does something here)
        assert np.array_equal(out, gpu.display(bloomed, exposure=exposure, **prm)[0]) and (lv, ex) == (level, exposure)
        assert np.array_equal(stats["hist"], hist) and stats["bloom"].taps == host(frame, levels=4)[2]
        # bloom=None: histogram, exposure, display as before
        out0, lv0, ex0, stats0 = without.step(frame)
        assert np.array_equal(out0, gpu.display(frame, exposure=exposure, **prm)[0]) and (lv0, ex0) == (level, exposure)
        assert sorted(stats0) == ["counts", "display", "hist", "histogram"]
    t_frame = __import__("torch").from_numpy(frames[0]).to("cuda:0")          # a device frame stays on the device
    with_bloom.reset()
    out_t = with_bloom.step(t_frame)[0]
    with_bloom.reset()
    assert hasattr(out_t, "data_ptr") and np.array_equal(out_t.cpu().numpy(), with_bloom.step(frames[0])[0])


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_error_paths_device(gpu):
    check_bloom_refusals(R.lib().rtw_ctx_bloom, (gpu._h,))
    frame = noise(5, 3)
    P = lambda a: R.C.c_void_p(a.ctypes.data)
    out = np.full((3, 5, 3), 7.0, F)
    prm = R.RtwBloom(2, 1.0, 0.5, 1, 0.5, 0.25)
    assert R.lib().rtw_ctx_bloom(None, P(frame), 5, 3, R.C.byref(prm), P(out), None, None) == -1
    assert (out == 7).all()                                                     # no context
    with pytest.raises(ValueError):
        gpu.bloom(frame, out=np.empty((3, 5, 4), F))
    with pytest.raises(R.RtwError):
        gpu.bloom(frame, levels=9)
