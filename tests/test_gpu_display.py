"""The display stage on the GPU (rtw_ctx_luminance_histogram, rtw_ctx_display, csrc/rtw_display.hip) against its host forms:
the histogram's counts exactly under every RTW_OPT_HISTOGRAM_COUNT, the display transform's bytes bit for bit over the whole parameter
matrix, at the sizes of the CPU tests (15 pixels: the tail alone) and at the smallest frame whose fourth-pixel groups wrap the histogram's
capped grid; numpy and torch memory, an input 12 bytes off 16-byte alignment and an RGB8 output one byte off, kinds mixed per argument;
the constant frame, the bin edges and a frame of NaN on the device, two calls in a row; torch producers still pending on the stream, a
second context, a scene left alone; DisplayTransform.step against the hand-chained calls and the float64 metering; the refusals.  The host
forms themselves are held to numpy restatements by tests/test_display_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.display_common import (F, SIZE_IDS, SIZES, all_params, bin_edge_column, noise, restate_exposure, same_bits, special_frame)
from tests.test_display_cpu import check_display_refusals, check_histogram_refusals
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 3]                                      # the measured choice, plain, per wave, ballot
SOME = [p for k, p in enumerate(all_params()) if k % 7 == 0] + [dict(tone=R.TONE_NONE, transfer=R.TRANSFER_GAMMA, gamma=1.0)]


@pytest.fixture()
def count(gpu, request):
    gpu.set_option(R.OPT_HISTOGRAM_COUNT, request.param)
    yield request.param
    gpu.set_option(R.OPT_HISTOGRAM_COUNT, 0)


def check_histogram(r, frame, dev_frame=None):
    """r.luminance_histogram of `dev_frame` (the frame itself unless given) against the host form's counts of `frame`."""
    want_h, want_c, _ = R.luminance_histogram(frame)
    hist, counts, st = r.luminance_histogram(frame if dev_frame is None else dev_frame)
    if hasattr(hist, "data_ptr"):
        hist, counts = hist.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
    assert np.array_equal(hist, want_h), np.flatnonzero(hist != want_h)
    assert np.array_equal(counts, want_c), (counts, want_c)
    assert st.taps == frame.shape[0] * frame.shape[1]
    return hist, counts


def check_display(r, frame, dev_frame=None, out=None, **prm):
    want = R.display(frame, **prm)[0]
    got, st = r.display(frame if dev_frame is None else dev_frame, out=out, **prm)
    if hasattr(got, "data_ptr"):
        got = got.cpu().numpy()
    assert same_bits(got, want), (prm, np.argwhere(got != want)[:4])
    return st


def wrap_size(torch):
    """The fewest pixels at which a thread's group of four pixels is a second pass of the capped grid (and one more: a tail pixel)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * R.HISTOGRAM_BLOCKS_PER_CU * R.HISTOGRAM_BLOCK_PIXELS + 4 + 1


# ---- 1. kernel against host form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS, indirect=True)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_histogram_device_equals_host(gpu, size, count):
    check_histogram(gpu, noise(*size))


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_display_device_equals_host(gpu, size):
    frame = noise(*size)
    frame[0, 0, 0] = -0.5
    for prm in all_params():
        st = check_display(gpu, frame, exposure=0.8, white=2.0, gamma=2.2, **prm)
        assert st.filter_ms > 0.0


def test_display_device_equals_host_on_special_values(gpu):
    frame = special_frame()
    for prm in all_params():
        check_display(gpu, frame, **prm)
    for white in (1e-30, 1e30):
        check_display(gpu, frame, tone=R.TONE_REINHARD_LUMA, white=white, out_format=R.DISPLAY_F32)
        check_display(gpu, frame, tone=R.TONE_REINHARD, white=white, out_format=R.DISPLAY_F32)


@pytest.fixture(scope="module")
def wrap_frame(torch):
    n = wrap_size(torch)
    rng = np.random.default_rng(7)
    return np.exp2(rng.uniform(-18.0, 17.0, (1, n, 3))).astype(F)


@pytest.mark.parametrize("count", COUNTS, indirect=True)
def test_histogram_wraps_the_capped_grid(gpu, wrap_frame, count):
    hist, counts = check_histogram(gpu, wrap_frame)
    assert hist[0] > 0 and hist[255] > 0


def test_display_beyond_the_histograms_grid(gpu, wrap_frame):
    for prm in (dict(out_format=R.DISPLAY_RGB8, dither=True), dict(out_format=R.DISPLAY_RGBA8), dict(out_format=R.DISPLAY_F32, tone=R.TONE_REINHARD_LUMA)):
        check_display(gpu, wrap_frame, **prm)


# ---- 2. memory kinds ---------------------------------------------------------------------------------------------------------------------------
def shifted(torch, frame, floats):
    """`frame` on the device in a tensor that starts `floats` floats into its allocation."""
    base = torch.zeros(frame.size + floats, dtype=torch.float32, device="cuda:0")
    t = base[floats:].view(*frame.shape)
    t.copy_(torch.from_numpy(frame))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 * floats) % 16
    return t


@pytest.mark.parametrize("size", [(5, 3), (64, 48), (257, 3)], ids=SIZE_IDS)
def test_memory_kinds(gpu, torch, size):
    w, h = size
    frame = noise(w, h)
    dev = torch.from_numpy(frame).to("cuda:0")
    off = shifted(torch, frame, 3)                                             # one pixel in: 12 bytes off 16-byte alignment
    host_off = np.zeros(frame.size + 3, F)[3:].reshape(frame.shape)            # a numpy view likewise (staged: aligned again on the device)
    host_off[...] = frame
    for f in (dev, off, host_off):
        check_histogram(gpu, frame, f)
        for prm in SOME:
            check_display(gpu, frame, f, **prm)
    # outputs: an RGB8 tensor one byte into its allocation, numpy outputs of tensor inputs and the other way round
    for prm in [p for p in SOME if p.get("out_format", R.DISPLAY_RGB8) == R.DISPLAY_RGB8]:
        odd = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device="cuda:0")[1:].view(h, w, 3)
        assert odd.data_ptr() % 4 == 1
        check_display(gpu, frame, dev, out=odd, **prm)
        check_display(gpu, frame, off, out=odd, **prm)
        check_display(gpu, frame, dev, out=np.empty((h, w, 3), np.uint8), **prm)
        check_display(gpu, frame, frame, out=torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0"), **prm)
    rgba = torch.zeros(h * w * 4 + 4, dtype=torch.uint8, device="cuda:0")[4:].view(h, w, 4)          # 4 bytes off 16
    check_display(gpu, frame, dev, out=rgba, out_format=R.DISPLAY_RGBA8)
    f32 = torch.zeros(h * w * 3 + 1, dtype=torch.float32, device="cuda:0")[1:].view(h, w, 3)
    check_display(gpu, frame, dev, out=f32, out_format=R.DISPLAY_F32)
    want_h, want_c, _ = R.luminance_histogram(frame)
    t_hist, n_counts = torch.full((256,), -1, dtype=torch.int32, device="cuda:0"), np.full(2, 9, np.uint32)
    gpu.luminance_histogram(dev, out_hist=t_hist, out_counts=n_counts)
    assert np.array_equal(t_hist.cpu().numpy().view(np.uint32), want_h) and np.array_equal(n_counts, want_c)
    n_hist, t_counts = np.full(256, 9, np.uint32), torch.full((2,), -1, dtype=torch.int32, device="cuda:0")
    gpu.luminance_histogram(frame, out_hist=n_hist, out_counts=t_counts)
    assert np.array_equal(n_hist, want_h) and np.array_equal(t_counts.cpu().numpy().view(np.uint32), want_c)


# ---- 3. the histogram's edges on the device --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS, indirect=True)
def test_histogram_edges_on_the_device(gpu, count):
    constant = np.full((48, 64, 3), 0.18, F)
    hist, counts = check_histogram(gpu, constant)                                # all lanes on one bin
    assert hist.max() == 64 * 48
    check_histogram(gpu, bin_edge_column())
    hist, counts = check_histogram(gpu, np.full((7, 33, 3), np.nan, F))
    assert counts.tolist() == [0, 7 * 33] and not hist.any()
    hist, counts = check_histogram(gpu, np.zeros((7, 33, 3), F))
    assert counts.tolist() == [7 * 33, 0]
    # two calls in a row, and again behind another frame: the counters start from zero every time
    a, b = noise(64, 48), noise(257, 3)
    for frame in (a, a, b, a, constant, constant):
        check_histogram(gpu, frame)


# ---- 4. stream order and contexts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_tensors_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """The frame and the outputs are tensors whose producers are still pending on the caller's stream when the calls are made
    (tests/test_gpu_stream_order.py): both passes read the new frame."""
    frame = noise(67, 35)
    prm = dict(tone=R.TONE_ACES_FIT, dither=True)
    want_h, want_c, _ = R.luminance_histogram(frame)
    want = R.display(frame, **prm)[0]
    check_histogram(ctx, frame)                                                  # own stream, host buffers: the scratch is grown
    hz = Hazard(torch, cycles_per_ms)
    t_frame = hz.input(frame)
    t_hist, t_counts = hz.output((256,), torch.int32, 3, 5), hz.output((2,), torch.int32, 3, 5)
    t_out = hz.output((35, 67, 3), torch.uint8, 3, 5)

    def calls():
        ctx.luminance_histogram(t_frame, out_hist=t_hist, out_counts=t_counts)
        ctx.display(t_frame, out=t_out, **prm)

    got, _ = hz.run(ctx, kind, calls)
    assert np.array_equal(got[0].view(np.uint32), want_h) and np.array_equal(got[1].view(np.uint32), want_c)
    assert np.array_equal(got[2], want)
    assert not np.array_equal(R.display(np.zeros_like(frame), **prm)[0], want)   # (the stale answer is another)


def test_second_context_gives_the_same_bytes(gpu):
    frame = noise(64, 48)
    check_histogram(gpu, frame)
    with R.Renderer(0) as other:
        check_histogram(other, frame)
        for prm in SOME:
            check_display(other, frame, **prm)
        check_display(other, noise(5, 3))                                        # (a smaller frame on the grown scratch)
        check_display(other, noise(257, 3), out_format=R.DISPLAY_F32)
        check_histogram(other, noise(257, 3))


def test_the_scene_is_left_alone(gpu):
    from tests.test_oracle_golden import small_view
    scene, cam, p = small_view(R.SCENE_C2, 64, 48, 4)
    p.accel = R.ACCEL_BVH
    gpu.set_scene(scene)
    before = gpu.render(cam, p)[0]
    check_histogram(gpu, before)
    check_display(gpu, before)
    check_display(gpu, before, out_format=R.DISPLAY_F32, tone=R.TONE_REINHARD)
    assert np.array_equal(gpu.render(cam, p)[0], before)


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------------------
def test_display_transform_step(gpu):
    frames = [noise(64, 48, seed=k, top=t) for k, t in ((0, 4.0), (1, 64.0), (2, 0.25))]
    prm = dict(tone=R.TONE_REINHARD_LUMA, white=3.0, dither=True)
    met = dict(rate=0.5, low_permille=100, high_permille=20, key=0.25)
    dt = R.DisplayTransform(gpu, **prm, **met)
    level, exposure = None, 1.0
    for k, frame in enumerate(frames):
        out, lv, ex, stats = dt.step(frame)
        hist, counts, _ = gpu.luminance_histogram(frame)                         # the three calls, chained by hand
        level_h, exposure_h = R.exposure_from_histogram(hist, prev_level=level, prev_exposure=exposure, **met)
        want = gpu.display(frame, exposure=exposure_h, **prm)[0]
        assert np.array_equal(out, want) and (lv, ex) == (level_h, exposure_h)
        assert np.array_equal(stats["hist"], hist) and np.array_equal(stats["counts"], counts)
        wl, we = restate_exposure(R.luminance_histogram(frame)[0], prev_level=level, prev_exposure=exposure, **met)
        assert np.float64(lv).tobytes() == np.float64(wl).tobytes() and F(ex).tobytes() == F(we).tobytes(), k
        level, exposure = lv, ex
    assert dt.level == level
    dt.reset()
    assert dt.step(frames[0])[1] == R.exposure_from_histogram(R.luminance_histogram(frames[0])[0], **met)[0]
    black = R.DisplayTransform(gpu)
    out, lv, ex, _ = black.step(np.zeros((3, 5, 3), F))                           # nothing counted on a first frame
    assert lv is None and ex == 1.0 and not out.any()
    with pytest.raises(TypeError):
        R.DisplayTransform(gpu, exposure=2.0)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_error_paths_device(gpu):
    check_histogram_refusals(R.lib().rtw_ctx_luminance_histogram, (gpu._h,))
    check_display_refusals(R.lib().rtw_ctx_display, (gpu._h,))
    frame = noise(5, 3)
    P = lambda a: R.C.c_void_p(a.ctypes.data)
    hist, counts, out = np.full(256, 7, np.uint32), np.full(2, 7, np.uint32), np.full((3, 5, 3), 7, np.uint8)
    prm = R.RtwDisplay(1.0, 0, 1.0, 0, 1.0, 0, 0, 0)
    assert R.lib().rtw_ctx_luminance_histogram(None, P(frame), 5, 3, P(hist), P(counts), None) == -1
    assert R.lib().rtw_ctx_display(None, P(frame), 5, 3, R.C.byref(prm), P(out), None) == -1
    assert (hist == 7).all() and (counts == 7).all() and (out == 7).all()      # no context
    with pytest.raises(R.RtwError):
        gpu.set_option(R.OPT_HISTOGRAM_COUNT, 4)
    with pytest.raises(ValueError):
        gpu.display(frame, out=np.empty((3, 5, 4), np.uint8))                  # RGB8 wants [h][w][3]
