"""Temporal accumulation on the GPU (rtw_ctx_temporal_accumulate, csrc/rtw_temporal.hip) against the host form, bit for bit (as
tests/temporal_common.py defines it: the same bits, or NaN on both sides): the CPU tests' cases at their four sizes -- 33 x 17 and 67 x 35
cross the 32 x 8 workgroup in both directions -- with numpy arrays and with torch tensors in place, out_color == cur, two sizes in a row on
one context, frames around the 32 x 8 workgroup, a ragged many-tile frame, the declared limit of 65535 in either direction, host and device
memory mixed per buffer, torch tensors behind use_torch_stream, a second context, the refusals, the reprojection against float64 geometry
(tests/temporal_geometry_common.py), and rendered views: a static camera, whose accumulation is the running mean of its frames bit for
bit, a small orbit through TemporalDenoiser, and two views of an analytically known scene, where the surface buffers and the rule must
mean the same depth.  The host form itself is held to a numpy restatement by tests/test_temporal_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.temporal_common import (ALL_OFF, ALL_ON, BUFFERS, CASE_NAMES, F, GEO_POSES, OFFSET, OUT_BUFFERS, OUT_KEYS, SENTINEL, SHAPES,
                                   TEMPORAL_TEST_DEFAULTS, assert_same_runs, c_call, cases, dyadic_camera, frame, host_answer, mismatch, orbit,
                                   raw_call, refusal_calls, run, same_bits, second_frame_buffers, turned)
from tests.temporal_geometry_common import (GEO_CASES, GEO_SHAPES, RENDERED_H, RENDERED_MAXT, RENDERED_MINT, RENDERED_SPHERES, RENDERED_TOL,
                                            RENDERED_UNDECIDED_MOST, RENDERED_W, analytic_guides, check_plane, check_probe,
                                            check_static_is_continuous, plane_case, probe, probe_case, rendered_cameras, rendered_sets)
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

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


# ---- 1b. the kernel's edges -----------------------------------------------------------------------------------------------------------------
TILE_W, TILE_H = 32, 8                                     # the kernel's workgroup (csrc/rtw_temporal.hip TBX, TBY)
TILE_SHAPES = [(h, w) for h in (TILE_H - 1, TILE_H, TILE_H + 1) for w in (TILE_W - 1, TILE_W, TILE_W + 1)]
MANY_TILES = (4 * TILE_H + 3, 2 * TILE_W + 7)              # 71 x 35: 3 x 5 ragged workgroups
LIMIT = 65535                                              # RTW_TEMPORAL_MAX_SIDE


@pytest.mark.parametrize("shape", TILE_SHAPES + [MANY_TILES], ids=shape_ids)
def test_frames_around_the_workgroup(gpu, shape):
    h, w = shape
    for name in ("terms-all", "holes-turned"):
        frames, params = cases(h, w)[name]
        assert_same_runs(run(gpu.temporal_accumulate, frames, params), host_answer(h, w, name), name)


@pytest.mark.parametrize("moved", [False, True], ids=["static", "moved"])
@pytest.mark.parametrize("shape", [(1, LIMIT), (LIMIT, 1)], ids=shape_ids)
def test_frames_at_the_declared_limit(gpu, shape, moved):
    """65535 x 1 is 2048 workgroups in a row with a ragged last one, 1 x 65535 is 8192 in a column that use one row of their eight; under
    the static camera every pixel keeps its history, under the moved one (every term off) some do; then a 5 x 3 frame on the same context."""
    h, w = shape
    A = dyadic_camera(h, w)
    frames = [frame(h, w, 0, A), frame(h, w, 1, turned(A, 0.4, (0.01, 0.0, 0.02)) if moved else A)]
    params = dict(TEMPORAL_TEST_DEFAULTS, **(ALL_OFF if moved else ALL_ON))
    want = run(R.temporal_accumulate, frames, params)
    kept = float((want[1]["len"] > 1).mean())
    assert (0.0 < kept < 1.0) if moved else kept == 1.0, kept
    assert_same_runs(run(gpu.temporal_accumulate, frames, params), want, (shape, moved))
    frames, params = cases(3, 5)["terms-all"]
    assert_same_runs(run(gpu.temporal_accumulate, frames, params), host_answer(3, 5, "terms-all"), "5x3 after the limit")


# ---- 1c. memory kinds -------------------------------------------------------------------------------------------------------------------
N_IN = 10
ALL = (1 << len(BUFFERS)) - 1
OUTPUTS_ONLY, HISTORY_ONLY = ALL & ~((1 << N_IN) - 1), 0b1111110000
MASKS = [(0, False), (ALL, False), (0b01010101010101, False), (0b10101010101010, False), (OUTPUTS_ONLY, False), (HISTORY_ONLY, False),
         (0, True), (ALL, True)]
mask_id = lambda m: "".join("d" if m[0] >> i & 1 else "h" for i in range(len(BUFFERS))) + ("+out_color-is-cur" if m[1] else "")


@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
def test_host_and_device_memory_mixed(gpu, torch, mask):
    """Each of the 14 buffers (temporal_common.BUFFERS, in the order of the ids' letters) independently host memory (staged) or device
    memory (in place), through the C call; and out_color == cur on either side."""
    on_device, alias = mask
    h, w = 35, 67
    buf, cam, prev_cam, params, want = second_frame_buffers(h, w, "terms-all")
    held = {}
    for i, name in enumerate(BUFFERS):
        held[name] = torch.from_numpy(np.array(buf[name])).to("cuda:0") if on_device >> i & 1 else np.array(buf[name])
    if alias:
        held["out_color"] = held["cur"]
    address = {k: (v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data) for k, v in held.items()}
    torch.cuda.synchronize()
    assert c_call(R.lib().rtw_ctx_temporal_accumulate, (gpu._h,), h, w, cam, prev_cam, address, params) == 0
    for name, key in OUT_BUFFERS.items():
        got = held[name].cpu().numpy() if hasattr(held[name], "cpu") else held[name]
        assert same_bits(got, want[key]), (name, mismatch(got, want[key]))
    for name in BUFFERS[:N_IN]:                                                      # (the inputs are only read)
        if not (alias and name == "cur"):
            got = held[name].cpu().numpy() if hasattr(held[name], "cpu") else held[name]
            assert same_bits(got, buf[name]), name


# ---- 1d. stream order and contexts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_torch_tensors_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """Every buffer a tensor whose producer is still pending on the caller's stream when the call is made (tests/test_gpu_stream_order.py):
    the ten inputs hold stale data until then -- zeros, and a history of length 1 everywhere, whose answer is another --, and each of the
    four outputs is filled behind the delay."""
    h, w = 35, 67
    frames, params = cases(h, w)["terms-all"]
    assert_same_runs(run(ctx.temporal_accumulate, frames, params), host_answer(h, w, "terms-all"), "own stream")      # host buffers: the scratch is as large as it gets
    buf, cam, prev_cam, params, want = second_frame_buffers(h, w, "terms-all")
    stale = {k: np.zeros_like(buf[k]) for k in BUFFERS[:N_IN]}
    stale["prev_len"] = np.ones((h, w), F)
    hz = Hazard(torch, cycles_per_ms)
    t = {k: hz.input(buf[k], stale=stale[k]) for k in BUFFERS[:N_IN]}
    t.update({k: hz.output(buf[k].shape, torch.float32, 3.0, 5.0) for k in BUFFERS[N_IN:]})
    address = {k: v.data_ptr() for k, v in t.items()}
    got, rc = hz.run(ctx, kind, lambda: c_call(R.lib().rtw_ctx_temporal_accumulate, (ctx._h,), h, w, cam, prev_cam, address, params))
    assert rc == 0
    for g, key in zip(got, OUT_BUFFERS.values()):
        assert same_bits(g, want[key]), (key, mismatch(g, want[key]))
    old = dict(stale, **{k: np.empty_like(buf[k]) for k in BUFFERS[N_IN:]})
    assert c_call(R.lib().rtw_temporal_accumulate, (), h, w, cam, prev_cam, {k: v.ctypes.data for k, v in old.items()}, params) == 0
    assert not same_bits(old["out_color"], want["color"]) and not same_bits(old["out_moments"], want["moments"])      # (the stale answer is another)


def test_second_context_gives_the_same_bytes(gpu):
    h, w = 35, 67
    frames, params = cases(h, w)["terms-all"]
    first = run(gpu.temporal_accumulate, frames, params)
    with R.Renderer(0) as other:
        second = run(other.temporal_accumulate, frames, params)
    assert_same_runs(first, second, "two contexts")
    assert_same_runs(first, host_answer(h, w, "terms-all"), "the host form")


# ---- 1e. the reprojection against float64 geometry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GEO_SHAPES, ids=shape_ids)
def test_reprojection_against_float64_geometry(gpu, shape):
    """The kernel's fx, fy, candidate test and s, read out through a ramp history (tests/temporal_geometry_common.py), against the float64
    solve on every camera pair and offset; and its bytes against the host form's, NaN frame and hand-made history included."""
    h, w = shape
    for case in GEO_CASES:
        c = probe_case(h, w, *case)
        check_probe(gpu.temporal_accumulate, c, f"device {w}x{h} {case}")
        check_plane(gpu.temporal_accumulate, plane_case(h, w, *case), f"device {w}x{h} {case}")
        for got, want in zip(probe(gpu.temporal_accumulate, c), probe(R.temporal_accumulate, c)):
            assert same_bits(got, want), (case, mismatch(got, want))


@pytest.mark.parametrize("shape", GEO_SHAPES, ids=shape_ids)
def test_static_shortcut_is_continuous_with_the_general_path(gpu, shape):
    h, w = shape
    for cam_name in GEO_POSES:
        check_static_is_continuous(gpu.temporal_accumulate, h, w, cam_name, f"device {w}x{h} {cam_name}")


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


def test_rendered_guides_and_the_rule_mean_the_same_depth(gpu):
    """A few spheres on a ground sphere, two Viewport cameras two degrees apart on an orbit, 64 x 36, the guides of both from surface_map,
    the depth and object tests on.  The float64 reference (tests/temporal_geometry_common.py: rendered_sets) projects each current pixel's
    point, from its float32 depth, into the previous view and intersects the previous camera's rays through the four integer taps with
    the spheres analytically: a pixel whose taps all hit its own object at depths within half of depth_tol of s must keep its history
    (len 2), one that projects more than a pixel outside the previous frame must start again (len 1).  A depth of surface_map in another
    unit than the rule's s -- along a normalised ray, say, or from another offset -- fails the first."""
    scene = R.Scene([R.Sphere.with_albedo(c, r, (0.5, 0.5, 0.5)) for c, r in RENDERED_SPHERES])
    cam, prev_cam = rendered_cameras()
    h, w = RENDERED_H, RENDERED_W
    gpu.set_scene(scene)
    g1, g0 = (gpu.surface_map(c, w, h, RENDERED_MINT, RENDERED_MAXT, R.INTEGRATOR_BG_COLOR, R.RAYS_PIXEL, OFFSET) for c in (cam, prev_cam))
    want_depth, want_idx = analytic_guides(cam, OFFSET)
    assert (g1["idx"] == want_idx).mean() > 0.99 and np.abs(g1["depth"] / want_depth - 1.0)[g1["idx"] == want_idx].max() < 1e-3
    rng = np.random.default_rng(12)
    kw = dict(TEMPORAL_TEST_DEFAULTS, depth_tol=RENDERED_TOL, normal_cos=0.0, same_object=1, offset=OFFSET)
    hist, _, _ = gpu.temporal_accumulate(rng.random((h, w, 3)).astype(F), prev_cam, depth=g0["depth"], ids=g0["idx"], **kw)
    assert np.all(hist["len"] == 1)
    hist, _, _ = gpu.temporal_accumulate(rng.random((h, w, 3)).astype(F), cam, depth=g1["depth"], ids=g1["idx"], history=hist, **kw)
    keep, reset = rendered_sets(cam, prev_cam, g1["depth"], g1["idx"], OFFSET)
    undecided = 1.0 - float(keep.mean()) - float(reset.mean())
    print(f"\n[temporal, rendered] must keep {keep.mean():.3f}, must reset {reset.mean():.4f}, undecided {undecided:.3f}; kept {(hist['len'] == 2).mean():.3f}")
    assert keep.any() and reset.any() and undecided <= RENDERED_UNDECIDED_MOST
    assert np.all(hist["len"][keep] == 2), int((hist["len"][keep] != 2).sum())
    assert np.all(hist["len"][reset] == 1), int((hist["len"][reset] != 1).sum())
