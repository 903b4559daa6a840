"""rtw_ctx_set_stream: every call of a context that uses its stream, made at once behind a busy producer on the caller's stream -- a torch
side stream by its raw handle, torch's default stream through Renderer.use_torch_stream, and the stream that is current at the time of
use_torch_stream() -- with no synchronise in between.

Each case enqueues on the stream S a delay (torch.cuda._sleep), then the producers of the call's device buffers: `t_in.copy_(t_src)` for an
input (read after write: a call that ran early reads the stale, valid data the buffer held before) and `t_out.fill_(..)` for an output
(write after write: a call that ran early has its answer overwritten by the late fill), then an event.  The context is pointed at S and
the call is made while that event is still pending -- a case whose event has already fired FAILS ("delay too short"), it does not pass.
The answer is compared on the bits with one from outside the path under test: the host filters, the CPU oracle's render, or the same query
on a fresh context on its own stream.  When the call returns the event must have fired (the call waits for its stream), and a torch op on S
that reads the output sees the same bytes.

Nothing here asserts what an unordered run gives.  The module's context is its own (never the session's `gpu`), it has made every call once
on its own stream before a case times anything (so that no first-use allocation or free -- a device-wide wait -- hides a missing order), and
every case sets the own stream back in a `finally`.

The delay.  torch.cuda._sleep spins for a number of device clock cycles; `cycles_per_ms` times a fixed sleep once per module with two events
and scales from it.  The delay has to outlast the host time between the first enqueue on S and the rtw call.  Measured on an MI355X over
this module's cases (time.perf_counter, printed by every case): the largest gap of two runs was 0.148 ms (0.12 .. 0.15 ms in the module's
first two cases, 0.007 .. 0.08 ms in the others), with the stream's first launch -- which brings its hardware queue up, 0.3 .. 5 ms --
made and waited for before the clock starts.  100 times that is 14.8 ms, so DELAY_MS is the floor of 20 ms."""
import ctypes as C
import time

import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests.guided_common import SIGMA_DEPTH, SIGMA_NORMAL, as_f32_frame, case_image, guides
from tests.test_oracle_golden import small_view

pytestmark = pytest.mark.gpu

F = np.float32
DELAY_MS = 20.0
KINDS = ["side-raw-handle", "torch-default", "torch-current"]
MINT, MAXT = 0.001, 1000.0
H, W, SIZE = 48, 64, 4                                   # the filters' frame: 64 x 48, size 4
GAPS = []                                                # host ms between the first enqueue on S and the call, case by case


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def cycles_per_ms(torch):
    """Device clock cycles of torch.cuda._sleep per millisecond: a fixed sleep between two events, lengthened until it is well above the
    cost of a launch."""
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)                               # (the kernel's first launch)
    cycles, ms = 250_000, 0.0
    for _ in range(8):
        cycles *= 4
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 5.0:
            break
    assert ms >= 5.0, (cycles, ms)
    return cycles / ms


@pytest.fixture(scope="module")
def ctx():
    """This module's context."""
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    with R.Renderer(0) as r:
        yield r


def fresh(step):
    """step(r) on a context created for it, on its own stream, after everything of torch's is done."""
    import torch
    torch.cuda.synchronize()
    with R.Renderer(0) as r:
        return step(r)


class Hazard:
    """One case: the device buffers of a call, their producers, and the checks around the call."""

    def __init__(self, torch, cycles_per_ms):
        self.torch, self.cycles = torch, int(cycles_per_ms * DELAY_MS)
        self.dev = torch.device("cuda:0")
        self.inputs, self.outputs = [], []

    def input(self, array, stale=None):
        """A device input that holds `stale` (zeros unless given) until the producer on S copies `array` into it."""
        src = self.torch.from_numpy(np.ascontiguousarray(array)).to(self.dev)
        t = self.torch.zeros_like(src) if stale is None else self.torch.from_numpy(np.ascontiguousarray(stale)).to(self.dev)
        assert t.shape == src.shape and t.dtype == src.dtype
        self.inputs.append((t, src))
        return t

    def output(self, shape, dtype, first, late):
        """A device output that holds `first` until the producer on S fills it with `late`; the call's answer holds neither."""
        t = self.torch.full(shape, first, dtype=dtype, device=self.dev)
        self.outputs.append((t, late))
        return t

    def run(self, ctx, kind, call):
        """Enqueue delay and producers on S, point `ctx` at S, make the call while they are pending; the outputs as numpy arrays."""
        torch = self.torch
        S = torch.cuda.default_stream(self.dev) if kind == "torch-default" else torch.cuda.Stream(self.dev)
        produced = torch.cuda.Event()
        with torch.cuda.stream(S):
            torch.cuda._sleep(1)                          # (a new stream's first launch brings its queue up: milliseconds that are no part of the gap)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S):
                t0 = time.perf_counter()
                torch.cuda._sleep(self.cycles)
                for t, src in self.inputs:
                    t.copy_(src)
                for t, late in self.outputs:
                    t.fill_(late)
                produced.record(S)
                if kind == "torch-current":
                    ctx.use_torch_stream()                # "current" is S here, and only here
            if kind == "side-raw-handle":
                ctx.set_stream(S.cuda_stream)
            elif kind == "torch-default":
                ctx.use_torch_stream(S)
            gap_ms = (time.perf_counter() - t0) * 1e3
            pending = not produced.query()
            result = call()
            waited = produced.query()
            with torch.cuda.stream(S):
                clones = [t.clone() for t, _ in self.outputs]      # a torch op on S behind the call, no synchronise in between
            got = [t.cpu().numpy() for t, _ in self.outputs]
            for c, g in zip(clones, got):
                assert same(c.cpu().numpy(), g), "a torch op on the stream behind the call read other bytes"
        finally:
            torch.cuda.synchronize()
            ctx.set_stream(0)
        GAPS.append(gap_ms)
        print(f"\n[stream order] {kind}: host gap {gap_ms:.3f} ms before the call, delay {DELAY_MS:.0f} ms; largest gap so far {max(GAPS):.3f} ms")
        assert pending, f"delay too short: the producers were done {gap_ms:.3f} ms after their enqueue, before the call was made"
        assert waited, "the call returned while the work enqueued before it on its stream was still pending"
        return got, result


# ---- the filters -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    img = case_image(H, W)
    depth, normal, ids = guides(H, W)
    kw = dict(sigma_depth=SIGMA_DEPTH, sigma_normal=SIGMA_NORMAL, same_object=True)
    return dict(img=img, f32=as_f32_frame(img), depth=depth, normal=normal, ids=ids, kw=kw,
                bilateral=R.bilateral_filter(img, SIZE)[0], guided=R.guided_filter(img, SIZE, depth=depth, normal=normal, ids=ids, **kw)[0])


@pytest.mark.parametrize("fmt", [R.PIXELS_U8, R.PIXELS_F32_RUST2], ids=["u8", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_bilateral_filter(ctx, torch, cycles_per_ms, frames, kind, fmt):
    src = frames["img"] if fmt == R.PIXELS_U8 else frames["f32"]
    assert same(ctx.bilateral_filter(src, SIZE)[0], frames["bilateral"])         # own stream, host frame: the scratch is as large as it gets
    hz = Hazard(torch, cycles_per_ms)
    t_in = hz.input(src)
    t_out = hz.output((H, W, 3), torch.uint8, 0x5A, 0xA5)
    (got,), _ = hz.run(ctx, kind, lambda: ctx.bilateral_filter(t_in.data_ptr(), SIZE, shape=(H, W), in_format=fmt, out=t_out.data_ptr()))
    assert same(got, frames["bilateral"])
    assert not same(frames["bilateral"], R.bilateral_filter(np.zeros_like(frames["img"]), SIZE)[0])      # (the stale frame's answer is another)


@pytest.mark.parametrize("kind", KINDS)
def test_guided_filter(ctx, torch, cycles_per_ms, frames, kind):
    g = {k: frames[k] for k in ("depth", "normal", "ids")}
    assert same(ctx.guided_filter(frames["img"], SIZE, **g, **frames["kw"])[0], frames["guided"])
    hz = Hazard(torch, cycles_per_ms)
    t_img = hz.input(frames["img"])
    t_g = {k: hz.input(v) for k, v in g.items()}
    t_out = hz.output((H, W, 3), torch.uint8, 0x5A, 0xA5)
    (got,), _ = hz.run(ctx, kind, lambda: ctx.guided_filter(t_img.data_ptr(), SIZE, shape=(H, W), in_format=R.PIXELS_U8, out=t_out.data_ptr(),
                                                            **{k: t.data_ptr() for k, t in t_g.items()}, **frames["kw"]))
    assert same(got, frames["guided"])
    # (each stale guide alone gives another answer)
    for k in g:
        assert not same(R.guided_filter(frames["img"], SIZE, **{**g, k: np.zeros_like(g[k])}, **frames["kw"])[0], frames["guided"]), k


# ---- the scene queries -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2():
    """The Book-1 scene (485 spheres: the queries walk the tree), 64 rays from the camera of which some hit, a 32 x 18 depth camera, and the
    answers of a fresh context on its own stream (tests/test_gpu_scene_hits.py holds that form to the oracle)."""
    scene, cam, p = small_view(R.SCENE_C2, 64, 36, 4)
    rng = np.random.default_rng(21)
    origin = np.array(list(cam.origin), F)
    rays = np.concatenate([np.broadcast_to(origin, (64, 3)), rng.normal(0.0, 4.0, (64, 3)).astype(F) - origin], 1).astype(F)
    away = np.tile(np.array([0.0, 2000.0, 0.0, 0.0, 1.0, 0.0], F), (64, 1))       # the stale rays: above everything, pointing up
    dcam = R.camera2_new(32 / 18, tuple(origin), (0.0, 1.0, 0.0), tuple(-origin), 40.0, 0.0)

    def answers(r):
        r.set_scene(scene)
        t, idx, nrm, st = r.scene_hits(rays, MINT, MAXT, normals=True)
        assert st.node_tests > 0
        t0, idx0, _, _ = r.scene_hits(away, MINT, MAXT, normals=True)
        assert np.isinf(t0).all() and (idx0 == -1).all()
        depth, ids, normals, _ = r.depth_map(dcam, 32, 18, MINT, MAXT, ids=True, normals=True)
        return (t, idx, nrm), (depth, ids, normals)
    hits, dmap = fresh(answers)
    assert 0 < int((hits[1] >= 0).sum()) < 64
    return dict(scene=scene, rays=rays, away=away, dcam=dcam, hits=hits, dmap=dmap)


@pytest.mark.parametrize("kind", KINDS)
def test_scene_hits(ctx, torch, cycles_per_ms, c2, kind):
    ctx.set_scene(c2["scene"])
    for a, b in zip(ctx.scene_hits(c2["rays"], MINT, MAXT, normals=True)[:3], c2["hits"]):
        assert same(a, b)
    hz = Hazard(torch, cycles_per_ms)
    d_rays = hz.input(c2["rays"], stale=c2["away"])
    d_t, d_i, d_n = hz.output((64,), torch.float32, -7.5, -9.5), hz.output((64,), torch.int32, -77, -99), hz.output((64, 3), torch.float32, -7.5, -9.5)
    st = R.RtwStats()
    got, rc = hz.run(ctx, kind, lambda: R.lib().rtw_ctx_scene_hits(ctx._h, d_rays.data_ptr(), 64, 0.0, MINT, MAXT, R.ACCEL_BVH, d_t.data_ptr(),
                                                                   d_i.data_ptr(), d_n.data_ptr(), C.byref(st)))
    assert rc == R.RTW_OK and st.node_tests > 0
    for k, (g, w) in enumerate(zip(got, c2["hits"])):
        assert same(g, w), k


@pytest.mark.parametrize("kind", KINDS)
def test_depth_map(ctx, torch, cycles_per_ms, c2, kind):
    ctx.set_scene(c2["scene"])
    for a, b in zip(ctx.depth_map(c2["dcam"], 32, 18, MINT, MAXT, ids=True, normals=True)[:3], c2["dmap"]):
        assert same(a, b)
    hz = Hazard(torch, cycles_per_ms)
    d_d, d_i, d_n = hz.output((18, 32), torch.float32, -7.5, -9.5), hz.output((18, 32), torch.int32, -77, -99), hz.output((18, 32, 3), torch.float32, -7.5, -9.5)
    st = R.RtwStats()
    got, rc = hz.run(ctx, kind, lambda: R.lib().rtw_ctx_depth_map(ctx._h, C.byref(c2["dcam"]), 32, 18, 0.0, MINT, MAXT, R.ACCEL_BVH, d_d.data_ptr(),
                                                                  d_i.data_ptr(), d_n.data_ptr(), C.byref(st)))
    assert rc == R.RTW_OK
    for k, (g, w) in enumerate(zip(got, c2["dmap"])):
        assert same(g, w), k


# ---- the renders -------------------------------------------------------------------------------------------------------------------------
PARTS = {"whole": (8, 0, 1), "part-1-of-3": (8, 1, 3)}     # (row_block, part_index, part_count); 36 rows: part 1 of 3 owns rows 8..15 and 32..35


@pytest.fixture(scope="module")
def c1():
    scene = R.Scene.generate(R.SCENE_C1)
    cam, p = R.default_view(R.SCENE_C1)
    p.width, p.height, p.samples, p.gamma, p.accel = 64, 36, 4, 1.0, R.ACCEL_BVH
    ref, _ = O.render(cam, scene, p)
    return scene, cam, p, ref


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("kind", KINDS)
def test_render(ctx, torch, cycles_per_ms, c1, kind, part):
    scene, cam, p, ref = c1
    q = R.RtwParams.from_buffer_copy(p)
    q.row_block, q.part_index, q.part_count = PARTS[part]
    want = ref if part == "whole" else np.concatenate([ref[8:16], ref[32:36]])
    ctx.set_scene(scene)
    warm = torch.zeros(want.shape, dtype=torch.float32, device="cuda:0")        # own stream, device rows: the allocations of the call below
    torch.cuda.synchronize()
    ctx.render(cam, q, out=warm.data_ptr())
    assert same(warm.cpu().numpy(), want)
    build = ctx.last_render_build()
    hz = Hazard(torch, cycles_per_ms)
    t_out = hz.output(want.shape, torch.float32, -7.5, -9.5)
    (got,), (_, st) = hz.run(ctx, kind, lambda: ctx.render(cam, q, out=t_out.data_ptr()))
    assert st.rows == len(want)
    assert same(got, want)
    assert ctx.last_render_build() == build


@pytest.mark.parametrize("kind", KINDS)
def test_render_multi(ctx, torch, cycles_per_ms, kind):
    """Two frames of a scene with a moving sphere into one device buffer: frame f at time f / fps, each the oracle's frame."""
    moving = R.Sphere.new_moving((0.0, 0.0, -1.5), 0.4, (0.9, 0.4, 0.4), R.SCATTER_M, (0.0, 3.0, 0.0))
    scene = R.Scene([R.Sphere.with_albedo((0, -100.5, -1), 100.0, (0.5, 0.5, 0.5)), moving,
                     R.Sphere.new((1.0, 0.0, -1.5), 0.4, (0.8, 0.8, 0.8), R.METALLIC_M)])
    vp = R.Viewport.new_from_res(64, 36, 8, 6, 1.0)
    vp.fps, vp.shutter_speed = 10.0, 0.05
    p = vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, R.ACCEL_BRUTE)
    want = []
    for f in (1, 2):
        vp.frame = f
        want.append(O.render(vp.camera(), scene, p)[0])
    want = np.stack(want)
    assert not same(want[0], want[1])
    cam = vp.camera()
    ctx.set_scene(scene, 0.1, 0.2 + 0.05)

    def clip(ptr):
        st = (R.RtwStats * 2)()
        return R.lib().rtw_ctx_render_multi(ctx._h, C.byref(cam), C.byref(p), 10.0, 1, 2, C.c_void_p(ptr), st)
    warm = torch.zeros(want.shape, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert clip(warm.data_ptr()) == R.RTW_OK and same(warm.cpu().numpy(), want)
    build = ctx.last_render_build()
    hz = Hazard(torch, cycles_per_ms)
    t_out = hz.output(want.shape, torch.float32, -7.5, -9.5)
    (got,), rc = hz.run(ctx, kind, lambda: clip(t_out.data_ptr()))
    assert rc == R.RTW_OK
    assert same(got, want)
    assert ctx.last_render_build() == build


# ---- the calls that touch no device memory of the caller ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_host_only_calls(ctx, torch, cycles_per_ms, kind):
    """rtw_ctx_triangle_hits, rtw_ctx_mesh_instance_hits and rtw_ctx_perlin_eval read and write host arrays: no hazard to set up.  Each runs
    once on S behind the delay and gives the own stream's bits."""
    vtx, faces = R.mesh_icosphere(0, (0.0, 0.0, 0.0), 1.0)
    mesh = R.Triangle.from_mesh(vtx, faces, mat=R.SCATTER_M, color=(0.3, 0.7, 0.4))
    assert len(mesh) == 20
    placements = [((0.0, 0.0, -4.0), (1.0, 0.0, 0.0, 0.0)), ((2.5, 0.0, -5.0), tuple(R.quat_from_axis(0.7, (0.0, 1.0, 0.0)))),
                  ((-2.5, 0.5, -5.0), tuple(R.quat_from_axis(-1.1, (1.0, 1.0, 0.0))))]
    rng = np.random.default_rng(5)
    rays = np.concatenate([np.zeros((64, 3), F), (rng.normal(0.0, 0.3, (64, 3)) + np.array([0.0, 0.0, -1.0])).astype(F)], 1).astype(F)
    tri_rays = rays.copy()
    tri_rays[:, 2] = 4.0                                                       # (the mesh itself sits at the origin)
    perlin, pts = R.PerlinNoise(2024), rng.uniform(-8.0, 8.0, (64, 3)).astype(F)
    ctx.set_scene(R.Scene([R.Sphere.new((0.0, -60.0, 0.0), 0.5, (0.5, 0.5, 0.5), R.SCATTER_M)]))
    ctx.set_triangles(mesh)
    ctx.set_mesh_instances(placements)
    calls = {"triangle_hits": lambda: ctx.triangle_hits(tri_rays, MINT, MAXT)[:2],
             "mesh_instance_hits": lambda: ctx.mesh_instance_hits(rays, MINT, MAXT)[:4],
             "perlin_eval": lambda: (ctx.perlin_eval(perlin, pts, 3),)}
    own = {name: call() for name, call in calls.items()}
    assert 0 < int((own["triangle_hits"][1] >= 0).sum()) < 64 and 0 < int((own["mesh_instance_hits"][1] >= 0).sum()) < 64
    assert len({int(v) for v in own["mesh_instance_hits"][1] if v >= 0}) == 3           # every placement is hit by some ray
    for name, call in calls.items():
        _, got = Hazard(torch, cycles_per_ms).run(ctx, kind, call)
        assert len(got) == len(own[name])
        for k, (g, w) in enumerate(zip(got, own[name])):
            assert same(g, w), (name, k)


# ---- one context from stream to stream ---------------------------------------------------------------------------------------------------
def test_switching_streams(ctx, torch, c1, frames):
    """Side stream -> own stream (with the synchronise that stream needs) -> torch's default stream -> a side stream again: a filter call and
    a render at each step, into device buffers that torch filled on the stream of the step; every answer the first one."""
    scene, cam, p, ref = c1
    ctx.set_scene(scene)
    dev = torch.device("cuda:0")
    src = torch.from_numpy(frames["img"]).to(dev)
    torch.cuda.synchronize()
    side, default = torch.cuda.Stream(dev), torch.cuda.default_stream(dev)
    steps = [("side", side, lambda: ctx.set_stream(side.cuda_stream)), ("own", default, lambda: ctx.set_stream(0)),
             ("default", default, lambda: ctx.use_torch_stream(default)), ("side again", side, lambda: ctx.set_stream(side.cuda_stream))]
    answers = []
    try:
        for name, S, point in steps:
            with torch.cuda.stream(S):
                t_in = torch.zeros_like(src)
                t_in.copy_(src)
                t_filtered = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev)
                t_frame = torch.full(ref.shape, -9.5, dtype=torch.float32, device=dev)
            if name == "own":
                torch.cuda.synchronize()                  # the own stream orders with nothing of torch's
            point()
            ctx.bilateral_filter(t_in.data_ptr(), SIZE, shape=(H, W), in_format=R.PIXELS_U8, out=t_filtered.data_ptr())
            ctx.render(cam, p, out=t_frame.data_ptr())
            with torch.cuda.stream(S):
                answers.append((name, t_filtered.cpu().numpy(), t_frame.cpu().numpy(), ctx.last_render_build()))
    finally:
        torch.cuda.synchronize()
        ctx.set_stream(0)
    assert same(answers[0][1], frames["bilateral"]) and same(answers[0][2], ref)
    for name, filtered, frame, build in answers[1:]:
        assert same(filtered, answers[0][1]) and same(frame, answers[0][2]) and build == answers[0][3], name
