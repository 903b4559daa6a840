"""Temporal accumulation with moving objects on the GPU (rtw_ctx_temporal_accumulate_motion, rtw_ctx_mesh_instance_motion; csrc/rtw_temporal.hip,
csrc/rtw_mesh_move.hip) against the host forms, bit for bit: the CPU tests' cases (every id class about the table, every term
combination, static and moved cameras) at 1 x 1, 31 x 7, 33 x 9 and 67 x 35 with the rows and out_prev_xy in host and in device memory,
65535 x 1 and 1 x 65535, every buffer's memory kind mixed through the C call, the refusals, the float64 geometry, the motion rows of 1 to
65 536 placements with each buffer in host or device memory and tensors in place, both calls behind a busy producer on the caller's
stream, two placements of an icosphere with the guides from surface_map between two move_mesh_instances calls, and the two denoisers with
motion against the hand-chained calls.  The host forms are held to numpy and to float64 geometry by tests/test_temporal_motion_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.temporal_common import (BUFFERS, CASE_NAMES, F, OFFSET, SENTINEL, TEMPORAL_TEST_DEFAULTS, assert_same_runs, cases, host_answer, mismatch, orbit,
                                   run, same_bits)
from tests.temporal_motion_common import (E2E_FIRST, E2E_H, E2E_MAXT, E2E_MINT, E2E_PARAMS, E2E_W, GEO_MOTION_CASES, MOTION_KEYS, MOTION_SHAPES, TABLES,
                                          TERMS, check_motion_geometry, class_answer, class_case, e2e_cameras, e2e_check, e2e_guides_host, e2e_mesh,
                                          e2e_poses, geo_motion_case, motion_probe, run_motion, terms_id)
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)
from tests.test_temporal_motion_cpu import MOTION_ACCEPTED, MOTION_REFUSALS, _poses, motion_raw_call

pytestmark = pytest.mark.gpu
shape_ids = lambda s: f"{s[1]}x{s[0]}"
LIMIT = 65535                                              # RTW_TEMPORAL_MAX_SIDE


def on_gpu(torch):
    return lambda a: torch.from_numpy(np.array(a)).to("cuda:0")


def rows_tensor(torch, rows):
    """A table of MOTION_ROW records as the float32 tensor [n][32] the device reads in place."""
    return torch.from_numpy(np.ascontiguousarray(rows).view(F).reshape(len(rows), 32).copy()).to("cuda:0")


def assert_same_motion_runs(got, want, what):
    assert len(got) == len(want)
    for k, (g, x) in enumerate(zip(got, want)):
        for key in MOTION_KEYS:
            assert same_bits(g[key], x[key]), (what, f"frame {k}", key, mismatch(g[key], x[key]))


# ---- 8. device against the host form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host-memory", "device-memory"])
@pytest.mark.parametrize("shape", MOTION_SHAPES, ids=shape_ids)
def test_device_equals_host(gpu, torch, shape, where):
    """host-memory: every buffer, the rows and out_prev_xy numpy arrays (staged); device-memory: all of them tensors, read and written in
    place."""
    h, w = shape
    wrap = on_gpu(torch) if where == "device-memory" else None
    for table in TABLES:
        for moved_cam in (False, True):
            frames, rows, first = class_case(h, w, table, moved_cam)
            table_arg = rows_tensor(torch, rows) if wrap else rows
            for tk, terms in enumerate(TERMS):
                got = run_motion(gpu.temporal_accumulate, frames, dict(TEMPORAL_TEST_DEFAULTS, **terms), table_arg, first, wrap=wrap)
                assert_same_motion_runs(got, class_answer(h, w, table, moved_cam, tk), (table, moved_cam, terms_id(terms)))


@pytest.mark.parametrize("moved_cam", [False, True], ids=["static-camera", "moved-camera"])
def test_nan_row_and_out_color_is_cur_on_the_device(gpu, torch, moved_cam):
    h, w = 35, 67
    frames, rows, first = class_case(h, w, "first3", moved_cam, True)
    params = dict(TEMPORAL_TEST_DEFAULTS, **TERMS[7])
    want = class_answer(h, w, "first3", moved_cam, 7, True)
    assert_same_motion_runs(run_motion(gpu.temporal_accumulate, frames, params, rows, first, out_color_is_cur=True), want, "host memory")
    assert_same_motion_runs(run_motion(gpu.temporal_accumulate, frames, params, rows_tensor(torch, rows), first, wrap=on_gpu(torch),
                                       out_color_is_cur=True), want, "device memory")


def test_without_rows_the_bytes_of_the_existing_call(gpu):
    """The new entry point with a table that does not move, or out_prev_xy alone, on the existing cases: the existing call's bytes."""
    h, w = 17, 33
    for name in CASE_NAMES:
        frames, params = cases(h, w)[name]
        top = int(max(fr["idx"].max() for fr in frames)) + 1
        assert_same_runs(run(lambda *a, **k: gpu.temporal_accumulate(*a, motion=R.motion_rows(top), **k), frames, params), host_answer(h, w, name), name)
        assert_same_runs(run(lambda *a, **k: gpu.temporal_accumulate(*a, out_prev_xy=True, **k), frames, params), host_answer(h, w, name), name)


@pytest.mark.parametrize("shape", [(1, LIMIT), (LIMIT, 1)], ids=shape_ids)
def test_frames_at_the_declared_limit(gpu, shape):
    h, w = shape
    frames, rows, first = class_case(h, w, "first3", True)
    params = dict(TEMPORAL_TEST_DEFAULTS, **TERMS[6])
    want = run_motion(R.temporal_accumulate, frames, params, rows, first)
    assert 0.0 < float((want[1]["len"] > 1).mean()) < 1.0
    assert_same_motion_runs(run_motion(gpu.temporal_accumulate, frames, params, rows, first), want, shape)


MOTION_BUFFERS = BUFFERS + ("rows", "out_prev_xy")                                 # the 16 buffers of a call with motion
N_IN = 10
ALL = (1 << len(MOTION_BUFFERS)) - 1
MASKS = [0, ALL, 0b0101010101010101, 0b1010101010101010, 1 << 14, 1 << 15, ALL & ~(1 << 14), ALL & ~(1 << 15)]
mask_id = lambda m: "".join("d" if m >> i & 1 else "h" for i in range(len(MOTION_BUFFERS)))


@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
def test_host_and_device_memory_mixed(gpu, torch, mask):
    """Each of the 16 buffers (MOTION_BUFFERS, in the order of the ids' letters) independently host memory (staged) or device memory (in
    place), through the C call."""
    h, w = 35, 67
    frames, rows, first = class_case(h, w, "first3", True)
    f0, f1 = frames
    want0, want = class_answer(h, w, "first3", True, 7)
    prm = dict(TEMPORAL_TEST_DEFAULTS, **TERMS[7])
    buf = dict(cur=f1["cur"], depth=f1["depth"], normal=f1["normal"], idx=f1["idx"], prev_color=want0["color"], prev_moments=want0["moments"],
               prev_len=want0["len"], prev_depth=f0["depth"], prev_normal=f0["normal"], prev_idx=f0["idx"],
               out_color=np.full((h, w, 3), SENTINEL), out_moments=np.full((h, w, 2), SENTINEL), out_len=np.full((h, w), SENTINEL),
               out_variance=np.full((h, w), SENTINEL), rows=rows.view(F).reshape(len(rows), 32), out_prev_xy=np.full((h, w, 2), SENTINEL))
    held = {k: on_gpu(torch)(buf[k]) if mask >> i & 1 else np.array(buf[k]) for i, k in enumerate(MOTION_BUFFERS)}
    a = [R.C.c_void_p(int(held[k].data_ptr() if hasattr(held[k], "data_ptr") else held[k].ctypes.data)) for k in MOTION_BUFFERS]
    C = R.C
    p = R.RtwTemporal(prm["alpha"], prm["alpha_moments"], prm["max_history"], prm["depth_tol"], prm["normal_cos"], prm["same_object"], (C.c_float * 2)(*OFFSET))
    st = R.RtwFilterStats()
    torch.cuda.synchronize()
    rc = R.lib().rtw_ctx_temporal_accumulate_motion(gpu._h, a[0], w, h, C.byref(f1["cam"]), a[1], a[2], a[3], C.byref(f0["cam"]), *a[4:10], C.byref(p),
                                                    a[14], len(rows), first, *a[10:14], a[15], C.byref(st))
    assert rc == 0 and st.taps == 4 * h * w and st.filter_ms > 0.0
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v
    for name, key in (("out_color", "color"), ("out_moments", "moments"), ("out_len", "len"), ("out_variance", "variance"), ("out_prev_xy", "prev_xy")):
        assert same_bits(host(held[name]), want[key]), (name, mismatch(host(held[name]), want[key]))
    for name in MOTION_BUFFERS[:N_IN] + ("rows",):                                  # (the inputs are only read)
        assert same_bits(host(held[name]), buf[name]), name


def test_refusals_leave_the_outputs_unwritten(gpu):
    call = R.lib().rtw_ctx_temporal_accumulate_motion
    for name, change in MOTION_REFUSALS:
        rc, out = motion_raw_call(call, (gpu._h,), **change)
        assert rc == -1, name
        assert all(np.all(v == SENTINEL) for v in out.values()), name
    rc, out = motion_raw_call(call, (None,))
    assert rc == -1 and all(np.all(v == SENTINEL) for v in out.values())
    for name, change in MOTION_ACCEPTED:
        rc, out = motion_raw_call(call, (gpu._h,), **change)
        want = motion_raw_call(R.lib().rtw_temporal_accumulate_motion, **change)[1]
        assert rc == 0 and all(same_bits(out[k], want[k]) for k in out), name


def test_reprojection_against_float64_geometry(gpu):
    """The kernel's carried point, fx, fy and turned normal against the float64 reference on every case of the CPU test, and its bytes
    against the host form's."""
    for case in GEO_MOTION_CASES:
        c = geo_motion_case(*case)
        check_motion_geometry(gpu.temporal_accumulate, c, f"device {case}")
        for got, want in zip(motion_probe(gpu.temporal_accumulate, c), motion_probe(R.temporal_accumulate, c)):
            assert same_bits(got, want), (case, mismatch(got, want))


def test_two_placements_end_to_end_as_arrays(gpu):
    """The end-to-end case of the CPU test, its guides from the host form, fed as arrays: the same conditions, the host form's bytes."""
    cam, prev_cam = e2e_cameras()
    prev_poses, cur_poses = e2e_poses()
    g0, g1 = e2e_guides_host(prev_cam, prev_poses), e2e_guides_host(cam, cur_poses)
    rows = R.mesh_instance_motion(prev_poses, cur_poses)[0]
    got, want = e2e_check(gpu.temporal_accumulate, g0, g1, rows, "device"), e2e_check(R.temporal_accumulate, g0, g1, rows, "host")
    for k in got:
        assert same_bits(got[k], want[k]), (k, mismatch(got[k], want[k]))


# ---- 9. rtw_ctx_mesh_instance_motion -----------------------------------------------------------------------------------------------------------
def _motion_poses(n):
    prev, cur = _poses(n, 11), _poses(n, 12)
    cur[::3] = prev[::3]                                                        # a third stands still
    if n > 40:
        cur[7, 1], prev[20, 5], cur[31, 3:] = np.nan, np.inf, 0.0
    return prev, cur


def same_rows(got, want):
    got = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 32)
    want = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 32)
    return got.shape == want.shape and np.array_equal(got, want)                 # (rtw_mesh_instance_motion writes one NaN: the bytes themselves agree)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536])
def test_motion_rows_equal_the_host_form(gpu, torch, n):
    """n about the kernel's workgroup of 256 and at RTW_MAX_MESH_INSTANCES; lists / arrays staged, tensors in place."""
    prev, cur = _motion_poses(n)
    want, want_bad = R.mesh_instance_motion(prev, cur)
    rows, bad = gpu.mesh_instance_motion(prev, cur)
    assert rows.dtype == R.MOTION_ROW and bad == want_bad and same_rows(rows, want)
    t_rows, bad = gpu.mesh_instance_motion(on_gpu(torch)(prev), on_gpu(torch)(cur))
    assert t_rows.is_cuda and tuple(t_rows.shape) == (n, 32) and bad == want_bad and same_rows(t_rows.cpu().numpy(), want)
    if n == 257:
        pairs = lambda p: [(q[:3], q[3:]) for q in p]
        assert same_rows(gpu.mesh_instance_motion(pairs(prev), on_gpu(torch)(cur))[0].cpu().numpy(), want)


@pytest.mark.parametrize("mask", range(8), ids=lambda m: "".join("d" if m >> i & 1 else "h" for i in range(3)))
def test_motion_rows_memory_kinds(gpu, torch, mask):
    """prev_poses, cur_poses, rows_out (in the order of the id's letters) each in host or device memory, through the C call."""
    n = 257
    prev, cur = _motion_poses(n)
    want, want_bad = R.mesh_instance_motion(prev, cur)
    out = np.full((n, 32), SENTINEL)
    held = [on_gpu(torch)(a) if mask >> i & 1 else a for i, a in enumerate((prev, cur, out))]
    ptr = [R.C.c_void_p(int(v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data)) for v in held]
    bad = R.C.c_uint32(99)
    torch.cuda.synchronize()
    assert R.lib().rtw_ctx_mesh_instance_motion(gpu._h, ptr[0], ptr[1], n, ptr[2], R.C.byref(bad)) == 0
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v
    assert bad.value == want_bad and same_rows(host(held[2]), want)
    assert same_bits(host(held[0]), prev) and same_bits(host(held[1]), cur)


def test_motion_rows_refusals(gpu):
    L, C = R.lib(), R.C
    p = np.zeros((2, 7), F)
    p[:, 3] = 1.0
    out = np.full((2, 32), SENTINEL)
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    for args in ((None, p, 2, out), (p, None, 2, out), (p, p, 2, None), (p, p, 0, out), (p, p, 65537, out)):
        assert L.rtw_ctx_mesh_instance_motion(gpu._h, a(args[0]), a(args[1]), args[2], a(args[3]), None) == -1
        assert np.all(out == SENTINEL)
    assert L.rtw_ctx_mesh_instance_motion(None, a(p), a(p), 2, a(out), None) == -1 and np.all(out == SENTINEL)
    assert L.rtw_ctx_mesh_instance_motion(gpu._h, a(p), a(p), 2, a(out), None) == 0 and same_rows(out, R.motion_rows(2))


@pytest.mark.parametrize("kind", KINDS)
def test_both_calls_behind_the_stream(ctx, torch, cycles_per_ms, kind):
    """rtw_ctx_mesh_instance_motion, then temporal_accumulate(motion=) on its rows, every buffer a tensor whose producer is still pending on
    the caller's stream when the calls are made (tests/test_gpu_stream_order.py): the poses hold zeros until then -- invalid poses, whose
    rows are NaN --, the frame's inputs zeros and a history of length 1, and every output is filled behind the delay."""
    h, w = 35, 67
    frames, _, first = class_case(h, w, "first3", True)
    f0, f1 = frames
    n = 5
    prev, cur = _poses(n, 21), _poses(n, 22)
    prev[:, :3], cur[:, :3] = (0.0, 0.0, -3.5), (0.02, 0.01, -3.5)
    cur[:, 3:] = prev[:, 3:] + F(0.01)
    rows = R.mesh_instance_motion(prev, cur)[0]
    prm = dict(TEMPORAL_TEST_DEFAULTS, **TERMS[7])
    first_out = run_motion(R.temporal_accumulate, [f0], prm, rows, first)[0]
    hist = dict(color=first_out["color"], moments=first_out["moments"], len=first_out["len"], depth=f0["depth"], normal=f0["normal"], idx=f0["idx"])
    want, _, _ = R.temporal_accumulate(f1["cur"], f1["cam"], depth=f1["depth"], normal=f1["normal"], ids=f1["idx"], history=dict(hist, cam=f0["cam"]),
                                       motion=rows, motion_first=first, out_prev_xy=True, offset=OFFSET, **prm)

    def both(r, t_prev, t_cur, t_rows, t_in, t_hist, t_out):
        bad = R.C.c_uint32()
        rc = R.lib().rtw_ctx_mesh_instance_motion(r._h, R.C.c_void_p(t_prev.data_ptr()), R.C.c_void_p(t_cur.data_ptr()), n,
                                                  R.C.c_void_p(t_rows.data_ptr()), R.C.byref(bad))
        assert rc == 0
        return r.temporal_accumulate(t_in["cur"], f1["cam"], depth=t_in["depth"], normal=t_in["normal"], ids=t_in["idx"],
                                     history=dict(t_hist, cam=f0["cam"]), motion=t_rows, motion_first=first, out_prev_xy=t_out["prev_xy"],
                                     out_color=t_out["color"], offset=OFFSET, **prm)

    dev = on_gpu(torch)
    z = lambda a: torch.zeros_like(dev(a))
    warm = both(ctx, dev(prev), dev(cur), torch.empty((n, 32), device="cuda:0"), {k: dev(f1[k]) for k in ("cur", "depth", "normal", "idx")},
                {k: dev(v) for k, v in hist.items()}, dict(prev_xy=z(want["prev_xy"]), color=z(want["color"])))[0]     # own stream: nothing is allocated later
    assert same_bits(warm["color"].cpu().numpy(), want["color"])
    hz = Hazard(torch, cycles_per_ms)
    t_prev, t_cur = hz.input(prev), hz.input(cur)
    t_rows = hz.output((n, 32), torch.float32, 3.0, 5.0)
    t_in = {k: hz.input(f1[k]) for k in ("cur", "depth", "normal", "idx")}
    t_hist = {k: hz.input(v, stale=np.ones_like(v) if k == "len" else None) for k, v in hist.items()}
    t_out = dict(prev_xy=hz.output((h, w, 2), torch.float32, 3.0, 5.0), color=hz.output((h, w, 3), torch.float32, 3.0, 5.0))
    got, (new, var, _) = hz.run(ctx, kind, lambda: both(ctx, t_prev, t_cur, t_rows, t_in, t_hist, t_out))
    assert same_rows(got[0], rows)
    assert same_bits(got[1], want["prev_xy"]) and same_bits(got[2], want["color"]), (mismatch(got[1], want["prev_xy"]), mismatch(got[2], want["color"]))
    assert same_bits(new["len"].cpu().numpy(), want["len"]) and same_bits(new["moments"].cpu().numpy(), want["moments"])


# ---- 10. the guides from surface_map, between two moves ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def placed():
    """A context of its own whose scene is one far sphere (object 0) and the two placements of the icosphere at their previous poses."""
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    prev_poses, _ = e2e_poses()
    with R.Renderer(0) as r:
        r.set_scene(R.Scene([R.Sphere.new((0.0, -2000.0, 0.0), 1.0, (0.5, 0.5, 0.5), R.SCATTER_M)], background=(0.7, 0.8, 1.0)))
        r.set_triangles(e2e_mesh())
        r.set_mesh_instances([(p[:3], p[3:]) for p in prev_poses])
        yield r


def _surface_guides(r, cam):
    g = r.surface_map(cam, E2E_W, E2E_H, E2E_MINT, E2E_MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, OFFSET)
    return g["depth"], g["normal"], g["idx"]


def test_two_placements_with_the_guides_of_surface_map(placed, torch):
    cam, prev_cam = e2e_cameras()
    prev_poses, cur_poses = e2e_poses()
    first = placed.mesh_instance_first()
    assert first == 1
    placed.move_mesh_instances(prev_poses)
    g0 = _surface_guides(placed, prev_cam)
    placed.move_mesh_instances(cur_poses)
    g1 = _surface_guides(placed, cam)
    rows, bad = placed.mesh_instance_motion(on_gpu(torch)(prev_poses), on_gpu(torch)(cur_poses))
    assert bad == 0
    # the host form's guides are these, but for the ids' base: placement k is object first + k here, E2E_FIRST + k there
    h0, h1 = e2e_guides_host(prev_cam, prev_poses), e2e_guides_host(cam, cur_poses)
    for g, hst in ((g0, h0), (g1, h1)):
        hit = hst[2] >= 0
        assert np.array_equal(g[2][hit], hst[2][hit] - E2E_FIRST + first) and np.all(g[2][~hit] == -1)
    shift = lambda g: (g[0], g[1], np.where(g[2] >= 0, g[2] - first + E2E_FIRST, -1).astype(np.int32))
    got = e2e_check(placed.temporal_accumulate, shift(g0), shift(g1), rows, "device, surface_map")
    want = e2e_check(R.temporal_accumulate, shift(g0), shift(g1), rows.cpu().numpy().view(R.MOTION_ROW).reshape(-1), "host, surface_map")
    for k in got:
        assert same_bits(got[k], want[k]), (k, mismatch(got[k], want[k]))
    # ... and with the ids as surface_map wrote them and motion_first = mesh_instance_first(): the same history
    hist = dict(color=np.zeros((E2E_H, E2E_W, 3), F), moments=np.zeros((E2E_H, E2E_W, 2), F), len=np.ones((E2E_H, E2E_W), F), depth=g0[0],
                normal=g0[1], idx=g0[2], cam=prev_cam)
    cur = np.ones((E2E_H, E2E_W, 3), F)
    a = placed.temporal_accumulate(cur, cam, depth=g1[0], normal=g1[1], ids=g1[2], history=hist, motion=rows, motion_first=first, out_prev_xy=True,
                                   offset=OFFSET, **E2E_PARAMS)[0]
    assert same_bits(a["prev_xy"], got["prev_xy"]) and same_bits(a["len"], got["len"])


# ---- 11. the denoisers -----------------------------------------------------------------------------------------------------------------------
DEN = dict(alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1)


def _step_poses(k):
    prev, cur = e2e_poses()
    return prev if k == 0 else cur if k == 1 else prev


@pytest.mark.parametrize("which", ["temporal", "svgf"])
def test_denoisers_with_motion_equal_the_chained_calls(placed, which):
    """Three steps, the placements moved before each, through TemporalDenoiser / SvgfDenoiser with motion= against the hand-chained host
    calls on the rendered inputs the step reports; a second context, stepped in between, shares no state."""
    eye = np.array([9.0, 3.0, 7.3])
    vp = R.Viewport.new_from_res(E2E_W, E2E_H, 4, 4, 1.0, vfov=24.0, origin=tuple(eye), direction=tuple(-eye / np.linalg.norm(eye)), vup=(0.0, 1.0, 0.0))
    cam = vp.camera()
    assert vp.height == E2E_H
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = E2E_W, E2E_H, 4, 4, 1.0
    p.mint, p.maxt = E2E_MINT, E2E_MAXT
    p.integrator, p.sampler, p.accel, p.flags, p.seed = R.INTEGRATOR_RUST2, R.SAMPLER_ROW, R.ACCEL_BVH, 0, 40
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    first = placed.mesh_instance_first()
    den = (R.TemporalDenoiser if which == "temporal" else R.SvgfDenoiser)(placed, **DEN)
    with R.Renderer(0) as other:
        other.set_scene(R.Scene([R.Sphere.new((0.0, 0.0, 0.0), 1.0, (0.5, 0.5, 0.5), R.SCATTER_M)], background=(0.7, 0.8, 1.0)))
        den2 = R.TemporalDenoiser(other, **DEN)
        hist_host, covers = None, []
        for k in range(3):
            placed.move_mesh_instances(_step_poses(k))
            rows = None if k == 0 else placed.mesh_instance_motion(_step_poses(k - 1), _step_poses(k))[0]
            frame, acc, var, st = den.step(orbit(cam, 0.5 * k), p, motion=rows, motion_first=first)
            den2.step(cam, vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW))
            g = st["guides"]
            hist_host, var_host, _ = R.temporal_accumulate(st["cur"], orbit(cam, 0.5 * k), depth=g["depth"], normal=g["normal"], ids=g["idx"],
                                                           history=hist_host, motion=rows, motion_first=first, offset=OFFSET, **DEN)
            for key in ("color", "moments", "len"):
                assert same_bits(den.history[key], hist_host[key]), (k, key, mismatch(den.history[key], hist_host[key]))
            if which == "temporal":
                assert same_bits(var, var_host)
                want = placed.atrous_filter(acc, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"])[0]
            else:
                v = placed.variance_estimate(den.history["moments"], den.history["len"], depth=g["depth"], normal=g["normal"], ids=g["idx"])[0]
                assert same_bits(var, v)
                want = placed.svgf_filter(acc, v, depth=g["depth"], normal=g["normal"], ids=g["idx"], albedo=g["albedo"], emitted=g["emitted"])[0]
            assert same_bits(frame, want)
            moved = g["idx"] == first
            covers.append(float((den.history["len"] > 1)[moved].mean()))
        assert den2.history is not None and den2.history["color"].shape == (E2E_H, E2E_W, 3) and np.all(den2.history["idx"] <= 0)
    print(f"\n[motion, denoiser {which}] coverage of the moved placement per step {covers}")
    assert covers[0] == 0.0 and covers[1] > 0.5 and covers[2] > 0.5
