"""Per-pixel motion on the GPU (rtw_ctx_surface_map_tri, rtw_ctx_scene_surface_tri, rtw_ctx_deform_motion,
rtw_ctx_temporal_accumulate_points; csrc/rtw_query.hip, csrc/rtw_mesh_move.hip, csrc/rtw_temporal.hip) against the host
forms, bit for bit: tri and bary of both surface calls over one triangle, a quad of two, and an 8 x 8 sheet through the tree and through
the list walk, unplaced, placed at the identity and at a turned pose, and behind a sphere, with the six existing outputs keeping their
bytes; the deform pass at 1, 255, 256, 257 and 67 x 35 pixels, unplaced and placed, every buffer in host or device memory, out-of-range tri
and idx and a refused pose; the temporal pass with points on all, alternating and no pixels at 1 x 1, 31 x 7, 33 x 9 and 67 x 35, with and
without rows, carried_normal and out_prev_xy, in host and device memory; both new passes behind a busy producer on the caller's stream; the
chain surface_map -> move_mesh_instances(poses, ouv) -> surface_map(tri, bary) -> deform_motion -> temporal_accumulate against the chain
through the host forms; TemporalDenoiser.step(prev_ouv=) against the chained calls.  The host forms are held to numpy and to float64
geometry by tests/test_deform_motion_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests.deform_motion_common import (DEFORM_SIZES, E2E_H, E2E_PARAMS, E2E_W, MAXT, MESH_ID, MINT, POINT_SHAPES, case_poses, deform_case, e2e_cameras,
                                        e2e_check, e2e_host_guides, e2e_meshes, e2e_poses, host, sheet, synthetic_points, triangles_of)
from tests.temporal_common import F, OFFSET, SENTINEL, TEMPORAL_TEST_DEFAULTS, look_camera, mismatch, orbit, same_bits
from tests.temporal_motion_common import TERMS, class_case, quat_axis, terms_id
from tests.test_deform_motion_cpu import (DEFORM_ACCEPTED, DEFORM_REFUSALS, E_INVALID, POINT_ACCEPTED, POINT_REFUSALS, assert_same_point_runs,
                                          deform_raw_call, points_raw_call, run_points)
from tests.test_gpu_stream_order import KINDS, Hazard, ctx, cycles_per_ms, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu
shape_ids = lambda s: f"{s[1]}x{s[0]}"
H, W = 35, 67
BOOK1 = dict(origin=(13.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), vfov=20.0)
FAR_SPHERE = ((0.0, -2000.0, 0.0), 1.0)                                      # object 0 of every scene here; no ray of these views meets it
FRONT_SPHERE = ((4.0, 0.6, 0.9), 0.7)                                        # between the Book-1 camera and the sheet: it wins some pixels


def on_gpu(torch):
    return lambda a: torch.from_numpy(np.array(a)).to("cuda:0")


def one_triangle():
    return np.array([(0.0, -2.0, -3.0), (0.0, 2.5, 0.5), (0.3, -1.5, 3.0)], F), np.array([[0, 1, 2]])


def quad():
    return np.array([(0.0, -2.0, -3.0), (0.0, 2.0, -3.0), (0.2, 2.0, 3.0), (0.1, -2.0, 3.0)], F), np.array([[0, 1, 2], [0, 2, 3]])


MESHES = {"one-triangle": one_triangle, "quad": quad, "sheet8": lambda: sheet(8, 0.7)}
TURNED = case_poses("placed-and-moved", (0.0, 0.0, 0.0))[1]
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], F)
# (mesh, pose or None, accel, a sphere in front)
SURFACE_CASES = [("one-triangle", None, R.ACCEL_BVH, False), ("quad", None, R.ACCEL_BVH, False), ("sheet8", None, R.ACCEL_BVH, False),
                 ("sheet8", None, R.ACCEL_BRUTE, False), ("sheet8", IDENTITY, R.ACCEL_BVH, False), ("sheet8", TURNED, R.ACCEL_BVH, False),
                 ("sheet8", TURNED, R.ACCEL_BRUTE, False), ("sheet8", None, R.ACCEL_BVH, True), ("sheet8", TURNED, R.ACCEL_BVH, True)]
surface_id = lambda c: f"{c[0]}-{'unplaced' if c[1] is None else 'identity' if c[1] is IDENTITY else 'turned'}-{'tree' if c[2] == R.ACCEL_BVH else 'list'}" \
                       f"{'-sphere' if c[3] else ''}"


def scene_of(r, v, f, pose, sphere):
    spheres = [R.Sphere.new(*FAR_SPHERE, (0.5, 0.5, 0.5), R.SCATTER_M)] + ([R.Sphere.new(*FRONT_SPHERE, (0.5, 0.5, 0.5), R.SCATTER_M)] if sphere else [])
    r.set_scene(R.Scene(spheres, background=(0.7, 0.8, 1.0)))
    r.set_triangles(triangles_of(v, f))
    r.set_mesh_instances(None if pose is None else [(pose[:3], pose[3:])])
    return len(spheres)


# ---- 1. the surface outputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SURFACE_CASES, ids=surface_id)
def test_tri_and_bary_of_the_surface_calls(case):
    name, pose, accel, sphere = case
    v, f = MESHES[name]()
    cam = look_camera(H, W, **BOOK1)
    rays = R.pixel_rays(cam, W, H, OFFSET)
    ouv = R.mesh_ouv(v, f)
    with R.Renderer(0) as r:
        base = scene_of(r, v, f, pose, sphere)
        old = r.surface_map(cam, W, H, MINT, MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, OFFSET, accel=accel)
        new = r.surface_map(cam, W, H, MINT, MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, OFFSET, accel=accel, tri=True, bary=True)
        old_s = r.scene_surface(rays, MINT, MAXT, R.INTEGRATOR_RUST2, accel=accel)
        new_s = r.scene_surface(rays, MINT, MAXT, R.INTEGRATOR_RUST2, accel=accel, tri=True, bary=True)
        only_tri = r.surface_map(cam, W, H, MINT, MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, OFFSET, accel=accel, tri=True)
        only_bary = r.scene_surface(rays, MINT, MAXT, R.INTEGRATOR_RUST2, accel=accel, bary=True)
    for k in ("depth", "idx", "normal", "albedo", "emitted", "material"):             # the six existing outputs keep their bytes
        assert same_bits(new[k], old[k]) and same_bits(only_tri[k], old[k]), k
    for k in ("t", "idx", "normal", "albedo", "emitted", "material"):
        assert same_bits(new_s[k], old_s[k]) and same_bits(only_bary[k], old_s[k]), k
    assert "bary" not in only_tri and "tri" not in only_bary
    assert same_bits(only_tri["tri"], new["tri"]) and same_bits(only_bary["bary"], new_s["bary"])
    # the host forms over the same rays and the device's t
    if pose is None:
        t_host, tri_host = R.triangle_hits(triangles_of(v, f), rays, MINT, MAXT)[:2]
        local = rays
    else:
        t_host, _, tri_host, _ = R.mesh_instance_hits(triangles_of(v, f), [(pose[:3], pose[3:])], rays, MINT, MAXT)
        local = R.mesh_local_rays(pose[None], np.full(len(rays), base, np.int32), rays, base)
    on_mesh = new_s["idx"] >= base
    assert on_mesh.mean() > 0.1 and (not sphere or (new_s["idx"] == 1).sum() > 20)
    want_tri = np.where(on_mesh, tri_host, -1).astype(np.int32)
    assert np.array_equal(new_s["tri"], want_tri) and same_bits(new_s["t"][on_mesh], t_host[on_mesh])
    if pose is None:
        assert np.array_equal(new_s["tri"][on_mesh], new_s["idx"][on_mesh] - base)
    else:
        assert np.all(new_s["idx"][on_mesh] == base)
    if name != "one-triangle":
        assert len(set(new_s["tri"][on_mesh].tolist())) == len(f) or name == "sheet8"      # (the quad: both sides of the shared edge)
    want_bary = R.tri_bary(ouv, local, new_s["t"], new_s["tri"])
    assert same_bits(new_s["bary"], want_bary), mismatch(new_s["bary"], want_bary)
    assert np.all(new_s["bary"][~on_mesh] == 0) and np.any(new_s["bary"][on_mesh] != 0)
    # the map writes what the ray call writes (but for the miss value of depth)
    assert same_bits(new["tri"].ravel(), new_s["tri"]) and same_bits(new["bary"].reshape(-1, 2), new_s["bary"])


def test_surface_outputs_in_device_memory(gpu, torch):
    """tri_out and bary_out, like every other output, written in place into device memory through the C call."""
    v, f = MESHES["sheet8"]()
    cam = look_camera(H, W, **BOOK1)
    with R.Renderer(0) as r:
        scene_of(r, v, f, TURNED, True)
        want = r.surface_map(cam, W, H, MINT, MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, OFFSET, tri=True, bary=True)
        C = R.C
        depth, albedo = np.empty((H, W), F), np.empty((H, W, 3), F)
        tri = torch.full((H, W), 77, dtype=torch.int32, device="cuda:0")
        bary = torch.full((H, W, 2), 77.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rc = R.lib().rtw_ctx_surface_map_tri(r._h, C.byref(cam), W, H, R.RAYS_PIXEL, (C.c_float * 2)(*OFFSET), 0.0, MINT, MAXT, R.ACCEL_BVH,
                                             R.INTEGRATOR_RUST2, depth.ctypes.data, None, None, albedo.ctypes.data, None, None,
                                             C.c_void_p(tri.data_ptr()), C.c_void_p(bary.data_ptr()), None)
        assert rc == 0
    assert same_bits(tri.cpu().numpy(), want["tri"]) and same_bits(bary.cpu().numpy(), want["bary"]) and same_bits(depth, want["depth"])


# ---- 2. the deform pass ------------------------------------------------------------------------------------------------------------------------
DEFORM_BUFFERS = ("tri", "bary", "prev_ouv", "idx", "prev_poses", "point", "normal")
DEFORM_MASKS = [0, 0b1111111, 0b0101010, 0b1010101, 0b0011111, 0b1100000]
mask_id = lambda m: "".join("d" if m >> i & 1 else "h" for i in range(len(DEFORM_BUFFERS)))


@pytest.mark.parametrize("mask", DEFORM_MASKS, ids=mask_id)
@pytest.mark.parametrize("placed", [False, True], ids=["unplaced", "placed"])
@pytest.mark.parametrize("n", DEFORM_SIZES + [H * W])
def test_deform_motion_equals_host(gpu, torch, n, placed, mask):
    """Each of the seven buffers (DEFORM_BUFFERS, in the order of the ids' letters) independently host memory (staged) or device memory (in
    place), through the C call; the cases hold every class of tri and idx and a refused pose."""
    c = deform_case(n, placed)
    want_p, want_n = R.deform_motion(**c)
    buf = dict(c, point=np.full((n, 3), SENTINEL), normal=np.full((n, 3), SENTINEL))
    held = {k: None if buf[k] is None else on_gpu(torch)(buf[k]) if mask >> i & 1 else np.array(buf[k]) for i, k in enumerate(DEFORM_BUFFERS)}
    a = {k: None if v is None else R.C.c_void_p(int(v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data)) for k, v in held.items()}
    torch.cuda.synchronize()
    for _ in range(2):                                                             # (the second call reuses the staging)
        rc = R.lib().rtw_ctx_deform_motion(gpu._h, a["tri"], a["bary"], n, a["prev_ouv"], len(c["prev_ouv"]), a["idx"], a["prev_poses"],
                                           len(c["prev_poses"]) if placed else 0, c["first"], a["point"], a["normal"])
        assert rc == 0
    assert same_bits(host(held["point"]), want_p), mismatch(host(held["point"]), want_p)
    assert same_bits(host(held["normal"]), want_n), mismatch(host(held["normal"]), want_n)


def test_deform_motion_through_python_with_tensors(gpu, torch):
    c = deform_case(H * W, True)
    want_p, want_n = R.deform_motion(**c)
    dev = on_gpu(torch)
    shaped = lambda a, *tail: a.reshape(H, W, *tail)
    p, n = gpu.deform_motion(dev(shaped(c["tri"])), dev(shaped(c["bary"], 2)), dev(c["prev_ouv"]), dev(shaped(c["idx"])), dev(c["prev_poses"]), c["first"])
    assert p.is_cuda and tuple(p.shape) == (H, W, 3)
    assert same_bits(p.cpu().numpy().reshape(-1, 3), want_p) and same_bits(n.cpu().numpy().reshape(-1, 3), want_n)
    p, n = gpu.deform_motion(c["tri"], c["bary"], c["prev_ouv"])                    # numpy, unplaced
    want_p, want_n = R.deform_motion(c["tri"], c["bary"], c["prev_ouv"])
    assert same_bits(p, want_p) and same_bits(n, want_n)


@pytest.mark.parametrize("name,change", DEFORM_REFUSALS, ids=[n for n, _ in DEFORM_REFUSALS])
def test_deform_refusals_on_the_device(gpu, name, change):
    rc, outs = deform_raw_call(R.lib().rtw_ctx_deform_motion, (gpu._h,), **change)
    assert rc == E_INVALID and all(np.all(o == SENTINEL) for o in outs)


@pytest.mark.parametrize("name,change", DEFORM_ACCEPTED, ids=[n for n, _ in DEFORM_ACCEPTED])
def test_deform_calls_next_to_the_refusals_on_the_device(gpu, name, change):
    rc, outs = deform_raw_call(R.lib().rtw_ctx_deform_motion, (gpu._h,), **change)
    want = deform_raw_call(R.lib().rtw_deform_motion, **change)[1]
    assert rc == 0 and all(same_bits(o, x) for o, x in zip(outs, want))


# ---- 3. the temporal pass with points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host-memory", "device-memory"])
@pytest.mark.parametrize("which", ["all", "alternating", "none", "edges"])
@pytest.mark.parametrize("shape", POINT_SHAPES, ids=shape_ids)
def test_points_on_the_device_equal_the_host_form(gpu, torch, shape, which, where):
    h, w = shape
    wrap = on_gpu(torch) if where == "device-memory" else None
    points = synthetic_points(h, w, 0, which)
    for moved_cam in (False, True):
        frames, rows, first = class_case(h, w, "first3", moved_cam)
        for terms in (TERMS[0], TERMS[2], TERMS[7]):
            params = dict(TEMPORAL_TEST_DEFAULTS, **terms)
            for table in (rows, None):
                dev_table = table if table is None or wrap is None else wrap(np.ascontiguousarray(table).view(F).reshape(len(table), 32).copy())
                for carried, prev_xy in ((True, True), (False, True), (True, False)):
                    got = run_points(gpu.temporal_accumulate, frames, params, dev_table, first, points, wrap=wrap, carried=carried, prev_xy=prev_xy)
                    want = run_points(R.temporal_accumulate, frames, params, table, first, points, carried=carried, prev_xy=prev_xy)
                    keys = ("color", "moments", "len", "variance") + (("prev_xy",) if prev_xy else ())
                    assert_same_point_runs(got, want, (moved_cam, terms_id(terms), table is not None, carried, prev_xy), keys)


@pytest.mark.parametrize("name,change", POINT_REFUSALS, ids=[n for n, _ in POINT_REFUSALS])
def test_points_refusals_on_the_device(gpu, name, change):
    rc, out = points_raw_call(R.lib().rtw_ctx_temporal_accumulate_points, (gpu._h,), **change)
    assert rc == E_INVALID and all(np.all(v == SENTINEL) for v in out.values())


@pytest.mark.parametrize("name,change", POINT_ACCEPTED, ids=[n for n, _ in POINT_ACCEPTED])
def test_points_calls_next_to_the_refusals_on_the_device(gpu, name, change):
    rc, out = points_raw_call(R.lib().rtw_ctx_temporal_accumulate_points, (gpu._h,), **change)
    want = points_raw_call(R.lib().rtw_temporal_accumulate_points, **change)[1]
    assert rc == 0 and all(same_bits(out[k], want[k]) for k in out)


# ---- 4. behind a busy stream -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_deform_and_points_behind_a_busy_stream(ctx, torch, cycles_per_ms, kind):  # noqa: F811
    """rtw_ctx_deform_motion into device points, then rtw_ctx_temporal_accumulate_points reading them in place, both behind a pending
    producer of every device buffer on the caller's stream."""
    h, w = H, W
    frames, rows, first = class_case(h, w, "first3", True)
    f0, f1 = frames
    c = deform_case(h * w, True)
    prm = dict(TEMPORAL_TEST_DEFAULTS, **TERMS[7])
    want_p, want_n = R.deform_motion(**c)
    first_out = run_points(R.temporal_accumulate, [f0], prm, rows, first, None)[0]
    hist = dict(color=first_out["color"], moments=first_out["moments"], len=first_out["len"], depth=f0["depth"], normal=f0["normal"], idx=f0["idx"])
    want, _, _ = R.temporal_accumulate(f1["cur"], f1["cam"], depth=f1["depth"], normal=f1["normal"], ids=f1["idx"], history=dict(hist, cam=f0["cam"]),
                                       motion=rows, motion_first=first, out_prev_xy=True, prev_point=want_p.reshape(h, w, 3),
                                       carried_normal=want_n.reshape(h, w, 3), offset=OFFSET, **prm)

    def both(r, t_def, t_pt, t_in, t_hist, t_out):
        rc = R.lib().rtw_ctx_deform_motion(r._h, *(R.C.c_void_p(t_def[k].data_ptr()) for k in ("tri", "bary")), h * w,
                                           R.C.c_void_p(t_def["prev_ouv"].data_ptr()), len(c["prev_ouv"]), R.C.c_void_p(t_def["idx"].data_ptr()),
                                           R.C.c_void_p(t_def["prev_poses"].data_ptr()), len(c["prev_poses"]), c["first"],
                                           R.C.c_void_p(t_pt[0].data_ptr()), R.C.c_void_p(t_pt[1].data_ptr()))
        assert rc == 0
        return r.temporal_accumulate(t_in["cur"], f1["cam"], depth=t_in["depth"], normal=t_in["normal"], ids=t_in["idx"],
                                     history=dict(t_hist, cam=f0["cam"]), motion=rows, motion_first=first, out_prev_xy=t_out["prev_xy"],
                                     out_color=t_out["color"], prev_point=t_pt[0], carried_normal=t_pt[1], offset=OFFSET, **prm)

    dev = on_gpu(torch)
    z = lambda a: torch.zeros_like(dev(a))
    names = ("tri", "bary", "prev_ouv", "idx", "prev_poses")
    warm = both(ctx, {k: dev(c[k]) for k in names}, (torch.empty((h, w, 3), device="cuda:0"), torch.empty((h, w, 3), device="cuda:0")),
                {k: dev(f1[k]) for k in ("cur", "depth", "normal", "idx")}, {k: dev(v) for k, v in hist.items()},
                dict(prev_xy=z(want["prev_xy"]), color=z(want["color"])))[0]            # own stream: nothing is allocated later
    assert same_bits(warm["color"].cpu().numpy(), want["color"])
    hz = Hazard(torch, cycles_per_ms)
    t_def = {k: hz.input(c[k], stale=np.full_like(c[k], -1) if k == "tri" else None) for k in names}
    t_pt = (hz.output((h, w, 3), torch.float32, 3.0, 5.0), hz.output((h, w, 3), torch.float32, 3.0, 5.0))
    t_in = {k: hz.input(f1[k]) for k in ("cur", "depth", "normal", "idx")}
    t_hist = {k: hz.input(v, stale=np.ones_like(v) if k == "len" else None) for k, v in hist.items()}
    t_out = dict(prev_xy=hz.output((h, w, 2), torch.float32, 3.0, 5.0), color=hz.output((h, w, 3), torch.float32, 3.0, 5.0))
    got, (new, var, _) = hz.run(ctx, kind, lambda: both(ctx, t_def, t_pt, t_in, t_hist, t_out))
    assert same_bits(got[0].reshape(-1, 3), want_p) and same_bits(got[1].reshape(-1, 3), want_n)
    assert same_bits(got[2], want["prev_xy"]) and same_bits(got[3], want["color"]), (mismatch(got[2], want["prev_xy"]), mismatch(got[3], want["color"]))
    assert same_bits(new["len"].cpu().numpy(), want["len"]) and same_bits(new["moments"].cpu().numpy(), want["moments"])


# ---- 5. the chain on the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def waving():
    """A context of its own whose scene is one far sphere (object 0) and the sheet of the end-to-end case, placed at its previous pose."""
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    (v0, _), f = e2e_meshes()
    pp, _ = e2e_poses()
    with R.Renderer(0) as r:
        r.set_scene(R.Scene([R.Sphere.new(*FAR_SPHERE, (0.5, 0.5, 0.5), R.SCATTER_M)], background=(0.7, 0.8, 1.0)))
        r.set_triangles(triangles_of(v0, f))
        r.set_mesh_instances([(pp[0, :3], pp[0, 3:])])
        yield r


def _map(r, cam, **kw):
    return r.surface_map(cam, E2E_W, E2E_H, MINT, MAXT, R.INTEGRATOR_RUST2, R.RAYS_PIXEL, OFFSET, **kw)


def test_the_chain_on_the_device_equals_the_chain_of_host_forms(waving, torch):
    cam, prev_cam = e2e_cameras()
    (v0, v1), f = e2e_meshes()
    pp, cp = e2e_poses()
    ouv0, ouv1 = R.mesh_ouv(v0, f), R.mesh_ouv(v1, f)
    first = waving.mesh_instance_first()
    assert first == 1
    waving.move_mesh_instances(pp, ouv0)
    g0 = _map(waving, prev_cam)
    waving.move_mesh_instances(on_gpu(torch)(cp), on_gpu(torch)(ouv1))
    g1 = _map(waving, cam, tri=True, bary=True)
    point, carried = waving.deform_motion(g1["tri"], g1["bary"], ouv0, g1["idx"], pp, first)
    # the host forms' guides are these, but for the ids' base and the miss value of the normal
    h0, h1 = e2e_host_guides()
    for g, hst in ((g0, h0), (g1, h1)):
        hit = hst["idx"] >= 0
        assert np.array_equal(g["idx"][hit], hst["idx"][hit] - MESH_ID + first) and np.all(g["idx"][~hit] == -1)
        assert same_bits(g["depth"][hit], hst["depth"][hit]) and same_bits(g["normal"][hit], hst["normal"][hit])
    assert same_bits(g1["tri"], h1["tri"]) and same_bits(g1["bary"], h1["bary"])
    want_point, want_carried = R.deform_motion(h1["tri"], h1["bary"], ouv0, h1["idx"], pp, MESH_ID)
    assert same_bits(point, want_point) and same_bits(carried, want_carried)
    shift = lambda g, hst: dict(hst, depth=g["depth"], normal=g["normal"], idx=np.where(g["idx"] >= 0, g["idx"] - first + MESH_ID, -1).astype(np.int32))
    got, counts = e2e_check(waving.temporal_accumulate, shift(g0, h0), shift(g1, h1), point, carried, "device, surface_map")
    want, counts_host = e2e_check(R.temporal_accumulate, shift(g0, h0), shift(g1, h1), want_point, want_carried, "host forms")
    assert counts == counts_host
    for k in got:
        assert same_bits(got[k], want[k]), (k, mismatch(got[k], want[k]))


DEN = dict(alpha=0.2, alpha_moments=0.2, max_history=32, depth_tol=0.05, normal_cos=0.9, same_object=1)


@pytest.mark.parametrize("which", ["temporal", "svgf"])
def test_denoisers_with_prev_ouv_equal_the_chained_calls(waving, which):
    """Three steps, the sheet waved and moved before each, through TemporalDenoiser / SvgfDenoiser with prev_ouv= and prev_poses= against
    the hand-chained calls on the rendered inputs the step reports."""
    eye = np.array(BOOK1["origin"])
    vp = R.Viewport.new_from_res(E2E_W, E2E_H, 4, 4, 1.0, vfov=20.0, origin=tuple(eye), direction=tuple(-eye / np.linalg.norm(eye)), vup=(0.0, 1.0, 0.0))
    cam = vp.camera()
    assert vp.height == E2E_H
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = E2E_W, E2E_H, 4, 4, 1.0
    p.mint, p.maxt = MINT, MAXT
    p.integrator, p.sampler, p.accel, p.flags, p.seed = R.INTEGRATOR_RUST2, R.SAMPLER_ROW, R.ACCEL_BVH, 0, 40
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    (v0, v1), f = e2e_meshes()
    pp, cp = e2e_poses()
    ouvs, poses = [R.mesh_ouv(v, f) for v in (v0, v1, v0)], [pp, cp, pp]
    first = waving.mesh_instance_first()
    den = (R.TemporalDenoiser if which == "temporal" else R.SvgfDenoiser)(waving, **DEN)
    hist_host, covers = None, []
    for k in range(3):
        waving.move_mesh_instances(poses[k], ouvs[k])
        kw = {} if k == 0 else dict(prev_ouv=ouvs[k - 1], prev_poses=poses[k - 1])
        c = orbit(cam, 0.5 * k)
        frame, acc, var, st = den.step(c, p, **kw)
        g = st["guides"]
        assert ("tri" in g) == (k > 0)
        points = {}
        if k:
            pt, cn = waving.deform_motion(g["tri"], g["bary"], ouvs[k - 1], g["idx"], poses[k - 1], first)
            assert same_bits(pt, R.deform_motion(g["tri"], g["bary"], ouvs[k - 1], g["idx"], poses[k - 1], first)[0])
            points = dict(prev_point=pt, carried_normal=cn)
        hist_host, var_host, _ = R.temporal_accumulate(st["cur"], c, depth=g["depth"], normal=g["normal"], ids=g["idx"], history=hist_host,
                                                       offset=OFFSET, **points, **DEN)
        for key in ("color", "moments", "len"):
            assert same_bits(den.history[key], hist_host[key]), (k, key, mismatch(den.history[key], hist_host[key]))
        if which == "temporal":
            assert same_bits(var, var_host)
        covers.append(float((den.history["len"] > 1)[g["idx"] == first].mean()))
    print(f"\n[deform, denoiser {which}] coverage of the sheet per step {covers}")
    assert covers[0] == 0.0 and covers[1] > 0.8 and covers[2] > 0.8                    # (the silhouette loses its history, rightly)
