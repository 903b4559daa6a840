"""What the shim's staging decides for a call's caller pointers, pinned in one place: for rtw_ctx_scene_hits, rtw_ctx_depth_map,
rtw_ctx_scene_occluded, rtw_ctx_ambient_occlusion and rtw_ctx_ao_map every caller pointer is, independently of the others, a numpy array or a
torch tensor on the context's device, and every optional output is absent as well.  Whatever the combination:

  * every output holds the bits of the all-host call, and segments, sphere_tests, node_tests and quad_tests are that call's -- the all-host
    answers come from ANOTHER context, computed once (tests/test_gpu_scene_hits.py, test_gpu_occluded.py and test_gpu_ao.py hold that form to
    the oracle);
  * every output buffer, host or device, is TAIL elements longer than the call may write and filled with a sentinel: the tail is untouched;
  * a device input holds after the call what it held before.

After each entry point's matrix one all-host call of a different entry point on the same context still gives its answer: no temporary and no
counter of a pass reaches the next.  rtw_ctx_triangle_hits, rtw_ctx_mesh_instance_hits and rtw_ctx_perlin_eval take host arrays only; their
answers are the host forms' (rtw_triangle_hits, rtw_mesh_instance_hits, rtw_perlin_eval).

The scene is occluded_common's "field": spheres, quads, instances and triangles, 63 top-level spheres -- more than RTW_OPT_LIST_WALK_MAX (48),
so RTW_ACCEL_BVH walks the sphere tree with its LDS stack.  257 rays or points are one 256-thread workgroup and one lane of a second; the
camera forms render 19 x 14 = 266 pixels; AO runs with 4 samples (the single-round build) and 128 (the looped one)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import rtw_amd as R
from tests import ao_common as AO
from tests import mesh_inst_common as MI
from tests import occluded_common as OC
from tests.test_gpu_occluded import install_placements
from tests.test_gpu_scene_hits import depth_camera

pytestmark = pytest.mark.gpu

F, I32, U8 = np.float32, np.int32, np.uint8
N, W, H = 257, 19, 14
TAIL = 64
SENTINEL = {F: -7.5, I32: -77, U8: 0x5A}                  # no answer holds one: t >= mint or +inf, ids >= -1, ao in 0 .. 1, bits 0 or 1
SAMPLES = (4, 128)
STATS = ("segments", "sphere_tests", "node_tests", "quad_tests")
FOLLOWED_BY = {"scene_hits": "ambient_occlusion 4", "depth_map": "scene_occluded", "scene_occluded": "ao_map 128",
               "ambient_occlusion 4": "depth_map", "ambient_occlusion 128": "scene_hits", "ao_map 4": "scene_occluded", "ao_map 128": "scene_hits"}


class Entry:
    """One entry point: its input arrays, its outputs as (elements, dtype, optional), and call(handle, input pointers, output pointers, stats)."""

    def __init__(self, ins, outs, call):
        self.ins, self.outs, self.call = ins, outs, call

    def kinds(self):
        """Every combination of where the caller pointers lie."""
        return itertools.product(*([("host", "device")] * len(self.ins)),
                                 *[("host", "device") + (("absent",) if optional else ()) for _, _, optional in self.outs])

    def all_host(self, kinds):
        """The all-host call with the same outputs asked for."""
        return tuple("absent" if k == "absent" else "host" for k in kinds)


def entries():
    scene, _, rays, time, mint, maxt = OC.scene_case("field")
    rays = np.ascontiguousarray(rays[:N])
    cam = depth_camera("geom", W, H)                        # ("field" is "geom" and 60 spheres among its objects)
    points, normals = AO.random_points(N, 11)
    normals[5] = 0.0                                        # a point that casts no ray: `segments` comes from the kernel's count
    radius, L, bvh = AO.RADIUS["field"], R.lib(), R.ACCEL_BVH
    e = {"scene_hits": Entry((rays,), ((N, F, False), (N, I32, False), (3 * N, F, True)),
                             lambda h, i, o, st: L.rtw_ctx_scene_hits(h, i[0], N, time, mint, maxt, bvh, o[0], o[1], o[2], st)),
         "depth_map": Entry((), ((W * H, F, False), (W * H, I32, True), (3 * W * H, F, True)),
                            lambda h, i, o, st: L.rtw_ctx_depth_map(h, C.byref(cam), W, H, time, mint, maxt, bvh, o[0], o[1], o[2], st)),
         "scene_occluded": Entry((rays,), ((N, U8, False),),
                                 lambda h, i, o, st: L.rtw_ctx_scene_occluded(h, i[0], N, time, mint, maxt, bvh, o[0], st))}
    for s in SAMPLES:
        e[f"ambient_occlusion {s}"] = Entry((points, normals), ((N, F, False),), lambda h, i, o, st, s=s: L.rtw_ctx_ambient_occlusion(
            h, i[0], i[1], N, s, 7, time, AO.AO_MINT, radius, bvh, o[0], st))
        e[f"ao_map {s}"] = Entry((), ((W * H, F, False), (W * H, F, True), (W * H, I32, True), (3 * W * H, F, True)), lambda h, i, o, st, s=s: L.rtw_ctx_ao_map(
            h, C.byref(cam), W, H, time, mint, maxt, s, 7, AO.AO_MINT, radius, bvh, o[0], o[1], o[2], o[3], st))
    return scene, e


def pointer(buf):
    return None if buf is None else buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr()


def bits(buf):
    return np.ascontiguousarray(buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()).view(np.uint8)


def run(torch, r, entry, kinds, what):
    """One call with its caller pointers as `kinds` says: (the outputs, None for an absent one; the counters).  Checks the status, the tails
    and the device inputs."""
    place = lambda a, kind: a if kind == "host" else torch.from_numpy(a).to("cuda:0")
    ins = [place(a.copy(), k) for a, k in zip(entry.ins, kinds)]
    outs = [None if k == "absent" else place(np.full(n + TAIL, SENTINEL[dt], dt), k) for (n, dt, _), k in zip(entry.outs, kinds[len(ins):])]
    torch.cuda.synchronize()                                # (the context's own stream orders with nothing of torch's)
    st = R.RtwStats()
    rc = entry.call(r._h, [pointer(b) for b in ins], [pointer(b) for b in outs], C.byref(st))
    assert rc == R.RTW_OK, (what, kinds, rc)
    for k, (a, b) in enumerate(zip(entry.ins, ins)):
        assert np.array_equal(bits(b), bits(a)), (what, kinds, "input", k)
    got = []
    for k, ((n, dt, _), b) in enumerate(zip(entry.outs, outs)):
        if b is None:
            got.append(None)
            continue
        host = np.ascontiguousarray(b if isinstance(b, np.ndarray) else b.cpu().numpy())
        assert (host[n:] == dt(SENTINEL[dt])).all(), (what, kinds, "the tail of output", k)
        got.append(host[:n])
    assert st.kernel_ms > 0.0, (what, kinds)
    return got, tuple(getattr(st, k) for k in STATS)


def assert_answer(got, want, what):
    (g_out, g_st), (w_out, w_st) = got, want
    for k, (g, w) in enumerate(zip(g_out, w_out)):
        assert (g is None) == (w is None), (what, k)
        if g is not None:
            bad = np.flatnonzero(g.view(np.uint8) != w.view(np.uint8))
            assert len(bad) == 0, (what, "output", k, len(bad), bad[:8])
    assert g_st == w_st, (what, dict(zip(STATS, g_st)), dict(zip(STATS, w_st)))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    with R.Renderer(0) as r:
        yield r


@pytest.fixture(scope="module")
def reference(torch):
    """(scene, entries, {(name, kinds): (outputs, counters)}): every all-host call, once, on a context of its own."""
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    scene, e = entries()
    want = {}
    with R.Renderer(0) as r:
        r.set_scene(scene)
        for name, entry in e.items():
            for kinds in {entry.all_host(k) for k in entry.kinds()}:
                want[name, kinds] = run(torch, r, entry, kinds, name)
    full = lambda name: want[name, ("host",) * (len(e[name].ins) + len(e[name].outs))]
    (t, idx, _), st = full("scene_hits")
    assert 0.1 <= (idx >= 0).mean() <= 0.9 and np.isinf(t[idx < 0]).all() and st[2] > 0, "both outcomes, through the tree"
    assert 0.1 <= full("scene_occluded")[0][0].mean() <= 0.9
    assert 0.1 <= (full("depth_map")[0][1] >= 0).mean() <= 0.95
    for s in SAMPLES:
        (ao,), st = full(f"ambient_occlusion {s}")
        assert ao[5] == 1.0 and st[0] == (N - 1) * s and ao.min() < 1.0 and len(np.unique(ao)) >= 3
        (ao, _, ids, _), st = full(f"ao_map {s}")
        assert st[0] == W * H + s * int((ids >= 0).sum()) and (ao[ids < 0] == 1.0).all() and ao.min() < 1.0
    return scene, e, want


@pytest.mark.parametrize("name", list(FOLLOWED_BY))
def test_every_pointer_host_or_device_or_absent(ctx, torch, reference, name):
    scene, e, want = reference
    ctx.set_scene(scene)
    entry, n_calls = e[name], 0
    for kinds in entry.kinds():
        assert_answer(run(torch, ctx, entry, kinds, name), want[name, entry.all_host(kinds)], (name, kinds))
        n_calls += 1
    assert n_calls == 2 ** len(entry.ins) * 2 ** sum(not o for _, _, o in entry.outs) * 3 ** sum(o for _, _, o in entry.outs)
    after = FOLLOWED_BY[name]
    kinds = ("host",) * (len(e[after].ins) + len(e[after].outs))
    assert_answer(run(torch, ctx, e[after], kinds, after), want[after, kinds], (after, "after", name))


def test_the_host_array_calls_equal_the_host_forms(ctx):
    """rtw_ctx_triangle_hits, rtw_ctx_mesh_instance_hits (normals asked for and not) and rtw_ctx_perlin_eval always stage; each twice, around
    the others, so that no temporary of one reaches the next."""
    pods, placements, rays = OC.placement_case("standard")
    rays = rays[:N].copy()
    rays[-2, 3:], rays[-1, 3:] = np.nan, 0.0                # (as the full set ends: a NaN ray and a zero direction)
    install_placements(ctx, pods, placements)
    perlin, pts = R.PerlinNoise(2024), np.random.default_rng(5).uniform(-8.0, 8.0, (N, 3)).astype(F)
    tri = R.triangle_hits(list(pods), rays, MI.MINT, MI.MAXT)
    mesh = R.mesh_instance_hits(list(pods), placements, rays, MI.MINT, MI.MAXT)
    turb = perlin.turb(pts, 3)
    assert 0 < int((tri[1] >= 0).sum()) < N and len({int(p) for p in mesh[1] if p >= 0}) >= 4 and int((mesh[1] < 0).sum()) > 0
    for _ in range(2):
        t, idx, st = ctx.triangle_hits(rays, MI.MINT, MI.MAXT)
        assert MI.same_nan(t, tri[0]).all() and np.array_equal(idx, tri[1]) and st.quad_tests > 0
        MI.assert_hits_equal(ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT)[:4], mesh, "with normals")
        MI.assert_hits_equal(ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT, normals=False)[:3], mesh[:3], "without normals")
        got = ctx.perlin_eval(perlin, pts, 3)
        assert np.array_equal(got.view(np.uint32), np.asarray(turb, F).view(np.uint32))
