"""rtw_ctx_refit_triangles on the MI355X: the device's nodes against the host refit byte for byte, from numpy and from a torch tensor;
queries, renders and placements after a refit against the host and against a fresh context that got the moved mesh through set_triangles;
the call's place on a torch stream; idempotence; statuses.  Parity is on the bits everywhere."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import refit_common as RC
from tests.mesh_inst_common import same_nan
from tests.test_gpu_stream_order import Hazard, cycles_per_ms, same, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

F = np.float32
MINT, MAXT = 1e-3, 1e4
N_RAYS = 4096
E_INVALID, E_NO_SCENE = -1, -6


@pytest.fixture(scope="module")
def ctx():
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    with R.Renderer(0) as r:
        yield r


def scene_of(tris, spheres=()):
    return R.Scene(list(spheres), background=(0.7, 0.8, 1.0), triangles=tris)


def rays_at(w, n=N_RAYS, seed=5):
    """n rays [n][6] at the mesh with vertices w from all round it: three in four aimed at a vertex (shared edges and corners) or near one,
    the rest pointing away.  A vertex beyond 10^6 is no target."""
    rng = np.random.default_rng(seed)
    sane = w[np.abs(w).max(axis=1) < 1e6].astype(np.float64)
    c = sane.mean(axis=0)
    ext = np.abs(sane - c).max()
    tgt = sane[rng.integers(0, len(sane), n)]
    tgt[n // 2:] += rng.normal(scale=0.03 * ext, size=(n - n // 2, 3))
    d = rng.normal(size=(n, 3))
    o = c + 3.0 * ext * d / np.linalg.norm(d, axis=1, keepdims=True)
    d = (tgt - o) * rng.uniform(0.3, 2.0, (n, 1))
    d[::4] = -d[::4]
    return np.concatenate([o, d], 1).astype(F)


def assert_hits(got, want, what):
    (t, i), (t0, i0) = got, want
    assert np.array_equal(i, i0), (what, int((i != i0).sum()))
    assert same_nan(t, t0).all(), (what, int((~same_nan(t, t0)).sum()))


# ---- node bytes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["numpy", "torch"])
@pytest.mark.parametrize("name", list(RC.MESHES))
def test_device_nodes_equal_the_host_refit(ctx, torch, name, source):  # noqa: F811
    v, f, n_nodes, _ = RC.mesh(name)
    tris = R.Triangle.from_mesh(v, f)
    built = R.triangle_bvh_dump(tris)[0]
    ctx.set_scene(scene_of(tris))
    assert RC.same_bytes(ctx.triangle_bvh_dump(), built)

    def give(ouv):
        if source == "numpy":
            return ouv
        t = torch.from_numpy(ouv).to("cuda:0")
        torch.cuda.synchronize()
        return t

    # the same vertices: the device's double sqrt and divide round as the host's, or these bytes differ
    ouv = R.mesh_ouv(v, f)
    assert ctx.refit_triangles(give(ouv)) == 0
    assert RC.same_bytes(ctx.triangle_bvh_dump(), built)
    # the first deformation
    ouv = R.mesh_ouv(RC.sine_wave(v, f), f)
    want, lw = R.triangle_bvh_refit(tris, ouv)
    assert lw == 0 and len(want) == n_nodes
    assert ctx.refit_triangles(give(ouv)) == 0
    got = ctx.triangle_bvh_dump()
    assert RC.same_bytes(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    # idempotence: the same input again changes no byte
    assert ctx.refit_triangles(give(ouv)) == 0
    assert RC.same_bytes(ctx.triangle_bvh_dump(), want)


def test_a_device_pointer_with_n(ctx, torch):  # noqa: F811
    v, f, _, _ = RC.mesh("icosphere1")
    tris = R.Triangle.from_mesh(v, f)
    ouv = R.mesh_ouv(RC.sine_wave(v, f), f)
    ctx.set_scene(scene_of(tris))
    t = torch.from_numpy(ouv).to("cuda:0")
    torch.cuda.synchronize()
    assert ctx.refit_triangles(int(t.data_ptr()), n=len(f)) == 0
    assert RC.same_bytes(ctx.triangle_bvh_dump(), R.triangle_bvh_refit(tris, ouv)[0])
    with pytest.raises(ValueError):
        ctx.refit_triangles(int(t.data_ptr()))
    with pytest.raises(ValueError):
        ctx.refit_triangles(t.to(torch.float64))
    with pytest.raises(ValueError):
        ctx.refit_triangles(t.cpu())


# ---- hits ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.DEFORMATIONS))
def test_hits_after_a_refit_equal_the_host_and_a_fresh_context(ctx, name):
    v, f, _, _ = RC.mesh("icosphere2")
    deform, walk = RC.DEFORMATIONS[name]
    w = deform(v, f)
    old, new = RC.triangles_of(v, f), RC.triangles_of(w, f)
    n = len(f)
    ctx.set_scene(scene_of(old))
    assert ctx.refit_triangles(R.mesh_ouv(w, f)) == walk
    rays = rays_at(w)
    host = R.triangle_hits(new, rays, MINT, MAXT)
    if name != "degenerate":                                  # (a degenerate triangle reports a NaN-t hit for every ray it is asked first, rtw.h)
        assert 0.25 <= (host[1] >= 0).mean() <= 0.9, (host[1] >= 0).mean()
    with R.Renderer(0) as fresh:
        fresh.set_scene(scene_of(new))
        for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
            t, i, st = ctx.triangle_hits(rays, MINT, MAXT, accel)
            t1, i1, st1 = fresh.triangle_hits(rays, MINT, MAXT, accel)
            assert_hits((t, i), host, (name, accel, "host"))
            assert_hits((t, i), (t1, i1), (name, accel, "fresh"))
            if accel == R.ACCEL_BVH and walk == 0:
                assert st.node_tests > 0 and st.quad_tests < n * len(rays), (st.node_tests, st.quad_tests)
            else:
                assert st.node_tests == 0 and st.quad_tests == n * len(rays)                 # the list answers
                assert st1.node_tests == 0
    # back to the sane vertices: 0, and the tree is in use again
    assert ctx.refit_triangles(R.mesh_ouv(v, f)) == 0
    rays = rays_at(v)
    t, i, st = ctx.triangle_hits(rays, MINT, MAXT, R.ACCEL_BVH)
    assert_hits((t, i), R.triangle_hits(old, rays, MINT, MAXT), (name, "back"))
    assert st.node_tests > 0 and st.quad_tests < n * len(rays)


# ---- render, scene_hits, depth_map -------------------------------------------------------------------------------------------------------------
def test_render_and_scene_queries_equal_a_fresh_contexts(ctx):
    v, f = R.mesh_icosphere(2, (0.0, 1.0, 0.0), 1.0)
    w = (RC.sine_wave(v, f).astype(np.float64) * 0.8 + np.array([-3.5, 2.6, -0.5])).astype(F)      # back in front of the camera
    old, new = RC.triangles_of(v, f), RC.triangles_of(w, f)
    spheres = [R.Sphere.new((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5)), R.Sphere.new((1.5, 0.4, 0.5), 0.4, (0.8, 0.3, 0.3), R.METALLIC_M)]
    cam = R.Viewport.new_from_res(64, 48, 1, 4, 1.0, vfov=40.0, origin=(6.0, 3.0, 8.0), direction=(-6.0, -2.2, -8.0), vup=(0.0, 1.0, 0.0)).camera()
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = 64, 48, 4, 6, 1.0
    p.mint, p.maxt = 0.001, 1e4
    p.integrator, p.sampler, p.flags, p.seed = R.INTEGRATOR_RUST2, R.SAMPLER_ROW, 0, 77
    dcam = R.camera2_new(64 / 48, (6.0, 3.0, 8.0), (0.0, 1.0, 0.0), (-6.0, -2.2, -8.0), 40.0, 0.0)
    rays = rays_at(w, 2048, seed=9)

    def answers(r):
        out = {}
        for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
            p.accel = accel
            img, st = r.render(cam, p)
            t, i, nrm, qs = r.scene_hits(rays, MINT, MAXT, accel=accel, normals=True)
            depth, ids, _ = r.depth_map(dcam, 64, 48, MINT, MAXT, accel=accel, ids=True)
            out[accel] = dict(img=img, segments=st.segments, t=t, i=i, nrm=nrm, depth=depth, ids=ids, tests=st.quad_tests, nodes=qs.node_tests)
        return out

    ctx.set_scene(scene_of(old, spheres))
    assert ctx.refit_triangles(R.mesh_ouv(w, f)) == 0
    got = answers(ctx)
    with R.Renderer(0) as fresh:
        fresh.set_scene(scene_of(new, spheres))
        want = answers(fresh)
    for accel in got:
        g, x = got[accel], want[accel]
        assert g["segments"] == x["segments"]
        for k in ("img", "t", "i", "nrm", "depth", "ids"):
            assert RC.same_bytes(g[k], x[k]), (accel, k)
    assert RC.same_bytes(got[R.ACCEL_BVH]["img"], got[R.ACCEL_BRUTE]["img"])
    assert got[R.ACCEL_BVH]["tests"] < got[R.ACCEL_BRUTE]["tests"] and got[R.ACCEL_BVH]["nodes"] > 0         # the refitted tree is walked
    assert (got[R.ACCEL_BVH]["ids"] >= len(spheres)).mean() > 0.02                                           # the mesh is in the picture


# ---- placements ---------------------------------------------------------------------------------------------------------------------------------
def test_placements_after_a_refit_and_the_refusal_while_they_are_set(ctx):
    v, f = R.mesh_icosphere(1)
    w = (v.astype(np.float64) * np.array([1.1, 0.7, 1.2])).astype(F)
    w[:, 1] += (0.1 * np.sin(3.0 * w[:, 0].astype(np.float64))).astype(F)
    T = MI.standard_mesh()
    moved = []
    for k, (a, b, c) in enumerate(f):
        moved.append(dict(T.tris[k], origin=w[a].tolist(), u=(w[b] - w[a]).astype(F).tolist(), v=(w[c] - w[a]).astype(F).tolist()))
    new = MI.TriSet(moved).pods()
    placements, rays = MI.standard_placements(), MI.standard_rays()
    want = R.mesh_instance_hits(new, placements, rays, MI.MINT, MI.MAXT)
    assert 0.2 <= (want[1] >= 0).mean() <= 0.8
    ctx.set_scene(scene_of(None))
    ctx.set_triangles(T.pods())
    assert ctx.refit_triangles(R.mesh_ouv(w, f)) == 0
    ctx.set_mesh_instances(placements)
    try:
        for list_max in (R.lib().rtw_mesh_list_max_default(), 0):            # the placements in list order, then through their top-level tree
            ctx.set_option(R.OPT_MESH_LIST_MAX, list_max)
            for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
                got = ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT, accel)
                MI.assert_hits_equal(got[:4], want, (list_max, accel))
                assert (got[4].node_tests > 0) == (accel == R.ACCEL_BVH)
        with pytest.raises(R.RtwError) as e:
            ctx.refit_triangles(R.mesh_ouv(v, f))
        assert e.value.status == E_INVALID
        ctx.set_mesh_instances(None)
        assert ctx.refit_triangles(R.mesh_ouv(v, f)) == 0
    finally:
        ctx.set_option(R.OPT_MESH_LIST_MAX, R.lib().rtw_mesh_list_max_default())


# ---- stream order ---------------------------------------------------------------------------------------------------------------------------------
def test_refit_runs_behind_the_producer_of_its_tensor(torch, cycles_per_ms):  # noqa: F811
    """The ouv tensor is written by torch behind a delay on the stream of use_torch_stream; refit_triangles follows with no synchronise."""
    v, f, _, _ = RC.mesh("icosphere2")
    tris = R.Triangle.from_mesh(v, f)
    old, new = R.mesh_ouv(v, f), R.mesh_ouv(RC.sine_wave(v, f), f)
    with R.Renderer(0) as r:
        r.set_scene(scene_of(tris))
        before = r.triangle_bvh_dump()
        t = torch.from_numpy(new).to("cuda:0")
        torch.cuda.synchronize()
        assert r.refit_triangles(t) == 0                      # the synchronised run, on the context's own stream
        want = r.triangle_bvh_dump()
        assert not same(want, before)
        assert r.refit_triangles(old) == 0
        assert same(r.triangle_bvh_dump(), before)
        hz = Hazard(torch, cycles_per_ms)
        t_in = hz.input(new, stale=old)                       # (a refit that ran early reads the old vertices: the tree stays `before`)
        _, lw = hz.run(r, "torch-current", lambda: r.refit_triangles(t_in))
        assert lw == 0
        assert same(r.triangle_bvh_dump(), want)


# ---- statuses -----------------------------------------------------------------------------------------------------------------------------------
def test_statuses(ctx):
    L = R.lib()
    v, f, n_nodes, _ = RC.mesh("row5")
    ouv = R.mesh_ouv(v, f)
    nn, lw = C.c_uint32(), C.c_uint32()
    ctx.set_scene(scene_of(None))
    assert L.rtw_ctx_refit_triangles(ctx._h, ouv.ctypes.data, 5, C.byref(lw)) == E_NO_SCENE
    assert L.rtw_ctx_triangle_bvh_dump(ctx._h, None, 0, C.byref(nn)) == E_NO_SCENE
    ctx.set_triangles(R.Triangle.from_mesh(v, f))
    assert L.rtw_ctx_refit_triangles(None, ouv.ctypes.data, 5, None) == E_INVALID
    assert L.rtw_ctx_refit_triangles(ctx._h, None, 5, None) == E_INVALID
    assert L.rtw_ctx_refit_triangles(ctx._h, ouv.ctypes.data, 4, None) == E_INVALID
    assert L.rtw_ctx_refit_triangles(ctx._h, ouv.ctypes.data, 6, None) == E_INVALID
    assert L.rtw_ctx_refit_triangles(ctx._h, ouv.ctypes.data, 5, None) == 0              # (list_walk_out may be NULL)
    nodes = np.zeros(n_nodes, R.TOP_NODE)
    assert L.rtw_ctx_triangle_bvh_dump(ctx._h, nodes.ctypes.data, n_nodes - 1, None) == E_INVALID
    assert L.rtw_ctx_triangle_bvh_dump(ctx._h, None, 0, C.byref(nn)) == 0 and nn.value == n_nodes
    assert L.rtw_ctx_triangle_bvh_dump(ctx._h, nodes.ctypes.data, n_nodes, None) == 0
    assert RC.same_bytes(nodes, R.triangle_bvh_dump(R.Triangle.from_mesh(v, f))[0])
