"""rtw_ctx_ambient_occlusion / rtw_ctx_ao_map on the MI355X, exactly: ao[i] is (samples - c_i) / samples with c_i what rtw_ctx_scene_occluded
counts over ray [i][k] of rtw_ao_rays on the same context -- for every point, under both accels and every fall-back, whatever lanes share a
wave -- with the counters of that call; against the CPU oracle on the point sets of tests/ao_common.py (tests/test_ao_cpu.py proves that they
exercise every outcome); and ao_map against its definition as a composition of depth_map and ambient_occlusion."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import ao_common as AO
from tests import mesh_inst_common as MI
from tests import mesh_move_common as MM
from tests import mesh_top_common as MT
from tests import occluded_common as OC
from tests import quat_common as QC
from tests import refit_common as RC
from tests.test_gpu_occluded import MODES, Mode, install_placements
from tests.test_gpu_scene_hits import MAXT, MINT, depth_camera
from tests.test_gpu_stream_order import Hazard, ctx, cycles_per_ms, fresh, same, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_NO_SCENE = -1, -6
COUNTERS = ("sphere_tests", "node_tests", "quad_tests")


def composition(r, points, normals, samples, radius, mint=AO.AO_MINT, seed=0, time=0.0, accel=R.ACCEL_BVH):
    """The contract's right-hand side on context `r`: (ao, counts, (segments, sphere_tests, node_tests, quad_tests)) from scene_occluded over
    the rays of ao_rays, the rays of skipped points left out (they are cast by nobody)."""
    points, normals = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    skip = AO.skipped(normals)
    rays = R.ao_rays(points, normals, samples, seed)
    counts = np.zeros(len(points), np.int64)
    stats = (0, 0, 0, 0)
    if not skip.all():
        occ, st = r.scene_occluded(np.ascontiguousarray(rays[~skip]).reshape(-1, 6), mint, radius, time=time, accel=accel)
        counts[~skip] = occ.reshape(-1, samples).sum(axis=1)
        stats = (st.segments,) + tuple(getattr(st, k) for k in COUNTERS)
    return AO.ao_of(counts, samples, skip), counts, stats


def check(r, points, normals, samples, radius, what, **kw):
    """ambient_occlusion against the composition, bytes and counters; returns (ao, counts, RtwStats)."""
    ao, st = r.ambient_occlusion(points, normals, samples, radius, **kw)
    want, counts, stats = composition(r, points, normals, samples, radius, **kw)
    assert ao.dtype == F and ao.shape == want.shape, (what, ao.dtype, ao.shape)
    bad = np.flatnonzero(ao.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:8], ao[bad[:8]], want[bad[:8]])
    assert (st.segments,) + tuple(getattr(st, k) for k in COUNTERS) == stats, (what, "segments and counters against scene_occluded's")
    assert st.kernel_ms > 0.0
    return ao, counts, st


def mixed(counts, samples):
    """Both outcomes among the rays, and a point that is neither free nor shut."""
    return 0 < counts.sum() < samples * len(counts) and bool(np.any((counts > 0) & (counts < samples)))


# ---- against the oracle and the composition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", AO.CASES)
def test_point_sets_equal_the_oracle_and_the_composition(gpu, oracle, name, mode):
    scene, (t0, t1), _, time, _, _ = AO.case(name)
    p, n = AO.points_of(oracle, name)
    want_counts, want = AO.reference(oracle, name)
    gpu.set_scene(scene, t0, t1)
    with Mode(gpu, mode) as accel:
        ao, counts, st = check(gpu, p, n, AO.SAMPLES, AO.RADIUS[name], (name, mode), time=time, accel=accel)
    assert np.array_equal(counts, want_counts) and same(ao, want), (name, mode, "against the oracle")
    assert st.segments == AO.SAMPLES * len(p)
    print(f"\n[ao] {name}, {mode}: {len(p)} points x {AO.SAMPLES}: " + ", ".join(f"{k} {getattr(st, k)}" for k in COUNTERS))
    if mode == "brute":
        assert st.node_tests == 0
    if mode == "tree forced" and name != "geom":                        # (geom's tree nodes would be its triangles': spheres or not)
        assert st.node_tests > 0 and st.sphere_tests < scene.n_spheres * st.segments


# ---- group and wave edges ------------------------------------------------------------------------------------------------------------------------
EDGES = [(s, n) for s in (1, 2, 16, 64, 128, 1024) for n in (1, 3, 4, 5, 63, 64, 65, 257)] + [(1024, 2)]     # (1, 2 and 3 points at 1024 samples)


@pytest.mark.parametrize("samples,n", EDGES)
def test_group_and_wave_edges(gpu, oracle, torch, samples, n):  # noqa: F811
    scene, _, _, _, _, _ = AO.case("field")
    p, nrm = AO.points_of(oracle, "field")
    p, nrm = np.ascontiguousarray(p[:n]), np.ascontiguousarray(nrm[:n])
    gpu.set_scene(scene)
    with Mode(gpu, "tree forced") as accel:
        ao, counts, _ = check(gpu, p, nrm, samples, AO.RADIUS["field"], (samples, n), accel=accel)
        d_out = torch.full((n + 1,), 7.0, dtype=torch.float32, device="cuda:0")
        d_p, d_n = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(nrm).to("cuda:0")
        torch.cuda.synchronize()
        out, st = gpu.ambient_occlusion(d_p, d_n, samples, AO.RADIUS["field"], accel=accel, out=d_out[:n])
    got = d_out.cpu().numpy()
    assert got[n] == 7.0, "the float behind ao_out was written"
    assert same(got[:n], ao) and out.data_ptr() == d_out.data_ptr() and st.segments == samples * n
    if samples == AO.SAMPLES:                                           # the prefix of the oracle's answer: ray [i][k] does not depend on n
        assert same(ao, AO.reference(oracle, "field")[1][:n])
    if n >= 63 and samples >= 16:
        assert mixed(counts, samples)


# ---- skipped and spoiling points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 16, 128])
def test_skipped_points(gpu, oracle, samples):
    scene, _, _, _, _, _ = AO.case("field")
    p, nrm = AO.points_of(oracle, "field")
    per_wave = max(1, 64 // samples)                                    # points of a wave
    n = min(len(p), 5 * per_wave + 3)
    p, base = np.ascontiguousarray(p[:n]), np.ascontiguousarray(nrm[:n])
    gpu.set_scene(scene)
    plain, _, _ = check(gpu, p, base, samples, AO.RADIUS["field"], (samples, "nobody skipped"))
    cases = {"first of a wave's groups": [0, 2 * per_wave], "last of a wave's groups": [per_wave - 1, 3 * per_wave - 1],
             "a whole wave": list(range(per_wave, 2 * per_wave)), "the last, partial wave": list(range(5 * per_wave, n)),
             "every point": list(range(n))}
    for what, which in cases.items():
        nrm = base.copy()
        nrm[which] = 0.0
        nrm[which[0]] = [-0.0, 0.0, -0.0]
        ao, _, st = check(gpu, p, nrm, samples, AO.RADIUS["field"], (samples, what))
        mates = np.ones(n, bool)
        mates[which] = False
        assert (ao[which] == 1.0).all() and same(ao[mates], plain[mates]), (samples, what)
        assert st.segments == samples * int(mates.sum())
        if what == "every point":
            assert (st.segments, st.sphere_tests, st.node_tests, st.quad_tests) == (0, 0, 0, 0) and (ao == 1.0).all()


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_spoilers_and_permutations(gpu, oracle, accel):
    scene, _, _, _, _, _ = AO.case("field")
    p, nrm = AO.points_of(oracle, "field")
    n = 256                                                             # 64 waves of 4 points at 16 samples
    p, nrm = np.ascontiguousarray(p[:n]), np.ascontiguousarray(nrm[:n])
    want = AO.reference(oracle, "field")[1][:n]
    gpu.set_scene(scene)
    with Mode(gpu, "tree forced" if accel == R.ACCEL_BVH else "brute") as a:
        ao, _, _ = check(gpu, p, nrm, 16, AO.RADIUS["field"], "unspoiled", accel=a)
        assert same(ao, want)
        for what in ("a NaN point", "a point beyond 2^60", "a NaN normal"):
            sp, sn = p.copy(), nrm.copy()
            pos = np.arange(0, n, 4) + (np.arange(n // 4) * 7) % 4      # one per wave, its place in the wave varying
            if what == "a NaN point":
                sp[pos, 1] = np.nan
            elif what == "a point beyond 2^60":
                sp[pos, 0] = F(2.0 ** 61)
            else:
                sn[pos, 2] = np.nan
            got, _, _ = check(gpu, sp, sn, 16, AO.RADIUS["field"], what, accel=a)       # the spoilers answer what the composition answers
            mates = np.ones(n, bool)
            mates[pos] = False
            assert same(got[mates], want[mates]), (what, "the three mates of every wave keep the oracle's answer")
        for perm in (np.arange(n)[::-1], np.random.default_rng(5).permutation(n)):
            got, counts, _ = check(gpu, p[perm], nrm[perm], 16, AO.RADIUS["field"], "permuted", accel=a)   # (the index is the position: recomputed)
            assert mixed(counts, 16) and not same(got, want[perm])


# ---- ao_map equals its definition ------------------------------------------------------------------------------------------------------------------
def map_points(r, cam, width, height, mint, maxt, time=0.0, accel=R.ACCEL_BVH):
    """The points the camera forms shade, by their text: depth_map, then o + d * depth and the normals faced towards the viewer in numpy (one
    f32 rounding per operation), zeros for a miss pixel; (points, faced normals, flipped, depth, ids, normals, depth_map's RtwStats)."""
    depth, ids, nrm, dst = r.depth_map(cam, width, height, mint, maxt, time=time, accel=accel, ids=True, normals=True)
    rays = R.depth_rays(cam, width, height)
    o, d = rays[:, :3], rays[:, 3:]
    t, hit, n = depth.reshape(-1), ids.reshape(-1) >= 0, nrm.reshape(-1, 3)
    p = (o + (d * t[:, None]).astype(F)).astype(F)
    dot = ((d[:, 0] * n[:, 0]).astype(F) + (d[:, 1] * n[:, 1]).astype(F)).astype(F) + (d[:, 2] * n[:, 2]).astype(F)
    flip = dot.astype(F) > 0.0
    faced = np.where(flip[:, None], -n, n).astype(F)
    faced[~hit] = 0.0
    p[~hit] = 0.0
    return p, faced, flip & hit, depth, ids, nrm, dst


def definition(r, cam, width, height, mint, maxt, samples, radius, ao_mint=AO.AO_MINT, seed=0, accel=R.ACCEL_BVH, time=0.0):
    """rtw_ctx_ao_map by its text: map_points, then ambient_occlusion; (ao, depth, ids, normals, faced, (segments, counters...))."""
    p, faced, flipped, depth, ids, nrm, dst = map_points(r, cam, width, height, mint, maxt, time, accel)
    ao, ast = r.ambient_occlusion(p, faced, samples, radius, mint=ao_mint, seed=seed, time=time, accel=accel)
    stats = (dst.segments + ast.segments,) + tuple(getattr(dst, k) + getattr(ast, k) for k in COUNTERS)
    return ao.reshape(height, width), depth, ids, nrm, flipped, stats


def check_map(r, cam, width, height, what, mint=MINT, maxt=MAXT, samples=16, radius=5.0, accel=R.ACCEL_BVH, ao_mint=AO.AO_MINT, seed=0, time=0.0):
    want, depth, ids, nrm, flipped, stats = definition(r, cam, width, height, mint, maxt, samples, radius, ao_mint, seed, accel, time)
    kw = dict(ao_mint=ao_mint, seed=seed, time=time, accel=accel)
    ao, d, i, n, st = r.ao_map(cam, width, height, mint, maxt, samples, radius, depth=True, ids=True, normals=True, **kw)
    assert ao.shape == (height, width) and same(ao, want), (what, "ao against the definition")
    assert same(d, depth) and same(i, ids) and same(n, nrm), (what, "depth, ids and normals are depth_map's bytes")
    assert (st.segments,) + tuple(getattr(st, k) for k in COUNTERS) == stats and st.kernel_ms > 0.0, (what, "counters")
    assert st.segments == width * height + samples * int((ids >= 0).sum())
    assert (ao[ids < 0] == 1.0).all()
    alone, st0 = r.ao_map(cam, width, height, mint, maxt, samples, radius, **kw)             # no depth-pass output asked for
    assert same(alone, ao) and st0.segments == st.segments
    return ao, ids, flipped


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_ao_map_equals_its_definition(gpu, accel):
    gpu.set_scene(AO.case("geom")[0])
    W, H = 96, 64
    ao, ids, flipped = check_map(gpu, depth_camera("geom", W, H), W, H, "geom 96 x 64", accel=accel)
    hit = ids >= 0
    assert 0.2 <= hit.mean() <= 0.8 and len(np.unique(ao[hit])) >= 8 and ao[hit].min() < 1.0
    assert flipped.any() and (hit.reshape(-1) & ~flipped).any(), "the floor is seen from its back, the wall from its front"


@pytest.mark.parametrize("width,height", [(1, 1), (5, 3), (64, 1), (65, 2)])
def test_ao_map_of_small_and_narrow_images(gpu, width, height):
    gpu.set_scene(AO.case("geom")[0])
    check_map(gpu, depth_camera("geom", width, height), width, height, (width, height))


def test_ao_map_of_the_sky_and_of_a_quad_from_behind(gpu):
    gpu.set_scene(AO.case("geom")[0])
    W, H = 40, 24
    sky = R.camera2_new(W / H, (0.0, 0.3, 1.5), (0.0, 1.0, 0.0), (0.0, 0.1, 1.0), 75.0, 0.0)             # away from everything
    ao, ids, _ = check_map(gpu, sky, W, H, "sky")
    assert (ids < 0).all() and (ao == 1.0).all()
    _, st = gpu.ao_map(sky, W, H, MINT, MAXT, 16, 5.0)
    assert st.segments == W * H
    behind = R.camera2_new(W / H, (0.0, 0.3, -9.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 60.0, 0.0)        # behind the wall z = -6, normal +z
    ao, ids, flipped = check_map(gpu, behind, W, H, "behind the wall")
    wall = ids.reshape(-1) == AO.case("geom")[0].n_spheres                                               # quad 0
    assert wall.sum() >= W * H // 4 and flipped[wall].all(), "the wall's normal is not turned towards the viewer"
    assert (ao.reshape(-1)[wall] == 1.0).mean() > 0.5                   # nothing lies behind the wall: faced the wrong way, its own scene would shade it


# ---- each group alone --------------------------------------------------------------------------------------------------------------------------------
def hit_points(r, rays, mint, maxt, accel=R.ACCEL_BVH):
    """Points and viewer-facing normals from this context's own closest hits of `rays` (inputs only: any points would do)."""
    t, idx, nrm, _ = r.scene_hits(rays, mint, maxt, accel=accel, normals=True)
    rays = np.asarray(rays, F).reshape(-1, 6)
    hit = (idx >= 0) & np.isfinite(t)
    o, d, n = rays[hit, :3], rays[hit, 3:], nrm[hit]
    flip = np.einsum("ij,ij->i", d.astype(np.float64), n.astype(np.float64)) > 0
    return np.ascontiguousarray((o + d * t[hit, None]).astype(F)), np.ascontiguousarray(np.where(flip[:, None], -n, n).astype(F))


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
@pytest.mark.parametrize("group", OC.GROUPS)
def test_each_group_alone(gpu, group, accel):
    scene, _, rays, _, mint, maxt = OC.scene_case(group)
    gpu.set_scene(scene)
    with Mode(gpu, "tree forced" if accel == R.ACCEL_BVH else "brute") as a:
        p, n = hit_points(gpu, rays, mint, maxt)
        assert len(p) >= 32, group
        q, m = AO.random_points(256, 11)                                # ... and points in the air about the objects
        p, n = np.concatenate([p, q]), np.concatenate([n, m])
        _, counts, st = check(gpu, p, n, 16, 2.5, (group, accel), accel=a)
    assert 0 < counts.sum() < 16 * len(p), (group, "one outcome only")
    if group == "spheres":
        assert st.quad_tests == 0 and st.sphere_tests > 0
    if group in ("quads", "triangles"):
        assert st.sphere_tests == 0 and st.quad_tests > 0


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_quaternion_instances(gpu, accel):
    g = QC.golden()
    QC.fixture_scene(g).install(gpu)
    cam = QC.camera(g, 40, 30)
    p, n = hit_points(gpu, R.depth_rays(cam, 40, 30), g["mint"], g["maxt"])
    assert len(p) >= 100
    q = (np.asarray(g["translation"]) + np.random.default_rng(11).uniform(-1.5, 1.5, (256, 3))).astype(F)       # ... and points in the air about the box
    p, n = np.concatenate([p, q]), np.concatenate([n, AO.random_points(256, 11)[1]])
    _, counts, _ = check(gpu, p, n, 16, 1.0, "the golden rotation scene", accel=accel)
    assert mixed(counts, 16)
    check_map(gpu, cam, 40, 30, "the golden rotation scene", mint=g["mint"], maxt=g["maxt"], radius=1.0, accel=accel)


def test_placements_in_list_order_and_through_the_top_level_tree(gpu):
    nodes = {}
    try:
        for name, list_max in (("standard", R.MESH_LIST_MAX_DEFAULT), ("grid8", 0), ("grid8", MT.NEVER)):
            pods, pl, rays = OC.placement_case(name)
            install_placements(gpu, pods, pl)
            gpu.set_option(R.OPT_MESH_LIST_MAX, list_max)
            p, n = hit_points(gpu, rays, MI.MINT, MI.MAXT)
            assert len(p) >= 100, name
            for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
                _, counts, st = check(gpu, p, n, 16, 1.5, (name, list_max, accel), accel=accel)
                assert mixed(counts, 16), (name, list_max, accel)
                assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
                nodes[name, list_max, accel] = st.node_tests
    finally:
        gpu.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)
    assert nodes["grid8", 0, R.ACCEL_BVH] < nodes["grid8", MT.NEVER, R.ACCEL_BVH]


def test_a_refit_and_a_move_are_seen_by_the_next_call(ctx):  # noqa: F811
    # a refit: points on the deformed terrain, occluded by its own waves
    v, f, _, _ = RC.mesh("terrain12")
    w = RC.sine_wave(v, f)
    ctx.set_scene(R.Scene((), triangles=RC.triangles_of(w, f)))
    p, n = hit_points(ctx, OC.mesh_rays(w, f), MI.MINT, MI.MAXT)
    ctx.set_scene(R.Scene((), triangles=RC.triangles_of(v, f)))
    before, _, _ = check(ctx, p, n, 16, 3.0, "before the refit")
    assert ctx.refit_triangles(R.mesh_ouv(w, f)) == 0
    after = {accel: check(ctx, p, n, 16, 3.0, ("after the refit", accel), accel=accel)[0] for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE)}
    with R.Renderer(0) as other:
        other.set_scene(R.Scene((), triangles=RC.triangles_of(w, f)))
        want, _ = other.ambient_occlusion(p, n, 16, 3.0)
    for accel in after:
        assert same(after[accel], want), ("a fresh context with the deformed mesh", accel)
    assert not same(want, before) and 0.0 < want.mean() < 1.0
    # a move
    pods, pl, rays = OC.placement_case("grid8")
    moved = MM.turn_and_shift(MM.as_array(pl))
    install_placements(ctx, pods, pl)
    p, n = hit_points(ctx, rays, MI.MINT, MI.MAXT)
    before, _, _ = check(ctx, p, n, 16, 1.5, "before the move")
    assert ctx.move_mesh_instances(moved) == 0
    after = {accel: check(ctx, p, n, 16, 1.5, ("after the move", accel), accel=accel)[0] for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE)}
    with R.Renderer(0) as other:
        install_placements(other, pods, MM.as_list(moved))
        want, _ = other.ambient_occlusion(p, n, 16, 1.5)
    for accel in after:
        assert same(after[accel], want), ("a fresh context with the moved placements", accel)
    assert not same(want, before)


# ---- torch and lifecycle -----------------------------------------------------------------------------------------------------------------------------
def test_torch_tensors_and_the_producers_of_them(ctx, oracle, torch, cycles_per_ms):  # noqa: F811
    scene, _, _, _, _, _ = AO.case("field")
    p, n = AO.points_of(oracle, "field")
    want = AO.reference(oracle, "field")[1]
    radius = AO.RADIUS["field"]
    ctx.set_scene(scene)
    d_p, d_n = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(n).to("cuda:0")
    torch.cuda.synchronize()
    out, st = ctx.ambient_occlusion(d_p, d_n, AO.SAMPLES, radius)       # out allocated; on the context's own stream
    assert out.dtype == torch.float32 and out.is_cuda and same(out.cpu().numpy(), want) and st.segments == AO.SAMPLES * len(p)
    ao, _ = ctx.ambient_occlusion(p, n, AO.SAMPLES, radius)
    assert same(ao, want), "numpy in and out"
    with pytest.raises(ValueError):
        ctx.ambient_occlusion(p, n, AO.SAMPLES, radius, out=np.zeros(len(p), F))
    with pytest.raises(ValueError):
        ctx.ambient_occlusion(d_p, n, AO.SAMPLES, radius)
    with pytest.raises(ValueError):
        ctx.ambient_occlusion(d_p, d_n, AO.SAMPLES, radius, out=torch.zeros(len(p), dtype=torch.float64, device="cuda:0"))
    # behind a delayed producer on torch's default stream: stale points far above everything (nothing occludes them), stale outputs
    away_p = np.tile(np.array([0.0, 2000.0, 0.0], F), (len(p), 1))
    away_n = np.tile(np.array([0.0, 1.0, 0.0], F), (len(p), 1))
    assert (ctx.ambient_occlusion(away_p, away_n, AO.SAMPLES, radius)[0] == 1.0).all() and want.min() < 1.0
    hz = Hazard(torch, cycles_per_ms)
    h_p, h_n = hz.input(p, stale=away_p), hz.input(n, stale=away_n)
    h_out = hz.output((len(p),), torch.float32, 9.0, 7.0)
    (got,), (_, st) = hz.run(ctx, "torch-default", lambda: ctx.ambient_occlusion(h_p, h_n, AO.SAMPLES, radius, out=h_out))
    assert same(got, want) and st.segments == AO.SAMPLES * len(p)


def test_lifecycle_and_statuses(ctx, oracle):  # noqa: F811
    L = R.lib()
    scene, _, _, _, _, _ = AO.case("geom")
    p, n = AO.points_of(oracle, "geom")
    p4, n4 = np.ascontiguousarray(p[:4]), np.ascontiguousarray(n[:4])
    out = np.zeros(4, F)
    cam = depth_camera("geom", 2, 2)
    pp, nn, oo = p4.ctypes.data, n4.ctypes.data, out.ctypes.data
    rng = (0.0, 1e-3, 5.0)                                              # time, mint, maxt

    def ao(h, points=pp, normals=nn, count=4, samples=16, accel=R.ACCEL_BVH, dst=oo):
        return L.rtw_ctx_ambient_occlusion(h, points, normals, count, samples, 0, *rng, accel, dst, None)

    def ao_map(h, camera=C.byref(cam), w=2, hh=2, samples=16, accel=R.ACCEL_BVH, dst=oo):
        return L.rtw_ctx_ao_map(h, camera, w, hh, 0.0, MINT, MAXT, samples, 0, 1e-3, 5.0, accel, dst, None, None, None, None)

    with R.Renderer(0) as other:
        assert ao(other._h) == E_NO_SCENE and ao_map(other._h) == E_NO_SCENE
        with pytest.raises(R.RtwError):
            other.ambient_occlusion(p4, n4)
        other.set_scene(scene)
        second, _ = other.ambient_occlusion(p, n, 16, 5.0)
        second_map = other.ao_map(cam, 2, 2, MINT, MAXT, 16, 5.0)[0]
    ctx.set_scene(scene)
    for bad in (ao(None), ao(ctx._h, points=None), ao(ctx._h, normals=None), ao(ctx._h, dst=None), ao(ctx._h, count=0), ao(ctx._h, accel=2),
                ao(ctx._h, samples=0), ao(ctx._h, samples=3), ao(ctx._h, samples=2048), ao(ctx._h, count=2 ** 32 - 1, samples=1024),
                ao_map(None), ao_map(ctx._h, camera=None), ao_map(ctx._h, dst=None), ao_map(ctx._h, w=0), ao_map(ctx._h, hh=0),
                ao_map(ctx._h, accel=2), ao_map(ctx._h, samples=5), ao_map(ctx._h, w=65536, hh=65535, samples=2)):
        assert bad == E_INVALID
    assert not out.any()
    assert ao(ctx._h) == R.RTW_OK                                       # (stats may be NULL)
    first, _ = ctx.ambient_occlusion(p, n, 16, 5.0)
    assert same(first, second) and same(first[:4], out) and same(first, AO.reference(oracle, "geom")[1])
    assert ao_map(ctx._h) == R.RTW_OK and same(out.reshape(2, 2), second_map)
