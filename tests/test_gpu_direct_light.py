"""rtw_ctx_direct_light / rtw_ctx_direct_light_map on the MI355X, exactly: for every (point, light) pair vis is v / samples with v the cast
samples for which rtw_ctx_scene_occluded answers 0 over ray [i][l][k] of rtw_light_samples on the same context, irr is rtw_light_reduce of
the host weights under that mask, and the counters are that call's -- under both accels and every fall-back, whatever lanes share a wave --;
against the CPU oracle on the point sets of tests/direct_light_common.py (tests/test_direct_light_cpu.py proves that they exercise every
outcome); and direct_light_map against its definition as a composition of depth_map and direct_light."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import ao_common as AO
from tests import direct_light_common as DL
from tests import mesh_inst_common as MI
from tests import mesh_move_common as MM
from tests import occluded_common as OC
from tests import quat_common as QC
from tests import query_edges_common as QE
from tests import refit_common as RC
from tests.test_gpu_ao import hit_points, map_points
from tests.test_gpu_occluded import MODES, Mode
from tests.test_gpu_query_staging import N, TAIL, H, W, Entry, assert_answer, run
from tests.test_gpu_scene_hits import MAXT, MINT, depth_camera, geom_scene
from tests.test_gpu_stream_order import Hazard, ctx, cycles_per_ms, same, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_NO_SCENE = -1, -6
COUNTERS = ("sphere_tests", "node_tests", "quad_tests")
LO, HI = DL.LO, DL.HI


def counters(st):
    return (st.segments,) + tuple(getattr(st, k) for k in COUNTERS)


def composition(r, scene, lights, points, normals, samples, seed=0, time=0.0, accel=R.ACCEL_BVH, lo=LO, hi=HI):
    """The contract's right-hand side on context `r`: (vis, irr, v, cast counts, (segments, sphere_tests, node_tests, quad_tests)) from
    scene_occluded over the cast rays of light_samples, then light_reduce."""
    rays, w = R.light_samples(scene, lights, points, normals, samples, seed)
    cast = DL.cast_mask(rays)
    occ = np.zeros(cast.shape, bool)
    stats = (0, 0, 0, 0)
    if cast.any():
        occ[cast], st = r.scene_occluded(np.ascontiguousarray(rays[cast]), lo, hi, time=time, accel=accel)
        stats = counters(st)
        assert st.segments == int(cast.sum())
    vis, irr, v = DL.outputs(w, cast, occ, samples)
    return vis, irr, v, cast.sum(axis=-1), stats


def check(r, scene, lights, points, normals, samples, what, **kw):
    """direct_light against the composition, bytes and counters; returns (vis, irr, v, cast counts, RtwStats)."""
    vis, irr, st = r.direct_light(points, normals, samples, **kw)
    want_vis, want_irr, v, cast, stats = composition(r, scene, lights, points, normals, samples, **kw)
    assert vis.dtype == F and irr.dtype == F and vis.shape == want_vis.shape == irr.shape, (what, vis.shape, want_vis.shape)
    for name, got, want in (("vis", vis, want_vis), ("irr", irr, want_irr)):
        bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
        assert len(bad) == 0, (what, name, len(bad), bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
    assert counters(st) == stats, (what, "segments and counters against scene_occluded's", counters(st), stats)
    assert st.kernel_ms > 0.0
    alone, st1 = r.direct_light(points, normals, samples, irradiance=False, **kw)         # irr_out absent
    assert same(alone, vis) and counters(st1) == stats, (what, "without irr_out")
    return vis, irr, v, cast, st


def install(r, name):
    scene, lights, (t0, t1), _, time, _, _ = DL.case(name)
    r.set_scene(scene, t0, t1)
    r.set_lights(lights)
    return scene, lights, time


def mixed(v, cast, samples):
    """Both outcomes among the cast rays, and an item that is neither dark nor fully lit."""
    return 0 < v.sum() < cast.sum() and bool(np.any((v > 0) & (v < samples)))


# ---- against the oracle and the composition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", DL.CASES)
def test_point_sets_equal_the_oracle_and_the_composition(gpu, oracle, name, mode):
    scene, lights, time = install(gpu, name)
    p, n = DL.points_of(oracle, name)
    want_vis, want_irr, want_v, want_cast = DL.reference(oracle, name)
    with Mode(gpu, mode) as accel:
        vis, irr, v, cast, st = check(gpu, scene, lights, p, n, DL.SAMPLES, (name, mode), time=time, accel=accel)
    assert np.array_equal(v, want_v) and np.array_equal(cast, want_cast) and same(vis, want_vis) and same(irr, want_irr), (name, mode, "against the oracle")
    assert st.segments == int(want_cast.sum())
    print(f"\n[direct] {name}, {mode}: {len(p)} points x {len(lights)} lights x {DL.SAMPLES}: " + ", ".join(f"{k} {getattr(st, k)}" for k in COUNTERS))
    if mode == "brute":
        assert st.node_tests == 0
    if mode == "tree forced" and name != "geom":                        # (geom's tree nodes would be its triangles': spheres or not)
        assert st.node_tests > 0 and st.sphere_tests < scene.n_spheres * st.segments


# ---- group and wave edges ------------------------------------------------------------------------------------------------------------------------
FIELD_LIGHTS = [(R.LIGHT_QUAD, 1), (R.LIGHT_SPHERE, 2), (R.LIGHT_SPHERE, 10), (R.LIGHT_QUAD, 0)] + [(R.LIGHT_SPHERE, 20 + k) for k in range(12)]
EDGES = ([(s, n, 1) for s in (1, 2, 16, 64, 128) for n in (1, 3, 63, 64, 65, 257)] +
         [(s, n, nl) for s in (1, 16, 128) for n in (1, 3, 65) for nl in (2, 3, 16)] +
         [(2, 64, 3), (64, 63, 2), (16, 257, 3), (1024, 2, 1), (1024, 2, 3)])


@pytest.fixture(scope="module")
def field_points():
    """Points among the objects of QE.field_scene(): random ones in the air about them, half with the normal turned upwards (towards the light
    above nothing stands on) so that many samples are cast."""
    p, n = AO.random_points(257, 31)
    n[::2, 1] = np.abs(n[::2, 1])
    return np.ascontiguousarray(p), np.ascontiguousarray(n)


@pytest.mark.parametrize("samples,n,nl", EDGES)
def test_group_and_wave_edges(gpu, torch, field_points, samples, n, nl):  # noqa: F811
    scene, lights = QE.field_scene(), FIELD_LIGHTS[:nl]
    p, nrm = field_points[0][:n].copy(), field_points[1][:n].copy()
    gpu.set_scene(scene)
    gpu.set_lights(lights)
    assert gpu.light_count() == nl
    with Mode(gpu, "tree forced") as accel:
        vis, irr, v, cast, _ = check(gpu, scene, lights, p, nrm, samples, (samples, n, nl), accel=accel)
        d_vis = torch.full((n * nl + 1,), 7.0, dtype=torch.float32, device="cuda:0")     # a guard float behind each device output
        d_irr = torch.full((n * nl + 1,), 7.0, dtype=torch.float32, device="cuda:0")
        d_p, d_n = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(nrm).to("cuda:0")
        torch.cuda.synchronize()
        out_vis, out_irr, st = gpu.direct_light(d_p, d_n, samples, accel=accel, out_vis=d_vis[:n * nl], out_irr=d_irr[:n * nl])
    got_vis, got_irr = d_vis.cpu().numpy(), d_irr.cpu().numpy()
    assert got_vis[-1] == 7.0 and got_irr[-1] == 7.0, "the float behind an output was written"
    assert same(got_vis[:-1].reshape(n, nl), vis) and same(got_irr[:-1].reshape(n, nl), irr)
    assert out_vis.data_ptr() == d_vis.data_ptr() and out_irr.data_ptr() == d_irr.data_ptr() and st.segments == int(cast.sum())
    if n >= 63 and samples >= 16:
        assert mixed(v, cast, samples)


# ---- skipped and spoiling points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples,nl", [(1, 1), (16, 3), (16, 1), (128, 2)])
def test_skipped_points(gpu, field_points, samples, nl):
    """(16, 3): a wave holds four groups and a point three items, so a wave's groups straddle points."""
    scene, lights = QE.field_scene(), FIELD_LIGHTS[:nl]
    items_per_wave = max(1, 64 // samples)
    n = min(257, 5 * items_per_wave + 3)
    p, base = field_points[0][:n].copy(), field_points[1][:n].copy()
    gpu.set_scene(scene)
    gpu.set_lights(lights)
    plain_vis, plain_irr, _, _, _ = check(gpu, scene, lights, p, base, samples, (samples, nl, "nobody skipped"))
    per = items_per_wave
    cases = {"first of a wave": [0, 2 * per], "last of a wave": [per - 1, 3 * per - 1], "a whole wave's worth": list(range(per, 2 * per)),
             "the last points": list(range(n - 3, n)), "alone in a wave": [per + 1], "every point": list(range(n))}
    for what, which in cases.items():
        nrm = base.copy()
        nrm[which] = 0.0
        nrm[which[0]] = [-0.0, 0.0, -0.0]
        vis, irr, _, cast, st = check(gpu, scene, lights, p, nrm, samples, (samples, nl, what))
        mates = np.ones(n, bool)
        mates[which] = False
        assert not vis[which].any() and not irr[which].any() and not cast[which].any(), (samples, nl, what)
        assert same(vis[mates], plain_vis[mates]) and same(irr[mates], plain_irr[mates]), (samples, nl, what)
        if what == "every point":
            assert counters(st) == (0, 0, 0, 0)


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_spoilers_permutations_and_the_order_of_the_lights(gpu, oracle, accel):
    scene, lights, _ = install(gpu, "golden")
    p, nrm = DL.points_of(oracle, "golden")
    n = 256                                                             # at 16 samples and 2 lights: 128 waves of 4 items, 2 points each
    p, nrm = np.ascontiguousarray(p[:n]), np.ascontiguousarray(nrm[:n])
    want_vis, want_irr = (a[:n] for a in DL.reference(oracle, "golden")[:2])
    with Mode(gpu, "tree forced" if accel == R.ACCEL_BVH else "brute") as a:
        vis, irr, v, cast, _ = check(gpu, scene, lights, p, nrm, 16, "unspoiled", accel=a)
        assert same(vis, want_vis) and same(irr, want_irr) and mixed(v, cast, 16)
        for what in ("a NaN point", "a point beyond 2^60", "a NaN normal"):
            sp, sn = p.copy(), nrm.copy()
            pos = np.arange(0, n, 2) + (np.arange(n // 2) * 7) % 2      # one per wave, its place in the wave varying
            if what == "a NaN point":
                sp[pos, 1] = np.nan
            elif what == "a point beyond 2^60":
                sp[pos, 0] = F(2.0 ** 61)
            else:
                sn[pos, 2] = np.nan
            got_vis, got_irr, _, got_cast, _ = check(gpu, scene, lights, sp, sn, 16, what, accel=a)   # the spoilers answer what the composition answers
            mates = np.ones(n, bool)
            mates[pos] = False
            assert same(got_vis[mates], want_vis[mates]) and same(got_irr[mates], want_irr[mates]), (what, "the mate of every wave keeps the oracle's answer")
            if what != "a point beyond 2^60":
                assert not got_cast[pos].any() and not got_vis[pos].any(), (what, "a NaN fails the comparison: nothing is cast")
        for perm in (np.arange(n)[::-1], np.random.default_rng(5).permutation(n)):
            got_vis, _, v, cast, _ = check(gpu, scene, lights, p[perm], nrm[perm], 16, "permuted", accel=a)   # (the index is the position: recomputed)
            assert mixed(v, cast, 16) and not same(got_vis, want_vis[perm])
        gpu.set_lights(lights[::-1])                                    # the light's place in the list is part of its stream
        got_vis, _, v, cast, _ = check(gpu, scene, lights[::-1], p, nrm, 16, "the list reversed", accel=a)
        assert mixed(v, cast, 16) and not same(got_vis[:, ::-1], want_vis)
        assert abs(float(got_vis[:, ::-1].mean()) - float(want_vis.mean())) < 0.05, "the same lights seen by other samples"


# ---- direct_light_map equals its definition ------------------------------------------------------------------------------------------------------
def definition(r, cam, width, height, mint, maxt, samples, seed=0, accel=R.ACCEL_BVH, time=0.0, lo=LO, hi=HI):
    """rtw_ctx_direct_light_map by its text: depth_map, then the points o + d * depth and the faced normals in numpy (one f32 rounding per
    operation; map_points of the ambient-occlusion tests), then direct_light; (vis, irr, depth, ids, normals, (segments, counters...))."""
    p, faced, _, depth, ids, nrm, dst = map_points(r, cam, width, height, mint, maxt, time, accel)
    vis, irr, lst = r.direct_light(p, faced, samples, lo=lo, hi=hi, seed=seed, time=time, accel=accel)
    nl = vis.shape[1]
    stats = tuple(a + b for a, b in zip(counters(dst), counters(lst)))
    return vis.reshape(height, width, nl), irr.reshape(height, width, nl), depth, ids, nrm, stats


def check_map(r, cam, width, height, what, mint=MINT, maxt=MAXT, samples=16, accel=R.ACCEL_BVH, seed=0, time=0.0, lo=LO, hi=HI):
    want_vis, want_irr, depth, ids, nrm, stats = definition(r, cam, width, height, mint, maxt, samples, seed, accel, time, lo, hi)
    kw = dict(lo=lo, hi=hi, seed=seed, time=time, accel=accel)
    vis, irr, d, i, n, st = r.direct_light_map(cam, width, height, mint, maxt, samples, depth=True, ids=True, normals=True, **kw)
    assert vis.shape == want_vis.shape and same(vis, want_vis) and same(irr, want_irr), (what, "vis and irr against the definition")
    assert same(d, depth) and same(i, ids) and same(n, nrm), (what, "depth, ids and normals are depth_map's bytes")
    assert counters(st) == stats and st.kernel_ms > 0.0, (what, "counters", counters(st), stats)
    assert not vis[ids < 0].any() and not irr[ids < 0].any(), (what, "a miss pixel is skipped")
    alone, st0 = r.direct_light_map(cam, width, height, mint, maxt, samples, irradiance=False, **kw)      # nothing optional asked for
    assert same(alone, vis) and st0.segments == st.segments
    return vis, irr, ids


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_the_map_equals_its_definition(gpu, accel):
    gpu.set_scene(geom_scene())
    gpu.set_lights(DL.GEOM_LIGHTS)
    width, height = 96, 64
    vis, irr, ids = check_map(gpu, depth_camera("geom", width, height), width, height, "geom 96 x 64", accel=accel)
    hit = ids >= 0
    assert 0.2 <= hit.mean() <= 0.8 and len(np.unique(vis[hit])) >= 8 and 0.0 < vis[hit].mean() < 1.0 and irr.max() > 0.0


@pytest.mark.parametrize("width,height", [(1, 1), (5, 3), (65, 2)])
def test_the_map_of_small_and_narrow_images(gpu, width, height):
    gpu.set_scene(geom_scene())
    gpu.set_lights(DL.GEOM_LIGHTS)
    check_map(gpu, depth_camera("geom", width, height), width, height, (width, height))


def test_the_map_of_the_sky(gpu):
    gpu.set_scene(geom_scene())
    gpu.set_lights(DL.GEOM_LIGHTS)
    width, height = 40, 24
    sky = R.camera2_new(width / height, (0.0, 0.3, 1.5), (0.0, 1.0, 0.0), (0.0, 0.1, 1.0), 75.0, 0.0)             # away from everything
    vis, irr, ids = check_map(gpu, sky, width, height, "sky")
    assert (ids < 0).all() and not vis.any() and not irr.any()
    assert gpu.direct_light_map(sky, width, height, MINT, MAXT)[-1].segments == width * height


# ---- each group alone as the occluder ------------------------------------------------------------------------------------------------------------
CEILING = ((-1.5, 3.5, -4.5), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0))        # a quad light above geom_scene()'s objects
LAMP = ((0.0, 3.5, -3.0), 0.5)                                        # ... and a sphere light at the same place


def group_with_a_light(group):
    """OC.sub_scene(group) and a light that belongs to another group: (Scene, lights)."""
    g = OC.sub_scene(group)
    pool = lambda arr, k: [type(arr[0]).from_buffer_copy(arr[i]) for i in range(k)]
    if group == "quads":
        scene = R.Scene([R.Sphere.new(LAMP[0], LAMP[1], (1.0, 1.0, 1.0), R.SCATTER_M)])
        scene._install_geom(pool(g._quads, g.pod.n_quads), [], [], [])
        return scene, [(R.LIGHT_SPHERE, 0)]
    scene = R.Scene(pool(g._spheres, g.n_spheres), triangles=[g.triangles[i] for i in range(g.n_triangles)] if g.n_triangles else None)
    scene._install_geom([R.Quad.new(*CEILING).pod], pool(g._instances, g.pod.n_instances), pool(g._inst_spheres, g.pod.n_inst_spheres),
                        pool(g._inst_quads, g.pod.n_inst_quads))
    return scene, [(R.LIGHT_QUAD, 0)]


def upward(p, n):
    """Normals with the y component turned towards the lights above."""
    n = n.copy()
    n[:, 1] = np.abs(n[:, 1])
    return p, n


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
@pytest.mark.parametrize("group", OC.GROUPS)
def test_each_group_alone(gpu, group, accel):
    scene, lights = group_with_a_light(group)
    _, _, rays, _, mint, maxt = OC.scene_case(group)
    gpu.set_scene(scene)
    gpu.set_lights(lights)
    with Mode(gpu, "tree forced" if accel == R.ACCEL_BVH else "brute") as a:
        p, n = upward(*hit_points(gpu, rays, mint, maxt))
        assert len(p) >= 32, group
        q, m = upward(*AO.random_points(256, 11))                       # ... and points in the air about the objects
        q[:, 1] -= 1.5                                                  # (below them)
        p, n = np.concatenate([p, q]), np.concatenate([n, m])
        _, _, v, cast, st = check(gpu, scene, lights, p, n, 16, (group, accel), accel=a)
    assert 0 < v.sum() < cast.sum(), (group, "one outcome only", int(v.sum()), int(cast.sum()))
    if group in ("quads", "triangles"):
        assert st.quad_tests > 0


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_quaternion_instances(gpu, accel):
    g = QC.golden()
    t = np.asarray(g["translation"], np.float64)
    lamp = {"origin": [float(x) for x in t + (-1.0, 2.5, -1.0)], "u": [2.0, 0.0, 0.0], "v": [0.0, 0.0, 2.0], "material": "lambertian",
            "color": [1.0, 1.0, 1.0], "emitted": [4.0, 4.0, 4.0]}
    bulb = {"origin": [float(x) for x in t + (2.0, 1.0, 1.0)], "radius": 0.3, "material": "lambertian", "color": [1.0, 1.0, 1.0],
            "emitted": [4.0, 4.0, 4.0]}
    lights = [(R.LIGHT_QUAD, 0), (R.LIGHT_SPHERE, 0)]
    fx = QC.fixture_scene(g, spheres=[bulb], quads=[lamp], lights=lights)             # the rotated box under a quad light, a sphere light beside it
    fx.install(gpu)
    scene = fx.scene
    cam = QC.camera(g, 40, 30)
    p, n = hit_points(gpu, R.depth_rays(cam, 40, 30), g["mint"], g["maxt"])
    assert len(p) >= 100
    q = (np.asarray(g["translation"]) + np.random.default_rng(11).uniform(-1.5, 1.5, (256, 3))).astype(F)       # ... and points in the air about the box
    p, n = np.concatenate([p, q]), np.concatenate([n, AO.random_points(256, 11)[1]])
    _, _, v, cast, _ = check(gpu, scene, lights, p, n, 16, "the golden rotation scene", accel=accel)
    assert mixed(v, cast, 16)
    check_map(gpu, cam, 40, 30, "the golden rotation scene", mint=g["mint"], maxt=g["maxt"], accel=accel)


def mesh_scene(tris):
    """A mesh under the ceiling light: (Scene, lights)."""
    scene = R.Scene((), quads=[R.Quad.new((-12.0, 6.0, -12.0), (24.0, 0.0, 0.0), (0.0, 0.0, 24.0))], triangles=tris)
    return scene, [(R.LIGHT_QUAD, 0)]


def install_placements_under_a_light(r, pods, pl):
    scene, lights = mesh_scene(None)
    r.set_scene(scene)
    r.set_triangles(list(pods))
    r.set_mesh_instances(pl)
    r.set_lights(lights)
    return scene, lights


def test_a_mesh_and_placements_as_occluders(gpu):
    pods, pl, rays = OC.placement_case("grid8")
    scene, lights = install_placements_under_a_light(gpu, pods, pl)
    p, n = upward(*hit_points(gpu, rays, MI.MINT, MI.MAXT))
    assert len(p) >= 100
    for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
        _, _, v, cast, st = check(gpu, scene, lights, p, n, 16, ("grid8", accel), accel=accel)
        assert mixed(v, cast, 16) and (st.node_tests > 0) == (accel == R.ACCEL_BVH)


def test_a_refit_and_a_move_are_seen_by_the_next_call(ctx):  # noqa: F811
    # a refit: points on the deformed terrain, shaded by its own waves
    vtx, f, _, _ = RC.mesh("terrain12")
    w = RC.sine_wave(vtx, f)
    scene_w, lights = mesh_scene(RC.triangles_of(w, f))
    ctx.set_scene(scene_w)
    p, n = upward(*hit_points(ctx, OC.mesh_rays(w, f), MI.MINT, MI.MAXT))
    scene_v, _ = mesh_scene(RC.triangles_of(vtx, f))
    ctx.set_scene(scene_v)
    ctx.set_lights(lights)
    before = ctx.direct_light(p, n, 16)[0]
    assert ctx.refit_triangles(R.mesh_ouv(w, f)) == 0
    after = {accel: check(ctx, scene_w, lights, p, n, 16, ("after the refit", accel), accel=accel)[:2] for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE)}
    with R.Renderer(0) as other:
        other.set_scene(scene_w)
        other.set_lights(lights)
        want_vis, want_irr, _ = other.direct_light(p, n, 16)
    for accel in after:
        assert same(after[accel][0], want_vis) and same(after[accel][1], want_irr), ("a fresh context with the deformed mesh", accel)
    assert not same(want_vis, before) and 0.0 < want_vis.mean() < 1.0
    # a move
    pods, pl, rays = OC.placement_case("grid8")
    moved = MM.turn_and_shift(MM.as_array(pl))
    scene, lights = install_placements_under_a_light(ctx, pods, pl)
    p, n = upward(*hit_points(ctx, rays, MI.MINT, MI.MAXT))
    before = ctx.direct_light(p, n, 16)[0]
    assert ctx.move_mesh_instances(moved) == 0
    after = {accel: check(ctx, scene, lights, p, n, 16, ("after the move", accel), accel=accel)[:2] for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE)}
    with R.Renderer(0) as other:
        install_placements_under_a_light(other, pods, MM.as_list(moved))
        want_vis, want_irr, _ = other.direct_light(p, n, 16)
    for accel in after:
        assert same(after[accel][0], want_vis) and same(after[accel][1], want_irr), ("a fresh context with the moved placements", accel)
    assert not same(want_vis, before)


# ---- memory and streams ----------------------------------------------------------------------------------------------------------------------------
def test_torch_tensors_and_the_producers_of_them(ctx, oracle, torch, cycles_per_ms):  # noqa: F811
    scene, lights, _ = install(ctx, "golden")
    p, n = DL.points_of(oracle, "golden")
    want_vis, want_irr, _, want_cast = DL.reference(oracle, "golden")
    d_p, d_n = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(n).to("cuda:0")
    torch.cuda.synchronize()
    vis, irr, st = ctx.direct_light(d_p, d_n, DL.SAMPLES)               # outputs allocated; on the context's own stream
    assert vis.dtype == torch.float32 and vis.is_cuda and tuple(vis.shape) == want_vis.shape
    assert same(vis.cpu().numpy(), want_vis) and same(irr.cpu().numpy(), want_irr) and st.segments == int(want_cast.sum())
    h_vis, h_irr, _ = ctx.direct_light(p, n, DL.SAMPLES)
    assert same(h_vis, want_vis) and same(h_irr, want_irr), "numpy in and out"
    only, _ = ctx.direct_light(d_p, d_n, DL.SAMPLES, irradiance=False)
    assert same(only.cpu().numpy(), want_vis)
    with pytest.raises(ValueError):
        ctx.direct_light(p, n, DL.SAMPLES, out_vis=np.zeros(want_vis.shape, F))
    with pytest.raises(ValueError):
        ctx.direct_light(d_p, n, DL.SAMPLES)
    with pytest.raises(ValueError):
        ctx.direct_light(d_p, d_n, DL.SAMPLES, out_vis=torch.zeros(want_vis.shape, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        ctx.direct_light(d_p, d_n, DL.SAMPLES, out_irr=torch.zeros(len(p), dtype=torch.float32, device="cuda:0"))
    # behind a delayed producer on torch's default stream: stale normals that face away from everything (nothing is cast), stale outputs
    away_n = np.zeros_like(n)
    assert not ctx.direct_light(p, away_n, DL.SAMPLES)[0].any() and want_vis.max() > 0.0
    hz = Hazard(torch, cycles_per_ms)
    t_p, t_n = hz.input(p), hz.input(n, stale=away_n)
    t_vis = hz.output(want_vis.shape, torch.float32, 9.0, 7.0)
    t_irr = hz.output(want_vis.shape, torch.float32, 9.0, 7.0)
    (got_vis, got_irr), (_, _, st) = hz.run(ctx, "torch-default", lambda: ctx.direct_light(t_p, t_n, DL.SAMPLES, out_vis=t_vis, out_irr=t_irr))
    assert same(got_vis, want_vis) and same(got_irr, want_irr) and st.segments == int(want_cast.sum())


STAGING_LIGHTS = FIELD_LIGHTS[:3]


def staging_entries():
    points, normals = AO.random_points(N, 11)
    normals[::2, 1] = np.abs(normals[::2, 1])
    normals[5] = 0.0                                        # a point that casts no ray
    cam = depth_camera("geom", W, H)
    L, bvh, nl = R.lib(), R.ACCEL_BVH, len(STAGING_LIGHTS)
    e = {}
    for s in (4, 128):
        e[f"direct_light {s}"] = Entry((points, normals), ((N * nl, F, False), (N * nl, F, True)), lambda h, i, o, st, s=s: L.rtw_ctx_direct_light(
            h, i[0], i[1], N, s, 7, 0.0, LO, HI, bvh, o[0], o[1], st))
    e["direct_light_map 4"] = Entry((), ((W * H * nl, F, False), (W * H * nl, F, True), (W * H, F, True), (W * H, np.int32, True), (3 * W * H, F, True)),
                                    lambda h, i, o, st: L.rtw_ctx_direct_light_map(h, C.byref(cam), W, H, 0.0, MINT, MAXT, 4, 7, LO, HI, bvh, o[0], o[1], o[2],
                                                                                   o[3], o[4], st))
    return e


@pytest.mark.parametrize("name", ["direct_light 4", "direct_light 128", "direct_light_map 4"])
def test_every_pointer_host_or_device_or_absent(ctx, torch, name):  # noqa: F811
    """As tests/test_gpu_query_staging.py holds the other passes: every caller pointer host or device, every optional output absent as well;
    the answers and counters are those of the all-host call on ANOTHER context, every tail is untouched, every device input unchanged."""
    assert TAIL > 0
    scene, entry = QE.field_scene(), staging_entries()[name]
    with R.Renderer(0) as other:
        other.set_scene(scene)
        other.set_lights(STAGING_LIGHTS)
        want = {kinds: run(torch, other, entry, kinds, name) for kinds in {entry.all_host(k) for k in entry.kinds()}}
        rays = np.ascontiguousarray(OC.scene_case("field")[2][:N])
        occ_want, occ_st = other.scene_occluded(rays, MINT, OC.FIELD_MAXT)
    full = want[("host",) * (len(entry.ins) + len(entry.outs))]
    assert 0.0 < full[0][0].mean() < 1.0 and full[0][1].max() > 0.0 and full[1][0] > 0, "both outcomes"
    ctx.set_scene(scene)
    ctx.set_lights(STAGING_LIGHTS)
    for kinds in entry.kinds():
        assert_answer(run(torch, ctx, entry, kinds, name), want[entry.all_host(kinds)], (name, kinds))
    occ, st = ctx.scene_occluded(rays, MINT, OC.FIELD_MAXT)             # no temporary and no counter of the pass reaches the next
    assert same(occ, occ_want) and counters(st) == counters(occ_st)


def test_lifecycle_and_statuses(ctx, oracle):  # noqa: F811
    L = R.lib()
    scene, lights, _, _, _, _, _ = DL.case("geom")
    p, n = DL.points_of(oracle, "geom")
    p4, n4 = np.ascontiguousarray(p[:4]), np.ascontiguousarray(n[:4])
    vis, irr = np.full(8, 7.0, F), np.full(8, 7.0, F)
    cam = depth_camera("geom", 2, 2)
    pp, nn, vv, ii = p4.ctypes.data, n4.ctypes.data, vis.ctypes.data, irr.ctypes.data

    def direct(h, points=pp, normals=nn, count=4, samples=16, accel=R.ACCEL_BVH, dst=vv, dst_irr=ii):
        return L.rtw_ctx_direct_light(h, points, normals, count, samples, 0, 0.0, LO, HI, accel, dst, dst_irr, None)

    def direct_map(h, camera=C.byref(cam), w=2, hh=2, samples=16, accel=R.ACCEL_BVH, dst=vv):
        return L.rtw_ctx_direct_light_map(h, camera, w, hh, 0.0, MINT, MAXT, samples, 0, LO, HI, accel, dst, ii, None, None, None, None)

    with R.Renderer(0) as other:
        assert direct(other._h) == E_NO_SCENE and direct_map(other._h) == E_NO_SCENE and other.light_count() == 0
        with pytest.raises(R.RtwError):
            other.direct_light(p4, n4)
        other.set_scene(scene)
        assert direct(other._h) == E_INVALID and direct_map(other._h) == E_INVALID, "no lights set"
        other.set_lights(lights)
        second = other.direct_light(p, n, 16)[:2]
        second_map = other.direct_light_map(cam, 2, 2, MINT, MAXT, 16)[:2]
        other.set_scene(scene)                                          # a new scene clears the lights
        assert other.light_count() == 0 and direct(other._h) == E_INVALID
    ctx.set_scene(scene)
    ctx.set_lights(lights)
    for bad in (direct(None), direct(ctx._h, points=None), direct(ctx._h, normals=None), direct(ctx._h, dst=None), direct(ctx._h, count=0),
                direct(ctx._h, accel=2), direct(ctx._h, samples=0), direct(ctx._h, samples=3), direct(ctx._h, samples=2048),
                direct(ctx._h, count=2 ** 31, samples=1024), direct(ctx._h, count=2 ** 31, samples=1),
                direct_map(None), direct_map(ctx._h, camera=None), direct_map(ctx._h, dst=None), direct_map(ctx._h, w=0), direct_map(ctx._h, hh=0),
                direct_map(ctx._h, accel=2), direct_map(ctx._h, samples=5), direct_map(ctx._h, w=65536, hh=65535, samples=1),
                direct_map(ctx._h, w=65536, hh=65536)):
        assert bad == E_INVALID
    ctx.set_lights(None)
    assert direct(ctx._h) == E_INVALID and direct_map(ctx._h) == E_INVALID, "the lights were cleared"
    assert (vis == 7.0).all() and (irr == 7.0).all(), "a refused call wrote"
    ctx.set_lights(lights)
    assert direct(ctx._h) == R.RTW_OK                                   # (stats may be NULL)
    first = ctx.direct_light(p, n, 16)[:2]
    want = DL.reference(oracle, "geom")[:2]
    assert same(first[0], second[0]) and same(first[1], second[1]) and same(first[0], want[0]) and same(first[1], want[1])
    assert same(first[0][:4].reshape(-1), vis) and same(first[1][:4].reshape(-1), irr)
    assert direct_map(ctx._h) == R.RTW_OK and same(vis.reshape(2, 2, 2), second_map[0]) and same(irr.reshape(2, 2, 2), second_map[1])
