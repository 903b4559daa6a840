"""rtw_ctx_ambient_occlusion, rtw_ctx_ao_map, rtw_ctx_direct_light and rtw_ctx_direct_light_map on the MI355X at the arguments their own
tests leave at one value: other seeds, ranges whose ends lie on a hit, times at and outside the shutter, NaN arguments, lights that move and
lights and points whose geometry leaves the plain arithmetic, the association of the weights' sum, and the context's state between calls.

Every comparison has the same parts: the outputs equal the composition's on the same context on the bits (`check` / `check_map` of
tests/test_gpu_ao.py and tests/test_gpu_direct_light.py), the counters equal rtw_ctx_scene_occluded's over the same cast rays, and where the
CPU oracle defines the answer the outputs equal the oracle's.  The inputs and references are tests/any_hit_edges_common.py's;
tests/test_any_hit_edges_cpu.py proves on the CPU that each reaches the edge it is named for."""
import numpy as np
import pytest

import rtw_amd as R
from tests import any_hit_edges_common as AE
from tests import ao_common as AO
from tests import direct_light_common as DL
from tests import query_edges_common as QE
from tests import test_gpu_ao as TA
from tests import test_gpu_direct_light as TD
from tests.test_gpu_occluded import Mode
from tests.test_gpu_scene_hits import MAXT, MINT, TIME, depth_camera, oracle_hits
from tests.test_gpu_stream_order import same

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID = -1
BOTH = ("brute", "tree forced")
SIZES = sorted(AE.POINTS_AT.items())                       # (samples, points): the ONE build and the round loop


def install_ao(r, oracle, name):
    scene, (t0, t1), time, p, n, radius = AE.ao_set(oracle, name)
    r.set_scene(scene, t0, t1)
    return scene, time, p, n, radius


def install_dl(r, oracle, name):
    scene, lights, (t0, t1), time, p, n = AE.dl_set(oracle, name)
    r.set_scene(scene, t0, t1)
    r.set_lights(lights)
    return scene, lights, time, p, n


def first(a, n):
    return np.ascontiguousarray(a[:n])


def direct_against(r, oracle, name, n_points, samples, what, **kw):
    """TD.check of the first n_points of dl_set(name), then the oracle's answer for the same arguments: (vis, irr, v, cast, RtwStats)."""
    scene, lights, _, time, p, n = AE.dl_set(oracle, name)
    kw.setdefault("time", time)
    vis, irr, v, cast, st = TD.check(r, scene, lights, first(p, n_points), first(n, n_points), samples, what, **kw)
    want = AE.dl_oracle(oracle, name, n_points, samples, kw.get("seed", 0), kw["time"], kw.get("lo", DL.LO), kw.get("hi", DL.HI))
    assert np.array_equal(v, want[2]) and np.array_equal(cast, want[3]) and same(vis, want[0]) and same(irr, want[1]), (what, "against the oracle")
    return vis, irr, v, cast, st


# ---- 1. seeds -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("samples,n", SIZES)
@pytest.mark.parametrize("name", ["field", "forty"])
def test_ambient_occlusion_under_other_seeds(gpu, oracle, name, samples, n, mode):
    scene, time, p, nrm, radius = install_ao(gpu, oracle, name)
    p, nrm = first(p, n), first(nrm, n)
    answers = {}
    with Mode(gpu, mode) as accel:
        for seed in (0,) + AE.SEEDS:
            ao, counts, _ = TA.check(gpu, p, nrm, samples, radius, (name, samples, mode, seed), seed=seed, time=time, accel=accel)
            want_counts, want = AE.ao_oracle(oracle, name, n, samples, seed)
            assert np.array_equal(counts, want_counts) and same(ao, want), (name, samples, mode, hex(seed), "against the oracle")
            answers[seed] = ao
        wrapped, _ = gpu.ambient_occlusion(p, nrm, samples, radius, seed=2 ** 32 + 5, time=time, accel=accel)
        assert same(wrapped, gpu.ambient_occlusion(p, nrm, samples, radius, seed=5, time=time, accel=accel)[0]), "the seed is 32 bits"
        assert not same(wrapped, answers[0])
    seeds = list(answers)
    assert all(not same(answers[a], answers[b]) for i, a in enumerate(seeds) for b in seeds[:i]), "two seeds, one answer"
    if samples == AO.SAMPLES:
        assert same(answers[0], AO.reference(oracle, name)[1][:n]), "seed 0 is the committed reference"


@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("samples,n", SIZES)
@pytest.mark.parametrize("name", ["golden", "forty"])
def test_direct_light_under_other_seeds(gpu, oracle, name, samples, n, mode):
    scene, lights, time, p, nrm = install_dl(gpu, oracle, name)
    answers = {}
    with Mode(gpu, mode) as accel:
        for seed in (0,) + AE.SEEDS:
            answers[seed] = direct_against(gpu, oracle, name, n, samples, (name, samples, mode, hex(seed)), seed=seed, accel=accel)[:2]
        wrapped = gpu.direct_light(first(p, n), first(nrm, n), samples, seed=2 ** 32 + 5, time=time, accel=accel)
        plain = gpu.direct_light(first(p, n), first(nrm, n), samples, seed=5, time=time, accel=accel)
        assert same(wrapped[0], plain[0]) and same(wrapped[1], plain[1]) and not same(wrapped[0], answers[0][0]), "the seed is 32 bits"
    seeds = list(answers)
    for k in (0, 1):
        assert all(not same(answers[a][k], answers[b][k]) for i, a in enumerate(seeds) for b in seeds[:i]), ("two seeds, one answer", k)
    if samples == DL.SAMPLES:
        want = DL.reference(oracle, name)
        assert same(answers[0][0], first(want[0], n)) and same(answers[0][1], first(want[1], n)), "seed 0 is the committed reference"


def ao_map_oracle(r, oracle, scene, cam, width, height, mint, maxt, samples, radius, ao_mint, seed, time, accel):
    """The oracle over the host rule's rays from the points the map shades (TA.map_points): ao [height][width]."""
    p, faced = TA.map_points(r, cam, width, height, mint, maxt, time, accel)[:2]
    skip = AO.skipped(faced)
    counts = np.zeros(len(p), np.int64)
    rays = R.ao_rays(p, faced, samples, seed)
    occ = oracle_hits(oracle, scene, np.ascontiguousarray(rays[~skip]).reshape(-1, 6), time, ao_mint, radius)[1] >= 0
    counts[~skip] = occ.reshape(-1, samples).sum(axis=1)
    return AO.ao_of(counts, samples, skip).reshape(height, width)


def direct_map_oracle(r, oracle, scene, lights, cam, width, height, mint, maxt, samples, seed, time, lo, hi, accel):
    p, faced = TA.map_points(r, cam, width, height, mint, maxt, time, accel)[:2]
    vis, irr = AE.dl_answer(oracle, scene, lights, p, faced, samples, seed, time, lo, hi)[:2]
    return vis.reshape(height, width, len(lights)), irr.reshape(height, width, len(lights))


@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("samples,width,height", AE.MAP_SIZES)
def test_the_camera_forms_under_other_seeds(gpu, oracle, samples, width, height, mode):
    scene, lights = AO.case("geom")[0], DL.GEOM_LIGHTS
    cam = depth_camera("geom", width, height)
    gpu.set_scene(scene)
    gpu.set_lights(lights)
    aos, viss = {}, {}
    with Mode(gpu, mode) as accel:
        for seed in (0,) + AE.SEEDS:
            what = (samples, mode, hex(seed))
            ao, ids, _ = TA.check_map(gpu, cam, width, height, what, samples=samples, radius=5.0, accel=accel, seed=seed)
            assert same(ao, ao_map_oracle(gpu, oracle, scene, cam, width, height, MINT, MAXT, samples, 5.0, AO.AO_MINT, seed, 0.0, accel)), what
            vis, irr, _ = TD.check_map(gpu, cam, width, height, what, samples=samples, accel=accel, seed=seed)
            want = direct_map_oracle(gpu, oracle, scene, lights, cam, width, height, MINT, MAXT, samples, seed, 0.0, DL.LO, DL.HI, accel)
            assert same(vis, want[0]) and same(irr, want[1]), what
            aos[seed], viss[seed] = ao, vis
        assert (ids >= 0).sum() >= 8
        wrapped = gpu.ao_map(cam, width, height, MINT, MAXT, samples, 5.0, seed=2 ** 32 + 5, accel=accel)[0]
        assert same(wrapped, gpu.ao_map(cam, width, height, MINT, MAXT, samples, 5.0, seed=5, accel=accel)[0]) and not same(wrapped, aos[0])
        wrapped = gpu.direct_light_map(cam, width, height, MINT, MAXT, samples, seed=2 ** 32 + 5, accel=accel)[0]
        assert same(wrapped, gpu.direct_light_map(cam, width, height, MINT, MAXT, samples, seed=5, accel=accel)[0]) and not same(wrapped, viss[0])
        # ... and with another range than the default for the second pass: it reaches the kernel, and the answers move
        what, (lo, hi) = (samples, mode, "another range"), AE.MAP_RANGE
        ao, _, _ = TA.check_map(gpu, cam, width, height, what, samples=samples, radius=AE.MAP_RADIUS, accel=accel, ao_mint=lo, seed=1)
        assert same(ao, ao_map_oracle(gpu, oracle, scene, cam, width, height, MINT, MAXT, samples, AE.MAP_RADIUS, lo, 1, 0.0, accel)), what
        vis, irr, _ = TD.check_map(gpu, cam, width, height, what, samples=samples, accel=accel, seed=1, lo=lo, hi=hi)
        want = direct_map_oracle(gpu, oracle, scene, lights, cam, width, height, MINT, MAXT, samples, 1, 0.0, lo, hi, accel)
        assert same(vis, want[0]) and same(irr, want[1]) and not same(ao, aos[1]) and not same(vis, viss[1]), what
    seeds = list(aos)
    assert all(not same(aos[a], aos[b]) and not same(viss[a], viss[b]) for i, a in enumerate(seeds) for b in seeds[:i]), "two seeds, one answer"


# ---- 2. ranges ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("samples,n", [(16, 64), (128, 16)])
def test_direct_light_turns_at_an_exact_edge(gpu, oracle, samples, n, mode):
    """Every segment of the flat scene meets the blocker's plane at t == 0.5 exactly: with 0.5 as either end of the range the blocked ones
    are occluded, one ulp outside none is."""
    install_dl(gpu, oracle, "flat")
    v = {}
    with Mode(gpu, mode) as accel:
        for what, (lo, hi) in AE.FLAT_RANGES.items():
            _, _, v[what], cast, st = direct_against(gpu, oracle, "flat", n, samples, (what, samples, mode), lo=lo, hi=hi, accel=accel)
            assert cast.sum() == n * samples == st.segments
    for what in AE.FLAT_CLOSED:
        assert 4 * (cast.sum() - v[what].sum()) >= cast.sum(), what
    for what in AE.FLAT_OPEN:
        assert v[what].sum() == cast.sum(), what
    assert not v["hi = 1"].any(), "at hi = 1 the light's own plane stops every segment"


@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("samples,n", SIZES)
def test_direct_light_about_the_sphere_lights_own_surface(gpu, oracle, samples, n, mode):
    """hi = 1 - 1e-3 leaves the light's surface out, 1 + 1e-3 takes it in; at 1.0 the rounding of each root decides, and the oracle says
    which way."""
    install_dl(gpu, oracle, "surface")
    with Mode(gpu, mode) as accel:
        v = [direct_against(gpu, oracle, "surface", n, samples, (hi, samples, mode), hi=hi, accel=accel)[2] for hi in AE.SURFACE_HI]
    assert v[0].sum() > v[1].sum() > v[2].sum()


@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("name", ["field", "forty"])
def test_ambient_occlusion_range_edges(gpu, oracle, name, mode):
    """The t of a ray's only hit as the radius and as mint, and the next f32 outside: the ray's bit turns, its point's count moves by one."""
    scene, time, p, nrm, radius = install_ao(gpu, oracle, name)
    p, nrm = first(p, AE.AO_EDGE_POINTS), first(nrm, AE.AO_EDGE_POINTS)
    flips = 0
    with Mode(gpu, mode) as accel:
        for i, k, t, cases in AE.ao_edge_reference(oracle, name):
            got = []
            for mint, rad, bit, count in cases:
                ao, counts, _ = TA.check(gpu, p, nrm, 16, rad, (name, mode, i, k, mint, rad), mint=mint, time=time, accel=accel)
                assert counts[i] == count and ao[i] == AO.ao_of(count, 16), (name, mode, i, k, mint, rad, "against the oracle")
                got.append(int(counts[i]))
            bits = [c[2] for c in cases]
            if bits == [True, False, True, False]:
                assert got[0] - got[1] == 1 and got[2] - got[3] == 1, (name, mode, i, k, got)
                flips += 1
    assert 2 * flips >= AE.AO_EDGE_RAYS


@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("samples,n", [(16, 65), (128, 17)])
@pytest.mark.parametrize("name", ["field", "forty"])
def test_ambient_occlusion_range_classes(gpu, oracle, name, samples, n, mode):
    scene, time, p, nrm, radius = install_ao(gpu, oracle, name)
    p, nrm = first(p, n), first(nrm, n)
    with Mode(gpu, mode) as accel:
        for cls, (mint, rad) in AE.AO_CLASSES.items():
            rad = radius if rad is None else rad
            ao, counts, st = TA.check(gpu, p, nrm, samples, rad, (name, cls, samples, mode), mint=mint, time=time, accel=accel)
            want_counts, want = AE.ao_oracle(oracle, name, n, samples, 0, None, mint, rad)
            assert np.array_equal(counts, want_counts) and same(ao, want), (name, cls, samples, mode, "against the oracle")
            assert st.segments == samples * n, "the rays are cast and counted whatever the range"
            if cls == "mint > radius":
                assert (ao == 1.0).all() and not counts.any()
            if cls.startswith("radius =") and name == "forty":
                # a scene of spheres alone: an unbounded radius is no whole-call fall-back (only a NaN or a time outside the shutter is,
                # query_uses_tree), and q_ray_ordinary reads the scene's span and the ray, not the range: the forced tree is walked
                print(f"\n[edges] forty, {cls}, {samples} samples, {mode}: node visits {st.node_tests}, sphere tests {st.sphere_tests}")
                assert (st.node_tests > 0) == (mode == "tree forced"), (cls, mode, st.node_tests)


@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("cls", list(QE.RANGES))
def test_ambient_occlusion_over_the_query_range_classes(gpu, oracle, cls, mode):
    mint, maxt = QE.RANGES[cls]
    scene, time, p, nrm, _ = install_ao(gpu, oracle, "field")
    for samples, n in ((16, 129), (128, 17)):
        with Mode(gpu, mode) as accel:
            ao, counts, _ = TA.check(gpu, first(p, n), first(nrm, n), samples, maxt, (cls, samples, mode), mint=mint, accel=accel)
        want_counts, want = AE.ao_oracle(oracle, "field", n, samples, 0, None, mint, maxt)
        assert np.array_equal(counts, want_counts) and same(ao, want), (cls, samples, mode, "against the oracle")


# ---- 3. whole-call fall-backs and time ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples,n", [(16, AE.FALLBACK_POINTS), (128, 17)])
def test_ambient_occlusion_whole_call_fallbacks(gpu, oracle, samples, n):
    scene, time, p, nrm, radius = install_ao(gpu, oracle, "forty")
    p, nrm = first(p, n), first(nrm, n)
    with Mode(gpu, "tree forced") as accel:
        for what, (tm, mint, rad) in {**AE.INSIDE, **AE.FALLBACKS}.items():
            mint, rad = AO.AO_MINT if mint is None else mint, radius if rad is None else rad
            ao, counts, st = TA.check(gpu, p, nrm, samples, rad, (what, samples), mint=mint, time=tm, accel=accel)
            assert (st.node_tests > 0) == (what in AE.INSIDE), (what, st.node_tests)
            if "NaN" not in what:
                want_counts, want = AE.ao_oracle(oracle, "forty", n, samples, 0, tm, mint, rad)
                assert np.array_equal(counts, want_counts) and same(ao, want), (what, samples, "against the oracle")


@pytest.mark.parametrize("samples,n", [(16, AE.FALLBACK_POINTS), (128, 17)])
def test_direct_light_whole_call_fallbacks(gpu, oracle, samples, n):
    install_dl(gpu, oracle, "moving 38+9")
    scene, lights, _, _, p, nrm = AE.dl_set(oracle, "moving 38+9")
    with Mode(gpu, "tree forced") as accel:
        for what, (tm, lo, hi) in {**AE.INSIDE, **AE.FALLBACKS}.items():
            lo, hi = DL.LO if lo is None else lo, DL.HI if hi is None else hi
            if "NaN" in what:
                _, _, _, _, st = TD.check(gpu, scene, lights, first(p, n), first(nrm, n), samples, (what, samples), time=tm, lo=lo, hi=hi, accel=accel)
            else:
                st = direct_against(gpu, oracle, "moving 38+9", n, samples, (what, samples), time=tm, lo=lo, hi=hi, accel=accel)[4]
            assert (st.node_tests > 0) == (what in AE.INSIDE), (what, st.node_tests)


def test_the_camera_forms_whole_call_fallbacks(gpu, oracle):
    """Both passes of a camera form fall back together with the time; with a NaN in one pass's range that pass walks the lists and the other
    keeps the tree, both ways round."""
    scene, lights, (t0, t1), _, _, _ = AE.dl_set(oracle, "moving 38+9")
    width, height = 17, 9
    cam = QE.forty_camera(width, height)
    gpu.set_scene(scene, t0, t1)
    gpu.set_lights(lights)
    nan = QE.NAN
    with Mode(gpu, "tree forced") as accel:
        def passes(tm, mint, second_lo, second_hi, ao):
            """(the depth pass's node visits, the second pass's) of one camera-form call, checked against its definition."""
            what = ("ao_map" if ao else "direct_light_map", tm, mint, second_lo, second_hi)
            if ao:
                TA.check_map(gpu, cam, width, height, what, mint=mint, maxt=MAXT, samples=16, radius=second_hi, accel=accel, ao_mint=second_lo, time=tm)
                total = gpu.ao_map(cam, width, height, mint, MAXT, 16, second_hi, ao_mint=second_lo, time=tm, accel=accel)[-1].node_tests
            else:
                TD.check_map(gpu, cam, width, height, what, mint=mint, maxt=MAXT, samples=16, accel=accel, time=tm, lo=second_lo, hi=second_hi)
                total = gpu.direct_light_map(cam, width, height, mint, MAXT, 16, lo=second_lo, hi=second_hi, time=tm, accel=accel)[-1].node_tests
            depth = gpu.depth_map(cam, width, height, mint, MAXT, time=tm, accel=accel)[-1].node_tests
            return depth, total - depth

        for ao, (lo, hi) in ((True, (AO.AO_MINT, 1.0)), (False, (DL.LO, DL.HI))):
            for tm in (TIME, 0.0, 1.0):
                depth, second = passes(tm, MINT, lo, hi, ao)
                assert depth > 0 and second > 0, (ao, tm, depth, second)
                if ao:
                    got = gpu.ao_map(cam, width, height, MINT, MAXT, 16, hi, ao_mint=lo, time=tm, accel=accel)[0]
                    assert same(got, ao_map_oracle(gpu, oracle, scene, cam, width, height, MINT, MAXT, 16, hi, lo, 0, tm, accel)), (tm, "against the oracle")
                else:
                    got = gpu.direct_light_map(cam, width, height, MINT, MAXT, 16, lo=lo, hi=hi, time=tm, accel=accel)[:2]
                    want = direct_map_oracle(gpu, oracle, scene, lights, cam, width, height, MINT, MAXT, 16, 0, tm, lo, hi, accel)
                    assert same(got[0], want[0]) and same(got[1], want[1]), (tm, "against the oracle")
            for tm in (-0.5, 1.5, nan):
                assert passes(tm, MINT, lo, hi, ao) == (0, 0), (ao, tm)
            depth, second = passes(TIME, nan, lo, hi, ao)
            assert depth == 0 and second > 0, (ao, "a NaN in the depth pass's range", depth, second)
            for second_range in ((nan, hi), (lo, nan)):
                depth, second = passes(TIME, MINT, *second_range, ao)
                assert depth > 0 and second == 0, (ao, "a NaN in the second pass's range", second_range, depth, second)


@pytest.mark.parametrize("mode", BOTH)
def test_the_camera_forms_round_loop_on_a_moving_scene(gpu, oracle, mode):
    """128 samples (two rounds) from the camera at a time inside the shutter, through the tree and the lists: the builds <CAM, TREE or not,
    MOVING, not ONE> of both fused kernels, which no other case launches.  A 65 x 2 map: a wave edge plus one."""
    scene, lights, (t0, t1), _, _, _ = AE.dl_set(oracle, "moving 38+9")
    width, height, samples = 65, 2, 128
    cam = QE.forty_camera(width, height)
    gpu.set_scene(scene, t0, t1)
    gpu.set_lights(lights)
    with Mode(gpu, mode) as accel:
        what = (mode, samples, TIME)
        ao, ids, _ = TA.check_map(gpu, cam, width, height, what, samples=samples, radius=1.0, accel=accel, time=TIME)
        assert same(ao, ao_map_oracle(gpu, oracle, scene, cam, width, height, MINT, MAXT, samples, 1.0, AO.AO_MINT, 0, TIME, accel)), what
        vis, irr, _ = TD.check_map(gpu, cam, width, height, what, samples=samples, accel=accel, time=TIME)
        want = direct_map_oracle(gpu, oracle, scene, lights, cam, width, height, MINT, MAXT, samples, 0, TIME, DL.LO, DL.HI, accel)
        assert same(vis, want[0]) and same(irr, want[1]), what
        st = gpu.direct_light_map(cam, width, height, MINT, MAXT, samples, time=TIME, accel=accel)[-1]
    assert (ids >= 0).sum() >= 8 and (st.node_tests > 0) == (mode == "tree forced"), (mode, int((ids >= 0).sum()), st.node_tests)


# ---- 4. a light that moves ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("key", list(AE.MOVING_LIGHTS))
def test_a_light_that_moves(gpu, oracle, key, mode):
    """The rule reads a sphere light's centre at time 0; the walk meets the sphere where it stands at `time`."""
    name = "moving " + key
    install_dl(gpu, oracle, name)
    v = {}
    with Mode(gpu, mode) as accel:
        for tm in (0.0, TIME, 1.0):
            v[tm] = direct_against(gpu, oracle, name, AE.MOVING_POINTS, 16, (key, mode, tm), time=tm, accel=accel)[2]
        if key == "5":
            for tm in (0.0, 1.0):
                direct_against(gpu, oracle, name, 33, 128, (key, mode, tm, 128), time=tm, accel=accel)
    assert np.any(v[0.0] != v[1.0]), "the time does not reach the walk"


# ---- 5. light and point geometry at the edges -----------------------------------------------------------------------------------------------------
def check_nan(r, scene, lights, points, normals, samples, what, **kw):
    """TD.check with one latitude: an item of irr whose host answer is a NaN must be a NaN on the device, payload and sign left open (x86 and
    the GPU form them differently); every other item of irr and all of vis are equal on the bits, the sign of a zero included."""
    vis, irr, st = r.direct_light(points, normals, samples, **kw)
    want_vis, want_irr, v, cast, stats = TD.composition(r, scene, lights, points, normals, samples, **kw)
    assert vis.dtype == F and irr.dtype == F and same(vis, want_vis), (what, "vis")
    bad = np.flatnonzero(~AE.same_or_nan(irr, want_irr).reshape(-1))
    assert len(bad) == 0, (what, "irr", len(bad), bad[:8], irr.reshape(-1)[bad[:8]], want_irr.reshape(-1)[bad[:8]])
    assert TD.counters(st) == stats, (what, "segments and counters against scene_occluded's", TD.counters(st), stats)
    alone, st1 = r.direct_light(points, normals, samples, irradiance=False, **kw)
    assert same(alone, vis) and TD.counters(st1) == stats, (what, "without irr_out")
    return vis, irr, v, cast, want_irr


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_one_spoiler_among_ordinary_items(gpu, oracle, accel):
    scene, plain, under = AE.edge_scene()
    p, nrm = AE.edge_points()
    gpu.set_scene(scene)
    mates = np.ones(AE.EDGE_POINTS, bool)
    mates[AE.SPOILED] = False
    with Mode(gpu, "tree forced" if accel == R.ACCEL_BVH else "brute") as a:
        for which, lights in enumerate((plain, under)):
            gpu.set_lights(lights)
            want = AE.edge_oracle(oracle, which)
            vis, irr, v, cast, _ = TD.check(gpu, scene, lights, p, nrm, 16, ("unspoiled", which), accel=a)
            assert same(vis, want[0]) and same(irr, want[1]) and TD.mixed(v, cast, 16)
        for kind, (_, _, which, light) in AE.SPOILERS.items():
            lights, sp, sn = AE.spoiled(kind)
            gpu.set_lights(lights)
            want = AE.edge_oracle(oracle, which)
            vis, irr, v, cast, host_irr = check_nan(gpu, scene, lights, sp, sn, 16, kind, accel=a)
            assert same(vis[mates], want[0][mates]) and same(irr[mates], want[1][mates]), (kind, "the ordinary items keep the oracle's answer")
            assert cast[AE.SPOILED].any(), (kind, "the spoilers cast nothing")
            if kind == "in the plane of the quad light":
                assert (cast[AE.SPOILED, 0] == 16).all() and not irr[AE.SPOILED, 0].any() and not np.signbit(irr[AE.SPOILED, 0]).any()
            if kind == "so far that dd * dd overflows":
                assert not irr[AE.SPOILED].any() and not np.signbit(irr[AE.SPOILED]).any()
            if kind == "so near that dd * dd underflows":
                lit = v[AE.SPOILED, 2] > 0
                assert lit.any() and not np.isfinite(host_irr[AE.SPOILED, 2][lit]).any() and not np.isfinite(irr[AE.SPOILED, 2][lit]).any()


def test_a_degenerate_quad_as_a_light(gpu, oracle):
    """A quad with u == v == 0: the constructors, set_scene and set_lights all accept it (nothing refuses a degenerate light).  A point
    exactly at its corner has d == 0 under it and casts nothing; every other point's segments end in that corner."""
    scene, lights = AE.degenerate_scene()
    p, nrm = (a.copy() for a in AE.edge_points())
    p[AE.SPOILED] = np.array([1.0, 0.25, -1.0], F)
    nrm[AE.SPOILED] = AE.UP
    gpu.set_scene(scene)
    gpu.set_lights(lights)
    assert gpu.light_count() == 3
    want = AE.dl_answer(oracle, scene, lights, p, nrm, 16, 0, 0.0, DL.LO, DL.HI)
    assert not want[2].any(), "as an occluder the degenerate quad stops every ray in the oracle: its NaN plane passes every comparison of the quad test"
    for mode in BOTH:
        with Mode(gpu, mode) as accel:
            vis, irr, v, cast, _ = check_nan(gpu, scene, lights, p, nrm, 16, ("a degenerate light", mode), accel=accel)
        print(f"\n[edges] a degenerate light, {mode}: cast {cast.sum(axis=0)}, visible {v.sum(axis=0)}, NaN irr {np.isnan(irr).sum(axis=0)}")
        assert not cast[AE.SPOILED, 2].any() and not vis[AE.SPOILED, 2].any() and not irr[AE.SPOILED, 2].any(), "d == 0 is not cast"
        assert cast[:, 2].any() and cast[AE.SPOILED, :2].any()
        assert same(vis, want[0]) and AE.same_or_nan(irr, want[1]).all() and np.array_equal(cast, want[3]), (mode, "against the oracle")


# ---- 6. the sum's association ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BOTH)
@pytest.mark.parametrize("samples", AE.ASSOC_SAMPLES)
def test_the_sum_of_weights_that_span_many_binades(gpu, oracle, samples, mode):
    """irr is rtw_light_reduce of the masked host weights on the bits, where (tests/test_any_hit_edges_cpu.py) an ascending sum and a
    round-major one give other bits for a quarter of the items."""
    scene, lights, _, p, nrm = install_dl(gpu, oracle, "corner")
    with Mode(gpu, mode) as accel:
        _, irr, v, _, _ = direct_against(gpu, oracle, "corner", len(p), samples, (samples, mode), accel=accel)
    _, w = R.light_samples(scene, lights, p, nrm, samples, 0)
    occ = AE.dl_oracle(oracle, "corner", len(p), samples)[4]
    assert same(irr, R.light_reduce(np.where(occ, F(0.0), w).astype(F)))
    assert (v > 0).all() and (v < samples).any()


# ---- 7. state between calls -------------------------------------------------------------------------------------------------------------------------
def test_the_lights_and_the_scene_between_calls(gpu, oracle):
    scene, lights, _, _, _, _, _ = DL.case("geom")
    p, nrm = (first(a, 129) for a in DL.points_of(oracle, "geom"))
    gpu.set_scene(scene)
    gpu.set_lights(lights)
    before = TD.check(gpu, scene, lights, p, nrm, 16, "the first list")[:2]
    assert same(before[0], first(DL.reference(oracle, "geom")[0], 129))
    other = [lights[1], (R.LIGHT_QUAD, 0), lights[0]]
    gpu.set_lights(other)                                               # another list: the next call follows it, and so does light_count
    assert gpu.light_count() == 3
    vis, irr, _, _, _ = TD.check(gpu, scene, other, p, nrm, 16, "another list")
    want = AE.dl_answer(oracle, scene, other, p, nrm, 16, 0, 0.0, DL.LO, DL.HI)
    assert vis.shape == (129, 3) and same(vis, want[0]) and same(irr, want[1])
    gpu.set_lights(lights[:1])
    assert gpu.light_count() == 1
    vis, _, _, _, _ = TD.check(gpu, scene, lights[:1], p, nrm, 16, "a shorter list")
    assert same(vis, np.ascontiguousarray(before[0][:, :1]))
    # a scene whose sphere at the light's index stands elsewhere, then the same (kind, index) list: the rows follow the new scene
    moved = AE.geom_with_its_sphere_light_moved()
    gpu.set_scene(moved)
    assert gpu.light_count() == 0, "a new scene clears the lights"
    vv, ii = np.full(4 * 2, 7.0, F), np.full(4 * 2, 7.0, F)
    rc = R.lib().rtw_ctx_direct_light(gpu._h, p.ctypes.data, nrm.ctypes.data, 4, 16, 0, 0.0, DL.LO, DL.HI, R.ACCEL_BVH, vv.ctypes.data, ii.ctypes.data, None)
    assert rc == E_INVALID and (vv == 7.0).all() and (ii == 7.0).all(), "after set_scene alone there are no lights"
    with pytest.raises(R.RtwError):
        gpu.direct_light(p, nrm, 16)
    gpu.set_lights(lights)
    vis, irr, _, _, _ = TD.check(gpu, moved, lights, p, nrm, 16, "the same list in the new scene")
    want = AE.dl_answer(oracle, moved, lights, p, nrm, 16, 0, 0.0, DL.LO, DL.HI)
    assert same(vis, want[0]) and same(irr, want[1]) and not same(vis[:, 1], before[0][:, 1]), "the rows are the old scene's"


def test_the_list_walk_option_between_calls(gpu, oracle):
    scene, lights, time, p, nrm = install_dl(gpu, oracle, "forty")
    p, nrm = first(p, 129), first(nrm, 129)
    radius = AO.RADIUS["forty"]
    want_ao = AE.ao_oracle(oracle, "forty", 129, 16)[1]
    q, m = (first(a, 129) for a in AO.points_of(oracle, "forty"))
    want = AE.dl_oracle(oracle, "forty", 129, 16)
    nodes = []
    try:
        for walk_max in (0, 48, 0, 1000, 39, 40):
            gpu.set_option(R.OPT_LIST_WALK_MAX, walk_max)
            ao, _, ast = TA.check(gpu, q, m, 16, radius, ("list_walk_max", walk_max), time=time)
            vis, irr, _, _, st = TD.check(gpu, scene, lights, p, nrm, 16, ("list_walk_max", walk_max), time=time)
            assert same(ao, want_ao) and same(vis, want[0]) and same(irr, want[1]), walk_max
            assert (ast.node_tests > 0) == (st.node_tests > 0) == (walk_max < 40), (walk_max, ast.node_tests, st.node_tests)
            nodes.append((ast.node_tests, st.node_tests))
    finally:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    assert nodes[0] == nodes[2] == nodes[4], "the option's history reaches a call"
