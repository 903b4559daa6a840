"""rtw_ctx_scene_occluded on the MI355X: the any-hit pass against the CPU oracle and against rtw_ctx_scene_hits on the same context, exactly --
occluded[i] is `index >= 0`, for every ray, under both accels and every fall-back -- and its early exit against scene_hits' counters.

The inputs and their references are tests/occluded_common.py's (tests/test_occluded_cpu.py proves on the CPU that each exercises both
outcomes); every comparison is exact and leaves no ray out."""
import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import mesh_move_common as MM
from tests import mesh_top_common as MT
from tests import occluded_common as OC
from tests import quat_common as QC
from tests import query_edges_common as QE
from tests import refit_common as RC
from tests.test_gpu_stream_order import Hazard, ctx, cycles_per_ms, fresh, same, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_NO_SCENE = -1, -6
MODES = {"brute": (R.ACCEL_BRUTE, 48), "bvh as shipped": (R.ACCEL_BVH, 48), "tree forced": (R.ACCEL_BVH, 0)}
COUNTERS = ("sphere_tests", "node_tests", "quad_tests")


def query(r, rays, mint, maxt, time=0.0, accel=R.ACCEL_BVH, what=""):
    """(occluded, its stats, scene_hits' stats) of one ray set on `r`, with the two checks every case makes: the bit is scene_hits' `index >= 0`,
    and no counter is above scene_hits' (an any-hit walk is a prefix of the closest-hit walk)."""
    occ, st = r.scene_occluded(rays, mint, maxt, time=time, accel=accel)
    _, idx, hst = r.scene_hits(rays, mint, maxt, time=time, accel=accel)
    OC.assert_same(occ, OC.occluded_of(idx), (what, "against scene_hits"))
    assert st.segments == hst.segments == len(np.asarray(rays).reshape(-1, 6)) and st.kernel_ms > 0.0
    for k in COUNTERS:
        assert getattr(st, k) <= getattr(hst, k), (what, k, getattr(st, k), getattr(hst, k))
    return occ, st, hst


class Mode:
    """RTW_OPT_LIST_WALK_MAX for the duration of a case, the default again afterwards."""

    def __init__(self, r, mode):
        self.r, (self.accel, self.walk_max) = r, MODES[mode]

    def __enter__(self):
        self.r.set_option(R.OPT_LIST_WALK_MAX, self.walk_max)
        return self.accel

    def __exit__(self, *exc):
        self.r.set_option(R.OPT_LIST_WALK_MAX, 48)


# ---- whole scenes and one group at a time ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", OC.SCENES)
def test_whole_scenes_equal_the_oracle_and_scene_hits(gpu, oracle, name, mode):
    scene, (t0, t1), rays, time, mint, maxt = OC.scene_case(name)
    want = OC.scene_reference(oracle, name)
    gpu.set_scene(scene, t0, t1)
    with Mode(gpu, mode) as accel:
        occ, st, hst = query(gpu, rays, mint, maxt, time, accel, (name, mode))
    OC.assert_same(occ, want, (name, mode, "against the oracle"))
    print(f"\n[occluded] {name}, {mode}: " + ", ".join(f"{k} {getattr(st, k)} / {getattr(hst, k)}" for k in COUNTERS) + " (any-hit / closest-hit)")
    if mode == "brute":
        assert st.node_tests == 0
    if mode == "tree forced" and scene.n_spheres:
        assert st.node_tests > 0
        if name in ("forty", "forty+duplicate", "field", "field, short range", "spheres"):
            assert st.sphere_tests < scene.n_spheres * len(rays)
    if name == "forty" and mode == "brute":                        # a list walk tests every sphere for every ray; an occluded ray stops at its sphere
        assert hst.sphere_tests == 40 * len(rays) and st.sphere_tests < hst.sphere_tests


# ---- waves with mixed lanes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_one_spoiler_per_wave(gpu, oracle, accel):
    base, want, kinds = QE.wave_reference(oracle)
    want = OC.occluded_of(want[1])
    assert len(base) == 1024 and 0.2 <= OC.share(want) <= 0.8
    gpu.set_scene(QE.field_scene())
    occ, st, _ = query(gpu, base, QE.D_MINT, QE.D_MAXT, accel=accel, what="the ordinary rays")
    OC.assert_same(occ, want, "the ordinary rays against the oracle")
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH) and (accel == R.ACCEL_BRUTE or st.sphere_tests < 63 * 1024)      # (63 spheres: the tree as shipped)
    for kind, (launch, pos, spoilers) in kinds.items():
        occ, _, _ = query(gpu, launch, QE.D_MINT, QE.D_MAXT, accel=accel, what=kind)         # the spoilers answer what scene_hits answers
        mates = np.ones(len(launch), bool)
        mates[pos] = False
        OC.assert_same(occ[mates], want[mates], (kind, "the 63 mates of every wave keep the oracle's answer"))
        if kind != "NaN":                                                                      # (a NaN ray's answer is the list walk's: scene_hits above)
            OC.assert_same(occ[pos], OC.occluded_of(spoilers[1]), (kind, "the spoilers against the oracle"))
    for perm in (np.arange(1024)[::-1], np.random.default_rng(5).permutation(1024)):
        occ, _, _ = query(gpu, np.ascontiguousarray(base[perm]), QE.D_MINT, QE.D_MAXT, accel=accel, what="permuted")
        OC.assert_same(occ, want[perm], "permuted rays give the permuted answer")


# ---- partial waves and blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 255, 256, 257])
def test_prefixes_and_the_byte_behind_the_output(gpu, oracle, torch, n_rays):  # noqa: F811
    scene, _, rays, time, mint, maxt = OC.scene_case("field")
    want = OC.scene_reference(oracle, "field")
    gpu.set_scene(scene)
    occ, _, _ = query(gpu, rays[:n_rays], mint, maxt, what=n_rays)
    OC.assert_same(occ, want[:n_rays], (n_rays, "the prefix of the 1024-ray answer"))
    d_rays = torch.from_numpy(np.ascontiguousarray(rays[:n_rays])).to("cuda:0")
    d_out = torch.full((n_rays + 1,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    out, st = gpu.scene_occluded(d_rays, mint, maxt, out=d_out[:n_rays])
    got = d_out.cpu().numpy()
    assert got[n_rays] == 7, "the byte behind occluded_out was written"
    OC.assert_same(got[:n_rays].view(np.bool_), want[:n_rays], (n_rays, "device tensors"))
    assert set(np.unique(got[:n_rays])) <= {0, 1} and out.data_ptr() == d_out.data_ptr() and st.segments == n_rays
    b_out = torch.zeros(n_rays, dtype=torch.bool, device="cuda:0")
    torch.cuda.synchronize()
    gpu.scene_occluded(d_rays, mint, maxt, out=b_out)
    OC.assert_same(b_out.cpu().numpy(), want[:n_rays], (n_rays, "a torch.bool output"))


# ---- range edges and the whole-call fall-backs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_range_edges(gpu, oracle, mode):
    scene, time, rays, cases, base = QE.range_reference(oracle, "forty")
    assert (base[1] >= 0).all()
    gpu.set_scene(scene, 0.0, 1.0)
    flips = visits = 0
    with Mode(gpu, mode) as accel:
        for mint, maxt, want, j in cases:
            occ, st, _ = query(gpu, rays, mint, maxt, time, accel, (mode, mint, maxt))
            OC.assert_same(occ, OC.occluded_of(want[1]), (mode, mint, maxt, "against the oracle"))
            visits += st.node_tests
            flips += int(not occ[j])
            if mint > maxt:
                assert not occ.any()
    assert (visits > 0) == (mode == "tree forced")
    assert flips >= 8                                                   # the edges do turn occluded rays free


@pytest.mark.parametrize("cls", list(QE.RANGES))
@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_the_edge_rays_of_every_range_class(gpu, oracle, cls, accel):
    mint, maxt, cuts, row, batch, pos, _, want = QE.edge_reference(oracle)[cls]
    gpu.set_scene(QE.field_scene())
    query(gpu, row, mint, maxt, accel=accel, what=(cls, "the edge rays in a row"))
    occ, _, _ = query(gpu, batch, mint, maxt, accel=accel, what=(cls, "scattered through ordinary rays"))
    mates = np.ones(len(batch), bool)
    mates[pos] = False
    OC.assert_same(occ[mates], OC.occluded_of(want[1])[mates], (cls, "the ordinary rays against the oracle"))


def test_whole_call_fallbacks_walk_the_lists(gpu, oracle):
    scene, rays, inside, cases = QE.fallback_reference(oracle)
    gpu.set_scene(scene, 0.0, 1.0)
    with Mode(gpu, "tree forced") as accel:
        occ, st, _ = query(gpu, rays, QE.MINT, QE.FALLBACK_MAXT, QE.TIME, accel, "inside the time range")
        OC.assert_same(occ, OC.occluded_of(inside[1]), "inside the time range, against the oracle")
        assert st.node_tests > 0
        for name, (tm, lo, hi, want) in cases.items():
            occ, st, _ = query(gpu, rays, lo, hi, tm, accel, name)
            assert st.node_tests == 0, name
            if "NaN" not in name:
                OC.assert_same(occ, OC.occluded_of(want[1]), (name, "against the oracle"))


# ---- quaternion instances ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_quaternion_instances(gpu, accel):
    g = QC.golden()
    qs = QC.fixture_scene(g)
    qs.install(gpu)
    rays = R.depth_rays(QC.camera(g, 40, 30), 40, 30)
    occ, _, _ = query(gpu, rays, g["mint"], g["maxt"], accel=accel, what="the golden rotation scene")
    assert occ.any() and not occ.all()


# ---- placements -----------------------------------------------------------------------------------------------------------------------------------
def install_placements(r, pods, pl):
    r.set_scene(R.Scene(()))
    r.set_triangles(list(pods))
    r.set_mesh_instances(pl)


def test_placements_in_list_order_and_through_the_top_level_tree(gpu):
    nodes = {}
    try:
        for name, list_max in (("standard", R.MESH_LIST_MAX_DEFAULT), ("grid8", 0), ("grid8", MT.NEVER)):
            pods, pl, rays = OC.placement_case(name)
            install_placements(gpu, pods, pl)
            gpu.set_option(R.OPT_MESH_LIST_MAX, list_max)
            for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
                occ, st, hst = query(gpu, rays, MI.MINT, MI.MAXT, accel=accel, what=(name, list_max, accel))
                OC.assert_same(occ, OC.placement_reference(name), (name, list_max, accel, "against the host list walk"))
                assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
                print(f"\n[occluded] {name}, list_max {list_max}, accel {accel}: node visits {st.node_tests} / {hst.node_tests}, "
                      f"triangle tests {st.quad_tests} / {hst.quad_tests} (any-hit / closest-hit)")
                nodes[name, list_max, accel] = st.node_tests
            if name == "grid8" and list_max == 0:                       # the host form is this walk: the same counters
                h_occ, h_st = R.mesh_instance_occluded(list(pods), pl, rays, MI.MINT, MI.MAXT)
                OC.assert_same(occ, h_occ, "the host any-hit form")
                occ, st = gpu.scene_occluded(rays, MI.MINT, MI.MAXT)
                assert (st.node_tests, st.quad_tests) == (h_st.node_tests, h_st.quad_tests)
    finally:
        gpu.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)
    assert nodes["grid8", 0, R.ACCEL_BVH] < nodes["grid8", MT.NEVER, R.ACCEL_BVH]


# ---- after a refit and after a move ----------------------------------------------------------------------------------------------------------------
def test_a_refit_is_seen_by_the_next_query(ctx):  # noqa: F811
    v, f, _, _ = RC.mesh("terrain12")
    w = RC.sine_wave(v, f)
    rays = OC.mesh_rays(w, f)
    ctx.set_scene(R.Scene((), triangles=RC.triangles_of(v, f)))
    before, _, _ = query(ctx, rays, MI.MINT, MI.MAXT, what="before the refit")
    assert ctx.refit_triangles(R.mesh_ouv(w, f)) == 0
    after = {accel: query(ctx, rays, MI.MINT, MI.MAXT, accel=accel, what=("after the refit", accel)) for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE)}
    assert after[R.ACCEL_BVH][1].node_tests > 0
    with R.Renderer(0) as other:
        other.set_scene(R.Scene((), triangles=RC.triangles_of(w, f)))
        want, _ = other.scene_occluded(rays, MI.MINT, MI.MAXT)
    for accel in after:
        OC.assert_same(after[accel][0], want, ("a fresh context with the deformed mesh", accel))
    assert want.sum() >= 20 and (~want).sum() >= 20 and np.any(want != before)


def test_a_move_is_seen_by_the_next_query(ctx):  # noqa: F811
    pods, pl, rays = OC.placement_case("grid8")
    moved = MM.turn_and_shift(MM.as_array(pl))
    install_placements(ctx, pods, pl)
    before, _, _ = query(ctx, rays, MI.MINT, MI.MAXT, what="before the move")
    OC.assert_same(before, OC.placement_reference("grid8"), "before the move")
    assert ctx.move_mesh_instances(moved) == 0
    after = {accel: query(ctx, rays, MI.MINT, MI.MAXT, accel=accel, what=("after the move", accel)) for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE)}
    assert after[R.ACCEL_BVH][1].node_tests > 0
    with R.Renderer(0) as other:
        install_placements(other, pods, MM.as_list(moved))
        want, _ = other.scene_occluded(rays, MI.MINT, MI.MAXT)
    for accel in after:
        OC.assert_same(after[accel][0], want, ("a fresh context with the moved placements", accel))
    assert np.any(want != before)


# ---- segments ---------------------------------------------------------------------------------------------------------------------------------------
def test_segments(gpu, oracle, torch):  # noqa: F811
    p, q = OC.segment_pairs()
    gpu.set_scene(QE.field_scene())
    by_hand, _, _ = query(gpu, OC.segment_rays(p, q), OC.SEG_LO, OC.SEG_HI, what="segments by hand")
    occ, st = gpu.segments_occluded(p, q)
    OC.assert_same(occ, by_hand, "segments_occluded against the rays built by hand")
    assert st.segments == 512 and 0.2 <= OC.share(occ) <= 0.8
    tp, tq = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(q).to("cuda:0")
    torch.cuda.synchronize()
    gpu.use_torch_stream()                                              # behind torch's subtraction, on torch's stream
    try:
        t_occ, _ = gpu.segments_occluded(tp, tq)
        assert t_occ.dtype == torch.uint8 and t_occ.is_cuda
        assert same(t_occ.cpu().numpy(), occ.view(np.uint8)), "the torch path's bytes are not the numpy path's"
    finally:
        torch.cuda.synchronize()
        gpu.set_stream(0)
    # other defaults than the whole segment: nothing within the first thousandth
    none, _ = gpu.segments_occluded(p, q, lo=0.0, hi=1e-3)
    assert not none.any()


# ---- device tensors and stream order -----------------------------------------------------------------------------------------------------------------
def test_the_call_runs_behind_the_producers_of_its_tensors(ctx, torch, cycles_per_ms):  # noqa: F811
    scene, _, rays, time, mint, maxt = OC.scene_case("field")
    away = np.tile(np.array([0.0, 2000.0, 0.0, 0.0, 1.0, 0.0], F), (len(rays), 1))          # the stale rays: above everything, pointing up

    def answers(r):
        r.set_scene(scene)
        occ, st = r.scene_occluded(rays, mint, maxt)
        assert st.node_tests > 0
        assert not r.scene_occluded(away, mint, maxt)[0].any()
        return occ
    want = fresh(answers)
    assert 0.2 <= OC.share(want) <= 0.8
    ctx.set_scene(scene)
    warm_rays = torch.from_numpy(rays).to("cuda:0")
    warm_out = torch.zeros(len(rays), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.scene_occluded(warm_rays, mint, maxt, out=warm_out)                                  # once on its own stream, device tensors
    assert same(warm_out.cpu().numpy(), want.view(np.uint8))
    hz = Hazard(torch, cycles_per_ms)
    d_rays = hz.input(rays, stale=away)
    d_out = hz.output((len(rays),), torch.uint8, 9, 7)
    (got,), (_, st) = hz.run(ctx, "torch-default", lambda: ctx.scene_occluded(d_rays, mint, maxt, out=d_out))
    assert st.node_tests > 0
    assert same(got, want.view(np.uint8))


# ---- lifecycle --------------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_statuses(ctx):  # noqa: F811
    L = R.lib()
    scene, _, rays, time, mint, maxt = OC.scene_case("geom")
    r4 = np.ascontiguousarray(rays[:4])
    out = np.zeros(4, np.uint8)
    args = (0.0, mint, maxt)
    with R.Renderer(0) as other:
        assert L.rtw_ctx_scene_occluded(other._h, r4.ctypes.data, 4, *args, R.ACCEL_BVH, out.ctypes.data, None) == E_NO_SCENE
        with pytest.raises(R.RtwError):
            other.scene_occluded(r4, mint, maxt)
        other.set_scene(scene)
        second, _ = other.scene_occluded(rays, mint, maxt)
    ctx.set_scene(scene)
    assert L.rtw_ctx_scene_occluded(ctx._h, r4.ctypes.data, 4, *args, 2, out.ctypes.data, None) == E_INVALID
    assert L.rtw_ctx_scene_occluded(ctx._h, r4.ctypes.data, 0, *args, R.ACCEL_BVH, out.ctypes.data, None) == E_INVALID
    assert L.rtw_ctx_scene_occluded(ctx._h, None, 4, *args, R.ACCEL_BVH, out.ctypes.data, None) == E_INVALID
    assert L.rtw_ctx_scene_occluded(ctx._h, r4.ctypes.data, 4, *args, R.ACCEL_BVH, None, None) == E_INVALID
    assert L.rtw_ctx_scene_occluded(None, r4.ctypes.data, 4, *args, R.ACCEL_BVH, out.ctypes.data, None) == E_INVALID
    assert not out.any()
    assert L.rtw_ctx_scene_occluded(ctx._h, r4.ctypes.data, 4, *args, R.ACCEL_BVH, out.ctypes.data, None) == R.RTW_OK      # (stats may be NULL)
    first, _ = ctx.scene_occluded(rays, mint, maxt)
    assert same(first, second) and same(first[:4].view(np.uint8), out)
    with pytest.raises(ValueError):
        ctx.scene_occluded(rays, mint, maxt, out=np.zeros(len(rays), np.uint8))
