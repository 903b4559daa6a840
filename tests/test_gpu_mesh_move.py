"""rtw_ctx_move_mesh_instances on the MI355X: the device's top-level tree and placement rows against the host form byte for byte, from numpy
and from a torch tensor; hits, renders and scene queries after a move against the host list walk and against a fresh context that got the
moved mesh and poses through the setters; invalid poses, the reach, the lifecycle, the call's place on a torch stream.  Parity is on the bits
everywhere."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import mesh_move_common as MM
from tests import mesh_top_common as MT
from tests.test_gpu_stream_order import Hazard, cycles_per_ms, same, torch  # noqa: F401  (the fixtures and helpers of the stream-order tests)

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_NO_SCENE = -1, -6
CASES = MM.cases()
FLOOR = [R.Sphere.new((0.0, -60.0, 0.0), 0.5, (0.5, 0.5, 0.5), R.SCATTER_M)]


@pytest.fixture(scope="module")
def ctx():
    assert R.device_count() > 0, "no HIP device visible: -m gpu tests need the MI355X"
    with R.Renderer(0) as r:
        yield r


def install(r, T, pl, spheres=FLOOR):
    r.set_scene(R.Scene(list(spheres), background=(0.7, 0.8, 1.0)))
    r.set_triangles(T.pods())
    r.set_mesh_instances(pl)


def give(torch, source, a):  # noqa: F811
    if source == "numpy":
        return a
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def assert_dump(r, want_nodes, want_rows, what):
    nodes, rows = r.mesh_top_dump()
    assert MM.same_bytes(nodes, want_nodes), (what, "nodes", int((nodes["lo"] != want_nodes["lo"]).sum()), int((nodes["hi"] != want_nodes["hi"]).sum()))
    assert MM.same_bytes(rows, want_rows), (what, "rows", int((rows.view(np.uint32) != want_rows.view(np.uint32)).sum()))


# ---- the dump after a move ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["numpy", "torch"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_dump_after_a_move_equals_the_host_form(ctx, torch, name, source):  # noqa: F811
    T, pl = CASES[name]
    pods = T.pods()
    install(ctx, T, pl)
    built = R.mesh_top_dump(pods, pl)[0]
    assert_dump(ctx, built, MM.rows_of(MM.as_array(pl)), (name, "as set"))
    for motion, fn in MM.MOTIONS.items():
        moved = fn(MM.as_array(pl))
        want = R.mesh_top_refit(pods, pl, moved)
        assert want[2:] == (0, 0)
        assert ctx.move_mesh_instances(give(torch, source, moved)) == 0
        assert_dump(ctx, want[0], want[1], (name, motion))
        assert ctx.move_mesh_instances(give(torch, source, moved)) == 0          # a second identical move changes no byte
        assert_dump(ctx, want[0], want[1], (name, motion, "again"))
        for climb in (1, 2):                                                      # both forms of the climb, whatever the default chooses
            ctx.set_option(R.OPT_MESH_CLIMB, climb)
            try:
                assert ctx.move_mesh_instances(MM.as_array(pl)) == 0
                assert ctx.move_mesh_instances(give(torch, source, moved)) == 0
            finally:
                ctx.set_option(R.OPT_MESH_CLIMB, 0)
            assert_dump(ctx, want[0], want[1], (name, motion, "climb", climb))
        assert ctx.move_mesh_instances(MM.as_array(pl)) == 0                      # back: the builder's bytes
        assert_dump(ctx, built, MM.rows_of(MM.as_array(pl)), (name, motion, "back"))


@pytest.mark.parametrize("source", ["numpy", "torch"])
@pytest.mark.parametrize("scale", [2.0 ** -60, 2.0 ** -70, 2.0 ** 60])
def test_tiny_and_huge_quaternions_give_the_hosts_rows(ctx, torch, scale, source):  # noqa: F811
    """At 2^-70 the squares of the components are f32 denormals: the device's normalisation, denormals included, must be the host's."""
    T, pl = CASES["grid64"]
    pods = T.pods()
    moved = MM.as_array(pl)
    moved[:, 3:] = (moved[:, 3:] * F(scale)).astype(F)
    want = R.mesh_top_refit(pods, pl, moved)
    install(ctx, T, pl)
    if want[3]:
        with pytest.raises(R.RtwError) as e:
            ctx.move_mesh_instances(give(torch, source, moved))
        assert e.value.status == E_INVALID
    else:
        assert ctx.move_mesh_instances(give(torch, source, moved)) == 0
    assert_dump(ctx, want[0], want[1], scale)
    assert want[3] < 32                                                           # (most poses are accepted at every scale)


def test_one_wide_case(ctx, torch):  # noqa: F811
    """128 x 128 placements: some height above the leaves holds more than 1024 nodes -- the largest workgroup HIP allows --, so the one-workgroup
    climb strides whatever its block size; both forms of the climb give the host's bytes."""
    T, pl = MI.standard_mesh(), MT.grid(128)
    pods = T.pods()
    install(ctx, T, pl)
    moved = MM.turn_and_shift(MM.as_array(pl))
    want = R.mesh_top_refit(pods, pl, moved)
    h = MM.heights(want[0])
    per_height = np.bincount(h)
    assert per_height[1:].max() > 1024, per_height[:4]
    for climb in (0, 1, 2):
        ctx.set_option(R.OPT_MESH_CLIMB, climb)
        try:
            assert ctx.move_mesh_instances(MM.as_array(pl)) == 0
            assert ctx.move_mesh_instances(give(torch, "torch", moved)) == 0
        finally:
            ctx.set_option(R.OPT_MESH_CLIMB, 0)
        assert_dump(ctx, want[0], want[1], ("wide", climb))


# ---- hits and frames after a move ----------------------------------------------------------------------------------------------------------------
def placements_of(n):
    return MI.standard_placements() if n == 6 else MM.grid_n(n)


_WANT = {}


def moved_case(n, motion):
    """(mesh, placements, moved poses, rays, the host LIST walk's answer for the moved poses), computed once."""
    if (n, motion) not in _WANT:
        T, pl = MI.standard_mesh(), placements_of(n)
        moved = MM.MOTIONS[motion](MM.as_array(pl))
        rays = MI.standard_rays(placements=pl)
        _WANT[(n, motion)] = (T, pl, moved, rays, R.mesh_instance_hits(T.pods(), MM.as_list(moved), rays, MI.MINT, MI.MAXT))
    return _WANT[(n, motion)]


def frame_inputs(moved):
    c = moved[:, :3].astype(np.float64)
    mid, ext = c.mean(axis=0), max(2.0, float(np.abs(c - c.mean(axis=0)).max()))
    eye = mid + np.array([0.3 * ext, 0.8 * ext + 2.0, -1.6 * ext - 4.0])
    cam = R.Viewport.new_from_res(64, 48, 1, 4, 1.0, vfov=50.0, origin=tuple(eye), direction=tuple(mid - eye), vup=(0.0, 1.0, 0.0)).camera()
    dcam = R.camera2_new(64 / 48, tuple(eye), (0.0, 1.0, 0.0), tuple(mid - eye), 50.0, 0.0)
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth, p.gamma = 64, 48, 4, 6, 1.0
    p.mint, p.maxt = 0.001, 1e4
    p.integrator, p.sampler, p.flags, p.seed = R.INTEGRATOR_RUST2, R.SAMPLER_ROW, 0, 77
    return cam, dcam, p


def answers(r, cam, dcam, p, rays, accel):
    p.accel = accel
    img, st = r.render(cam, p)
    t, i, nrm, _ = r.scene_hits(rays, MI.MINT, MI.MAXT, accel=accel, normals=True)
    depth, ids, dn, _ = r.depth_map(dcam, 64, 48, MI.MINT, MI.MAXT, accel=accel, ids=True, normals=True)
    return dict(img=img, segments=st.segments, t=t, i=i, nrm=nrm, depth=depth, ids=ids, dn=dn)


def assert_answers(got, want, what):
    assert got["segments"] == want["segments"], what
    for k in ("img", "t", "nrm", "depth", "dn"):
        assert MI.same_nan(got[k], want[k]).all(), (what, k, int((~MI.same_nan(got[k], want[k])).sum()))
    for k in ("i", "ids"):
        assert np.array_equal(got[k], want[k]), (what, k)


SPHERES = FLOOR + [R.Sphere.new((0.8, 0.4, 2.0), 0.6, (0.8, 0.3, 0.3), R.METALLIC_M)]


@pytest.mark.parametrize("motion", list(MM.MOTIONS))
@pytest.mark.parametrize("n", [6, 64, 1024])
def test_hits_and_frames_after_a_move(ctx, n, motion):
    T, pl, moved, rays, want = moved_case(n, motion)
    share = float((want[1] >= 0).mean())
    print(f"\n[mesh move] {n} placements, {motion}: {share:.3f} of the rays hit")
    if motion != "shrink_to_a_point":                                              # (exempt: it leaves one spot to hit)
        assert 0.2 <= share <= 0.8, share
    install(ctx, T, pl, SPHERES)
    assert ctx.move_mesh_instances(moved) == 0
    cam, dcam, p = frame_inputs(moved)
    with R.Renderer(0) as fresh:
        install(fresh, T, MM.as_list(moved), SPHERES)
        for list_max in (R.MESH_LIST_MAX_DEFAULT, 0):
            ctx.set_option(R.OPT_MESH_LIST_MAX, list_max)
            fresh.set_option(R.OPT_MESH_LIST_MAX, list_max)
            try:
                for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
                    t, pidx, tri, nrm, st = ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT, accel=accel)
                    MI.assert_hits_equal((t, pidx, tri, nrm), want, (n, motion, list_max, accel))
                    tree_in_use = accel == R.ACCEL_BVH and n > list_max
                    if accel == R.ACCEL_BVH:
                        assert st.node_tests > 0
                    if tree_in_use and n == 1024:
                        assert st.node_tests < 1024 * len(rays)
                    assert_answers(answers(ctx, cam, dcam, p, rays, accel), answers(fresh, cam, dcam, p, rays, accel), (n, motion, list_max, accel))
            finally:
                ctx.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)


# ---- poses and mesh together ---------------------------------------------------------------------------------------------------------------------
def test_poses_and_mesh_together(ctx, torch):  # noqa: F811
    T, pl = MI.standard_mesh(), MM.grid_n(64)
    pods = T.pods()
    ouv, moved_T = MM.sine_ouv(T)
    ouv = ((ouv.reshape(-1, 3, 3) * F(0.4)).astype(F) + np.array([[[-1.8, 0.8, -0.4], [0, 0, 0], [0, 0, 0]]], F)).reshape(-1, 9).astype(F)
    moved_T = MI.TriSet([dict(t, origin=ouv[k, 0:3].tolist(), u=ouv[k, 3:6].tolist(), v=ouv[k, 6:9].tolist()) for k, t in enumerate(T.tris)])
    moved = MM.turn_and_shift(MM.as_array(pl))
    rays = MI.standard_rays(placements=pl)
    want_hits = R.mesh_instance_hits(moved_T.pods(), MM.as_list(moved), rays, MI.MINT, MI.MAXT)
    assert 0.1 <= float((want_hits[1] >= 0).mean()) <= 0.9
    want = R.mesh_top_refit(pods, pl, moved, ouv)
    install(ctx, T, pl, SPHERES)
    assert ctx.move_mesh_instances(give(torch, "torch", moved), give(torch, "torch", ouv)) == 0
    assert_dump(ctx, want[0], want[1], "poses and mesh")
    tri_nodes, lw = R.triangle_bvh_refit(pods, ouv)
    assert lw == 0 and MM.same_bytes(ctx.triangle_bvh_dump(), tri_nodes)
    cam, dcam, p = frame_inputs(moved)
    with R.Renderer(0) as fresh:
        install(fresh, moved_T, MM.as_list(moved), SPHERES)
        for accel in (R.ACCEL_BVH, R.ACCEL_BRUTE):
            got = ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT, accel=accel)
            MI.assert_hits_equal(got[:4], want_hits, ("poses and mesh", accel))
            assert_answers(answers(ctx, cam, dcam, p, rays, accel), answers(fresh, cam, dcam, p, rays, accel), ("poses and mesh", accel))


def test_the_mesh_alone_grows_under_standing_placements(ctx):
    """ouv alone with the mesh enlarged 1.7 x: a top-level box left at the old size would lose the hits on the rim."""
    T, pl = MI.standard_mesh(), MM.grid_n(64)
    ouv, big = MM.scaled_mesh(T, 1.7)
    rays = MI.standard_rays(placements=pl)
    small_hits = R.mesh_instance_hits(T.pods(), pl, rays, MI.MINT, MI.MAXT)
    want_hits = R.mesh_instance_hits(big.pods(), pl, rays, MI.MINT, MI.MAXT)
    assert ((want_hits[1] >= 0) & (small_hits[1] < 0)).sum() >= 100                # rays that only the enlarged mesh stops
    install(ctx, T, pl)
    ctx.set_option(R.OPT_MESH_LIST_MAX, 0)
    try:
        assert ctx.move_mesh_instances(None, ouv) == 0
        want = R.mesh_top_refit(T.pods(), pl, None, ouv)
        assert_dump(ctx, want[0], want[1], "ouv alone")
        got = ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT)
        MI.assert_hits_equal(got[:4], want_hits, "ouv alone")
        assert got[4].node_tests > 0
    finally:
        ctx.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)


# ---- invalid poses on the device -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["numpy", "torch"])
def test_invalid_poses_keep_their_placements(ctx, torch, source):  # noqa: F811
    T, pl = MI.standard_mesh(), MM.grid_n(64)
    pods = T.pods()
    old = MM.as_array(pl)
    moved = MM.turn_and_shift(old)
    where = [0, 32, 63]
    subst = moved.copy()
    subst[where] = old[where]
    rays = MI.standard_rays(placements=pl)
    install(ctx, T, pl)
    with pytest.raises(R.RtwError) as e:
        ctx.move_mesh_instances(give(torch, source, MM.spoil(moved, where)))
    assert e.value.status == E_INVALID
    want = R.mesh_top_refit(pods, pl, subst)
    assert_dump(ctx, want[0], want[1], "invalid poses")
    ctx.set_option(R.OPT_MESH_LIST_MAX, 0)
    try:
        got = ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT)
        MI.assert_hits_equal(got[:4], R.mesh_instance_hits(pods, MM.as_list(subst), rays, MI.MINT, MI.MAXT), "invalid poses")
        assert got[4].node_tests > 0
        assert ctx.move_mesh_instances(give(torch, source, moved)) == 0            # the next valid move succeeds
        want = R.mesh_top_refit(pods, pl, moved)
        assert_dump(ctx, want[0], want[1], "valid again")
        got = ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT)
        MI.assert_hits_equal(got[:4], R.mesh_instance_hits(pods, MM.as_list(moved), rays, MI.MINT, MI.MAXT), "valid again")
    finally:
        ctx.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)


# ---- reach -------------------------------------------------------------------------------------------------------------------------------------------
def test_beyond_the_reach_the_list_is_walked_and_a_move_back_recovers(ctx):
    T, pl = MI.standard_mesh(), MM.grid_n(64)
    pods = T.pods()
    near = MM.as_array(pl)
    far = near.copy()
    far[17, 0] = F(2.0 ** 39)
    rays = MI.standard_rays(placements=pl)

    def visits(value):
        ctx.set_option(R.OPT_MESH_LIST_MAX, value)
        try:
            return ctx.mesh_instance_hits(rays, MI.MINT, MI.MAXT)
        finally:
            ctx.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)

    for start in ("near", "far"):
        install(ctx, T, pl if start == "near" else MM.as_list(far))               # (far: set_mesh_instances itself was beyond reach)
        base = R.mesh_top_dump(pods, pl if start == "near" else MM.as_list(far))
        if start == "near":
            assert ctx.move_mesh_instances(far) == 2
        tree, never = visits(0), visits(MT.NEVER)
        want = R.mesh_instance_hits(pods, MM.as_list(far), rays, MI.MINT, MI.MAXT)
        MI.assert_hits_equal(tree[:4], want, (start, "far"))
        assert tree[4].node_tests == never[4].node_tests and tree[4].quad_tests == never[4].quad_tests     # no top-level visit: the list
        assert ctx.move_mesh_instances(near) == 0
        nodes, rows = ctx.mesh_top_dump()
        root = R.triangle_bvh_dump(pods)[0][0]
        assert MM.same_bytes(nodes, MM.expected_nodes(base[0], base[1], root, rows))
        tree, never = visits(0), visits(MT.NEVER)
        MI.assert_hits_equal(tree[:4], R.mesh_instance_hits(pods, pl, rays, MI.MINT, MI.MAXT), (start, "back"))
        assert 0 < tree[4].node_tests < never[4].node_tests                        # the tree is in use again


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_statuses(ctx):
    L = R.lib()
    T, pl = MI.standard_mesh(), MM.grid_n(5)
    pods = T.pods()
    poses = MM.as_array(pl)
    ouv = np.ascontiguousarray(np.concatenate([T.origin, T.u, T.v], 1), F)
    lw = C.c_uint32()
    ctx.set_scene(R.Scene(list(FLOOR)))
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 5, None, 0, C.byref(lw)) == E_NO_SCENE
    assert L.rtw_ctx_mesh_top_dump(ctx._h, None, 0, C.byref(lw), None) == E_NO_SCENE
    ctx.set_triangles(pods)
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 5, None, 0, C.byref(lw)) == E_NO_SCENE     # triangles, no placements
    ctx.set_mesh_instances(pl)
    assert L.rtw_ctx_move_mesh_instances(None, poses.ctypes.data, 5, None, 0, None) == E_INVALID
    assert L.rtw_ctx_move_mesh_instances(ctx._h, None, 5, None, T.k, None) == E_INVALID                       # both NULL
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 4, None, 0, None) == E_INVALID
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 6, None, 0, None) == E_INVALID
    assert L.rtw_ctx_move_mesh_instances(ctx._h, None, 0, ouv.ctypes.data, T.k - 1, None) == E_INVALID
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 5, ouv.ctypes.data, T.k + 1, None) == E_INVALID
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 5, None, 12345, None) == 0                # (n_tris is not read without ouv)
    assert L.rtw_ctx_move_mesh_instances(ctx._h, None, 99, ouv.ctypes.data, T.k, C.byref(lw)) == 0 and lw.value == 0
    with pytest.raises(ValueError):
        ctx.move_mesh_instances()
    with pytest.raises(ValueError):
        ctx.move_mesh_instances(12345)                                                                         # a device pointer needs n=
    built = R.mesh_top_dump(pods, pl)[0]
    nodes = np.zeros(len(built), R.TOP_NODE)
    assert L.rtw_ctx_mesh_top_dump(ctx._h, nodes.ctypes.data, len(built) - 1, None, None) == E_INVALID
    assert L.rtw_ctx_mesh_top_dump(ctx._h, nodes.ctypes.data, len(built), C.byref(lw), None) == 0 and lw.value == len(built)
    assert MM.same_bytes(nodes, built)
    # refit_triangles is still refused while placements are set; after clearing them it works as before
    with pytest.raises(R.RtwError) as e:
        ctx.refit_triangles(ouv)
    assert e.value.status == E_INVALID
    assert ctx.move_mesh_instances(MM.turn_and_shift(poses)) == 0
    ctx.set_mesh_instances(None)
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 5, None, 0, None) == E_NO_SCENE
    assert ctx.refit_triangles(ouv) == 0
    assert MM.same_bytes(ctx.triangle_bvh_dump(), R.triangle_bvh_dump(pods)[0])
    # set_triangles and set_scene clear everything
    ctx.set_mesh_instances(pl)
    assert ctx.move_mesh_instances(poses) == 0
    ctx.set_triangles(pods)
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 5, None, 0, None) == E_NO_SCENE
    ctx.set_mesh_instances(pl)
    ctx.set_scene(R.Scene(list(FLOOR)))
    assert L.rtw_ctx_move_mesh_instances(ctx._h, poses.ctypes.data, 5, None, 0, None) == E_NO_SCENE
    assert L.rtw_ctx_mesh_top_dump(ctx._h, None, 0, C.byref(lw), None) == E_NO_SCENE


# ---- stream order ----------------------------------------------------------------------------------------------------------------------------------
def test_a_move_runs_behind_the_producer_of_its_tensor(torch, cycles_per_ms):  # noqa: F811
    """The pose tensor is written by torch behind a delay on the stream of use_torch_stream; move_mesh_instances follows with no synchronise."""
    T, pl = MI.standard_mesh(), MM.grid_n(64)
    pods = T.pods()
    old = MM.as_array(pl)
    new = MM.turn_and_shift(old)
    want = R.mesh_top_refit(pods, pl, new)
    with R.Renderer(0) as r:
        install(r, T, pl)
        before = r.mesh_top_dump()
        hz = Hazard(torch, cycles_per_ms)
        t_in = hz.input(new, stale=old)                       # (a move that ran early reads the old poses: the tree stays `before`)
        _, lw = hz.run(r, "torch-current", lambda: r.move_mesh_instances(t_in))
        assert lw == 0
        nodes, rows = r.mesh_top_dump()
        assert not MM.same_bytes(nodes, before[0])
        assert MM.same_bytes(nodes, want[0]) and MM.same_bytes(rows, want[1])
