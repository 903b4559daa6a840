"""The top-level tree over mesh placements on the GPU: rtw_ctx_mesh_instance_hits, the query kernel's placed path and the
placement build of the render kernels with RTW_OPT_MESH_LIST_MAX = 0 (always the tree) against the host LIST form, the restated path and the
same request with the option at 4294967295 (never).  Parity is bit for bit; no tolerance anywhere."""
import contextlib

import numpy as np
import pytest

import rtw_amd as R
from tests import builds_common as B
from tests import mesh_inst_common as M
from tests import mesh_top_common as MT
from tests.test_gpu_lights import variants
from tests.test_gpu_mesh_instances import (FRAME_QUADS, FRAME_SPHERES, H, SPOILERS, W, differ, frame_camera, frame_params, install, query_scene)

pytestmark = pytest.mark.gpu
F = np.float32
E_NO_SCENE = -6
ALL_SPOILERS = dict(SPOILERS, **{"far origin": [2.0 ** 39, 0.0, 6.0, -1.0, 0.0, 0.0]})


@contextlib.contextmanager
def list_max(r, value):
    """OPT_MESH_LIST_MAX = value for the block (0: always the top-level tree; MT.NEVER: never), the default again afterwards."""
    r.set_option(R.OPT_MESH_LIST_MAX, value)
    try:
        yield
    finally:
        r.set_option(R.OPT_MESH_LIST_MAX, R.MESH_LIST_MAX_DEFAULT)


def standard_case():
    T, pl, rays = M.standard_mesh(), M.standard_placements(), M.standard_rays()
    return T, pl, rays, R.mesh_instance_hits(T.pods(), pl, rays, M.MINT, M.MAXT)


CASES = {"standard": standard_case, "grid 32": lambda: MT.grid_case(32)}


# ---- 1. rtw_ctx_mesh_instance_hits through the tree against the host list form ------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_device_tree_equals_the_host_list_form_in_any_order(gpu, case):
    T, pl, rays, want = CASES[case]()
    install(gpu, T, pl)
    with list_max(gpu, 0):
        for name, order in (("as built", np.arange(len(rays))), ("reversed", np.arange(len(rays))[::-1])):
            t, p, tri, nrm, st = gpu.mesh_instance_hits(rays[order], M.MINT, M.MAXT)
            M.assert_hits_equal((t, p, tri, nrm), tuple(w[order] for w in want), f"{case}, {name}")
            assert st.node_tests > 0


@pytest.mark.parametrize("kind", list(ALL_SPOILERS))
@pytest.mark.parametrize("case", list(CASES))
def test_one_spoiler_lane_per_wave_changes_no_other_lane(gpu, case, kind):
    """Every wave of 64 holds one spoiler at lane 0, 31, 32 or 63 -- a ray the top-level tree refuses, or one with zero components, which it
    answers --: the 63 mates keep the host list form's bits, and so does the spoiler."""
    T, pl, rays, want = CASES[case]()
    install(gpu, T, pl)
    launch = rays.copy()
    pos = np.array([64 * w + (0, 31, 32, 63)[w % 4] for w in range(len(rays) // 64)])
    launch[pos] = np.array(ALL_SPOILERS[kind], F)
    want_sp = R.mesh_instance_hits(T.pods(), pl, launch[pos[:8]], M.MINT, M.MAXT)       # (one spoiler ray: eight copies answer for all)
    with list_max(gpu, 0):
        t, p, tri, nrm, _ = gpu.mesh_instance_hits(launch, M.MINT, M.MAXT)
    mates = np.setdiff1d(np.arange(len(rays)), pos)
    M.assert_hits_equal((t[mates], p[mates], tri[mates], nrm[mates]), tuple(w[mates] for w in want), f"{case}, {kind}: the mates")
    for j in range(0, len(pos), 8):
        sl = pos[j:j + 8]
        M.assert_hits_equal((t[sl], p[sl], tri[sl], nrm[sl]), tuple(w[:len(sl)] for w in want_sp), f"{case}, {kind}: the spoilers")


def test_the_tree_prunes_on_the_grid_of_32(gpu):
    T, pl, rays, want = MT.grid_case(32)
    n = len(pl)
    install(gpu, T, pl)
    with list_max(gpu, 0):
        tree = gpu.mesh_instance_hits(rays, M.MINT, M.MAXT)
    with list_max(gpu, MT.NEVER):
        lst = gpu.mesh_instance_hits(rays, M.MINT, M.MAXT)
    M.assert_hits_equal(tree[:4], want, "tree")
    M.assert_hits_equal(lst[:4], want, "list order")
    print(f"g = 32: node visits per ray {tree[4].node_tests / len(rays):.1f} (tree) / {lst[4].node_tests / len(rays):.1f} (list order), "
          f"triangle tests per ray {tree[4].quad_tests / len(rays):.1f} / {lst[4].quad_tests / len(rays):.1f}")
    assert tree[4].node_tests / len(rays) < n / 4
    assert lst[4].node_tests >= MT.ordinary(rays).sum() * n               # at least the mesh's root per placement and ordinary ray
    assert tree[4].quad_tests <= lst[4].quad_tests


def test_the_default_switch(gpu):
    """Six placements with no option set walk the list exactly as under `never`; 64 placements under 0 count other node visits, same outputs."""
    T, pl, rays, want = standard_case()
    install(gpu, T, pl)
    default = gpu.mesh_instance_hits(rays, M.MINT, M.MAXT)
    with list_max(gpu, MT.NEVER):
        never = gpu.mesh_instance_hits(rays, M.MINT, M.MAXT)
    assert (default[4].node_tests, default[4].quad_tests) == (never[4].node_tests, never[4].quad_tests)
    M.assert_hits_equal(default[:4], never[:4], "6 placements: default against never")
    T, pl, rays, want = MT.grid_case(8)
    install(gpu, T, pl)
    with list_max(gpu, MT.NEVER):
        never = gpu.mesh_instance_hits(rays, M.MINT, M.MAXT)
    with list_max(gpu, 0):
        tree = gpu.mesh_instance_hits(rays, M.MINT, M.MAXT)
    M.assert_hits_equal(tree[:4], never[:4], "64 placements: tree against never")
    M.assert_hits_equal(tree[:4], want, "64 placements: tree against the host list form")
    assert tree[4].node_tests != never[4].node_tests and tree[4].node_tests > 0


# ---- 2. scene_hits and depth_map -------------------------------------------------------------------------------------------------------------------
def grid_query_scene():
    """3 spheres, 1 quad and 1 Euler-rotated instance about the 8 x 8 grid (x, z in -10.5 .. 10.5 about (0, 0, 6))."""
    sp = [R.Sphere.new((0.3, 0.2, 6.4), 0.8, (0.5, 0.5, 0.5), R.SCATTER_M),
          R.Sphere.new((-4.5, 1.4, 1.5), 0.9, (0.5, 0.5, 0.5), R.METALLIC_M),
          R.Sphere.new((6.0, 0.5, 9.6), 0.7, (0.5, 0.5, 0.5), R.GLASS_M)]
    quads = [R.Quad.new((-14.0, -2.2, -8.0), (28.0, 0.0, 0.0), (0.0, 0.0, 28.0))]
    box = R.Instance.new_box((-0.7, -0.7, -0.7), (0.7, 0.7, 0.7), (0.7, 0.7, 0.7), R.SCATTER_M)
    box.rotate((0.3, 0.5, -0.2))
    box.translate((3.0, 0.2, 4.4))
    return R.Scene(sp, quads=quads, instances=[box])


def test_scene_hits_and_depth_map_are_the_same_under_both_options(gpu):
    T, pl, rays, _ = MT.grid_case(8)
    scene = grid_query_scene()
    base = scene.n_spheres + scene.n_quads + scene.n_instances
    install(gpu, T, pl, scene)
    w, h = 24, 16
    cam = R.camera2_new(w / h, (0.0, 3.0, -12.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 60.0, 0.0)
    assert (R.depth_rays(cam, w, h)[:, 3].reshape(h, w)[:, w // 2] == 0).all()     # the zero column
    out = {}
    for value in (0, MT.NEVER):
        with list_max(gpu, value):
            out[value] = (gpu.scene_hits(rays, M.MINT, M.MAXT, accel=R.ACCEL_BVH, normals=True),
                          gpu.depth_map(cam, w, h, M.MINT, M.MAXT, accel=R.ACCEL_BVH, ids=True, normals=True))
    (t0, i0, n0, s0), (d0, ids0, dn0, ds0) = out[0]
    (t1, i1, n1, s1), (d1, ids1, dn1, ds1) = out[MT.NEVER]
    assert not differ(t0, t1).any() and np.array_equal(i0, i1) and not differ(n0, n1).any()
    assert not differ(d0, d1).any() and np.array_equal(ids0, ids1) and not differ(dn0, dn1).any()
    assert (i0 >= base).sum() >= 500 and ((i0 >= 0) & (i0 < base)).sum() >= 100 and (i0 < 0).sum() >= 100    # the group wins, loses, rays miss
    assert (ids0 >= base).sum() >= 20
    assert s0.node_tests < s1.node_tests and ds0.node_tests != ds1.node_tests


# ---- 3. frames ----------------------------------------------------------------------------------------------------------------------------------
def grid_frame_scene(moving=False):
    """frame_scene's spheres and quad with 16 placements: the 4 x 4 grid drawn together about (0.3, 0.2, 3.6), several to a pixel."""
    spheres = [dict(s) for s in FRAME_SPHERES]
    if moving:
        spheres[1]["velocity"] = [0.0, 0.4, 0.0]
    pl = [([0.3 + 0.45 * p[0], 0.2 + p[1] * 0.5, 3.6 + 0.45 * (p[2] - 6.0)], q) for p, q in MT.grid(4)]
    return M.MeshScene(M.standard_mesh(), pl, spheres, FRAME_QUADS, background=(0.5, 0.6, 0.8))


@pytest.mark.parametrize("sampler", [R.SAMPLER_CENTRES, R.SAMPLER_ROW])
@pytest.mark.parametrize("moving", [False, True])
def test_frames_through_the_tree_equal_the_restated_path(gpu, moving, sampler):
    ms = grid_frame_scene(moving)
    ms.install(gpu, 0.0, 1.0)
    cam, p = frame_camera(moving), frame_params(ms, sampler)
    ref, seg = M.render(ms, cam, p, ("top frame", moving))
    assert np.isfinite(ref).all()
    with list_max(gpu, MT.NEVER):
        never = variants(gpu, cam, p, build=(12, moving, True))
    with list_max(gpu, 0):
        tree = variants(gpu, cam, p, build=(12, moving, True))           # (variants asserts the SPEC 12 tag of every render: builds_common)
    for name, (img, st) in tree.items():
        bad = differ(img, ref)
        print(f"moving {moving} sampler {sampler} [{name}]: {int(bad.sum())} values differ, node tests {st.node_tests} / {never[name][1].node_tests}")
        assert not bad.any(), (name, int(bad.sum()))
        assert not differ(img, never[name][0]).any() and st.segments == seg == never[name][1].segments
    B.ran(gpu, B.bvh(moving, 0, 12, True), "the last variant: the tree with global nodes")
    assert tree["list"][1].node_tests == 0 == never["list"][1].node_tests          # RTW_ACCEL_BRUTE: no tree of either kind
    for name in ("bvh as shipped", "tree, lds nodes", "tree, global nodes"):
        assert tree[name][1].node_tests != never[name][1].node_tests


# ---- 4. lifecycle ---------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_of_the_top_level_tree(gpu, rtw):
    ms = grid_frame_scene()
    cam, p = frame_camera(), frame_params(ms, R.SAMPLER_CENTRES)
    p.accel = R.ACCEL_BVH
    rays = M.standard_rays(placements=ms.placements)[:1024]
    hits = lambda r, pl: (r.mesh_instance_hits(rays, M.MINT, M.MAXT)[:4], R.mesh_instance_hits(ms.T.pods(), pl, rays, M.MINT, M.MAXT))
    with list_max(gpu, 0):
        ms.install(gpu)
        whole, st_whole = gpu.render(cam, p)
        M.assert_hits_equal(*hits(gpu, ms.placements), "16 placements")
        # set_mesh_instances twice with different counts: the second tree replaces the first
        gpu.set_mesh_instances(ms.placements[:5])
        M.assert_hits_equal(*hits(gpu, ms.placements[:5]), "then 5")
        gpu.set_mesh_instances(ms.placements)
        M.assert_hits_equal(*hits(gpu, ms.placements), "then 16 again")
        assert not differ(gpu.render(cam, p)[0], whole).any()
        # set_triangles / set_scene clear the placements and their tree
        for clear in (lambda: gpu.set_triangles(ms.T.pods()), lambda: (gpu.set_scene(ms.scene), gpu.set_triangles(ms.T.pods()))):
            ms.install(gpu)
            clear()
            with pytest.raises(rtw.RtwError) as e:
                gpu.mesh_instance_hits(rays[:64], M.MINT, M.MAXT)
            assert e.value.status == E_NO_SCENE
            gpu.render(cam, p)                                            # (the plain triangle build: nothing of the tree is read)
            assert gpu.last_render_build() in (B.brute(False, 8, True), B.bvh(False, 1, 8, True))
        # two contexts on one GPU with different placement sets
        ms.install(gpu)
        with rtw.Renderer(0) as other:
            other.set_option(R.OPT_MESH_LIST_MAX, 0)
            ms.install(other)
            other.set_mesh_instances(ms.placements[:7])
            M.assert_hits_equal(*hits(other, ms.placements[:7]), "the other context: 7")
            M.assert_hits_equal(*hits(gpu, ms.placements), "this context: still 16")
            assert differ(other.render(cam, p)[0], whole).any()
        assert not differ(gpu.render(cam, p)[0], whole).any()
    # a MultiRenderer row partition under the option equals the unsplit frame
    with rtw.MultiRenderer([0, 0]) as m:
        m.set_option(R.OPT_MESH_LIST_MAX, 0)
        m.set_scene(ms.scene)
        m.set_triangles(ms.T.pods())
        m.set_mesh_instances(ms.placements)
        out = m.render(cam, p)
    assert not differ(out[0], whole).any()
    with list_max(gpu, MT.NEVER):
        never, st_never = gpu.render(cam, p)
    assert not differ(never, whole).any() and st_never.node_tests != st_whole.node_tests
