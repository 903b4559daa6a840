"""Mesh placements on the GPU: rtw_ctx_mesh_instance_hits, the query kernel's placed path, depth_map, and the placement build of the render
kernels (SPEC 12) against the host form and the restatement of tests/mesh_inst_common.py.  Parity is bit for bit (a NaN in both counts as
equal: a NaN's payload is not part of the contract); no tolerance anywhere."""
import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as M
from tests import quat_common as QC
from tests.test_gpu_lights import variants
from tests.test_gpu_scene_hits import oracle_hits

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID, E_NO_SCENE = -1, -6
ACCELS = [R.ACCEL_BRUTE, R.ACCEL_BVH]
RUST2 = R.INTEGRATOR_RUST2


def differ(a, b):
    return ~M.same_nan(a, b)


@pytest.fixture(scope="module")
def standard():
    """The standard mesh, placements and rays, and the host form's answer (test_mesh_instances_cpu.py pins it to the restatement)."""
    T, pl, rays = M.standard_mesh(), M.standard_placements(), M.standard_rays()
    return T, pl, rays, R.mesh_instance_hits(T.pods(), pl, rays, M.MINT, M.MAXT)


def install(gpu, T, pl, scene=None):
    gpu.set_scene(scene if scene is not None else R.Scene([R.Sphere.new((0.0, -60.0, 0.0), 0.5, (0.5, 0.5, 0.5), R.SCATTER_M)]))
    gpu.set_triangles(T.pods())
    gpu.set_mesh_instances(pl)


# ---- 1. rtw_ctx_mesh_instance_hits against the host form ----------------------------------------------------------------------------------------
SPOILERS = {
    "refused by tri_ray_ordinary in the local frame": [2.0 ** 41, 0.0, 0.0, -1.0, 0.0, 0.0],     # |o| beyond the cull's reach in every placement's frame
    "NaN": [0.0, 0.0, -5.0, 0.0, np.nan, 1.0],
    "zero component": [0.0, 0.1, -5.0, 0.0, 0.0, 1.0],
}


@pytest.mark.parametrize("accel", ACCELS)
def test_device_form_equals_the_host_form_in_any_order(gpu, standard, accel):
    T, pl, rays, want = standard
    install(gpu, T, pl)
    for name, order in (("as built", np.arange(len(rays))), ("reversed", np.arange(len(rays))[::-1])):
        t, p, tri, nrm, st = gpu.mesh_instance_hits(rays[order], M.MINT, M.MAXT, accel=accel)
        M.assert_hits_equal((t, p, tri, nrm), tuple(w[order] for w in want), f"{name}, accel {accel}")
        assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
        if accel == R.ACCEL_BRUTE:
            assert st.quad_tests == len(rays) * len(pl) * T.k
        else:
            assert st.quad_tests < len(rays) * len(pl) * T.k // 4     # the tree prunes (the NaN ray alone walks the list)


@pytest.mark.parametrize("kind", list(SPOILERS))
@pytest.mark.parametrize("accel", ACCELS)
def test_one_spoiler_lane_per_wave_changes_no_other_lane(gpu, standard, accel, kind):
    """Every wave of 64 holds one spoiler at lane 0, 31, 32 or 63: the 63 mates keep the host form's bits, the spoiler answers what the host
    form answers for it.  Under the tree a refused ray walks the list of every placement."""
    T, pl, rays, want = standard
    install(gpu, T, pl)
    launch = rays.copy()
    pos = np.array([64 * w + (0, 31, 32, 63)[w % 4] for w in range(len(rays) // 64)])
    launch[pos] = np.array(SPOILERS[kind], F)
    want_sp = R.mesh_instance_hits(T.pods(), pl, launch[pos], M.MINT, M.MAXT)
    t, p, tri, nrm, st = gpu.mesh_instance_hits(launch, M.MINT, M.MAXT, accel=accel)
    mates = np.setdiff1d(np.arange(len(rays)), pos)
    M.assert_hits_equal((t[mates], p[mates], tri[mates], nrm[mates]), tuple(w[mates] for w in want), f"{kind}: the mates, accel {accel}")
    M.assert_hits_equal((t[pos], p[pos], tri[pos], nrm[pos]), want_sp, f"{kind}: the spoilers, accel {accel}")
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
    if accel == R.ACCEL_BVH and kind != "zero component":
        alone = gpu.mesh_instance_hits(launch[pos], M.MINT, M.MAXT, accel=accel)[4]
        assert alone.node_tests == 0 and alone.quad_tests == len(pos) * len(pl) * T.k      # the list is walked for the refused rays
    if kind == "zero component":
        assert (want_sp[1] == 0).all()                               # ... and the zero-safe walk finds what the list finds


# ---- 2. scene_hits and depth_map ---------------------------------------------------------------------------------------------------------------
def query_scene():
    """3 spheres, 1 quad and 1 Euler-rotated instance about the standard placements."""
    sp = [R.Sphere.new((0.3, 0.2, 0.4), 0.8, (0.5, 0.5, 0.5), R.SCATTER_M),          # inside placement 0, poking out of it
          R.Sphere.new((2.0, 1.4, 2.0), 0.7, (0.5, 0.5, 0.5), R.METALLIC_M),
          R.Sphere.new((-3.0, 0.5, 2.6), 0.5, (0.5, 0.5, 0.5), R.GLASS_M)]
    quads = [R.Quad.new((-5.0, -1.2, -2.0), (10.0, 0.0, 0.0), (0.0, 0.0, 8.0))]
    box = R.Instance.new_box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (0.7, 0.7, 0.7), R.SCATTER_M)
    box.rotate((0.3, 0.5, -0.2))
    box.translate((3.0, 0.2, 1.2))                                                   # overlaps placement 1
    return R.Scene(sp, quads=quads, instances=[box])


def combine(first, mesh, base):
    """The group rule: the placement group replaces the result of the first three groups only when strictly closer."""
    t, idx, nrm = (x.copy() for x in first)
    mt, mp, _, mn = mesh
    with np.errstate(invalid="ignore"):
        take = (mp >= 0) & ((idx < 0) | (t > mt))
    t[take], idx[take], nrm[take] = mt[take], base + mp[take], mn[take]
    return t, idx, nrm, take


@pytest.fixture(scope="module")
def scene_reference(oracle, standard):
    T, pl, rays, mesh = standard
    scene = query_scene()
    sub = rays[::4]                                                   # 1024 rays: the oracle answers them one by one
    first = oracle_hits(oracle, scene, sub, 0.0, M.MINT, M.MAXT)
    return scene, sub, combine(first, tuple(m[::4] for m in mesh), scene.n_spheres + scene.n_quads + scene.n_instances)


@pytest.mark.parametrize("accel", ACCELS)
def test_scene_hits_combine_the_oracle_and_the_host_form(gpu, standard, scene_reference, accel):
    T, pl, _, _ = standard
    scene, rays, (wt, widx, wn, take) = scene_reference
    assert take.sum() >= 100 and ((widx >= 0) & ~take).sum() >= 100 and (widx < 0).sum() >= 100      # the group wins, loses, and rays miss
    install(gpu, T, pl, scene)
    t, idx, nrm, st = gpu.scene_hits(rays, M.MINT, M.MAXT, accel=accel, normals=True)
    bad = differ(t, wt) | (idx != widx) | differ(nrm, wn).any(axis=1)
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:5])
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)


@pytest.mark.parametrize("accel", ACCELS)
def test_depth_map_with_a_zero_column_in_every_wave(gpu, oracle, standard, accel):
    """34 x 15, an axis-aligned camera: pixel 17 of every row has d.x == 0 exactly, which the identity placements hand to the tree walk as it
    is.  Tree and list give the oracle's first three groups combined with the host form."""
    T, pl, _, _ = standard
    scene = query_scene()
    w, h = 34, 15
    cam = R.camera2_new(w / h, (0.0, 0.0, -7.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 60.0, 0.0)
    rays = R.depth_rays(cam, w, h)
    assert (rays[:, 3].reshape(h, w)[:, w // 2] == 0).all()
    first = oracle_hits(oracle, scene, rays, 0.0, M.MINT, M.MAXT)
    mesh = R.mesh_instance_hits(T.pods(), pl, rays, M.MINT, M.MAXT)
    wt, widx, wn, take = combine(first, mesh, scene.n_spheres + scene.n_quads + scene.n_instances)
    assert take.reshape(h, w)[:, w // 2].any() and take.sum() >= 30
    install(gpu, T, pl, scene)
    depth, ids, nrm, st = gpu.depth_map(cam, w, h, M.MINT, M.MAXT, accel=accel, ids=True, normals=True)
    wd = np.where(widx >= 0, wt, F(F(M.MAXT) * F(1.6))).astype(F)
    assert not differ(depth.reshape(-1), wd).any() and np.array_equal(ids.reshape(-1), widx) and not differ(nrm.reshape(-1, 3), wn).any()
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
    if accel == R.ACCEL_BVH:
        assert st.quad_tests < w * h * (len(pl) * T.k) // 4            # the zero column does not fall back to testing every triangle


# ---- 3. frames, bounce for bounce, through every kernel of the build -------------------------------------------------------------------------------
W, H = 24, 16
FRAME_SPHERES = [
    {"origin": [0.0, -101.2, 3.0], "radius": 100.0, "material": "lambertian", "color": [0.6, 0.6, 0.5], "emitted": [0.0, 0.0, 0.0]},
    {"origin": [-1.6, 0.1, 2.2], "radius": 0.6, "material": "mirror", "color": [0.9, 0.8, 0.7], "emitted": [0.0, 0.0, 0.0]},
    {"origin": [2.2, 2.4, 3.0], "radius": 0.7, "material": "lambertian", "color": [1.0, 1.0, 1.0], "emitted": [6.0, 5.0, 4.0]},
]
FRAME_QUADS = [{"origin": [-4.0, -1.2, 6.0], "u": [8.0, 0.0, 0.0], "v": [0.0, 5.0, 0.0], "material": "lambertian", "color": [0.4, 0.5, 0.7],
                "emitted": [0.0, 0.0, 0.0]}]


def frame_scene(moving=False, world_dir=False):
    spheres = [dict(s) for s in FRAME_SPHERES]
    if moving:
        spheres[1]["velocity"] = [0.0, 0.4, 0.0]
    return M.MeshScene(M.standard_mesh(), M.standard_placements()[:5], spheres, FRAME_QUADS, background=(0.5, 0.6, 0.8), world_dir=world_dir)


def frame_camera(moving=False):
    cam = R.camera2_new(W / H, (0.3, 0.6, -5.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 55.0, 0.0)
    if moving:
        cam.time0, cam.shutter = 0.0, 1.0
    return cam


def frame_params(ms, sampler, seed=7):
    p = ms.params(W, H, RUST2, 4, samples=4, seed=seed)
    p.sampler = sampler
    return p


@pytest.mark.parametrize("sampler", [R.SAMPLER_CENTRES, R.SAMPLER_ROW])
@pytest.mark.parametrize("moving", [False, True])
def test_bounce_for_bounce(gpu, moving, sampler):
    """render_brute<MOVING, 12, GEOM> and render_bvh<MOVING, {global, LDS nodes}, 12, GEOM> against the restated path, 4 samples, depth 4: the
    mesh carries Lambertian, Mirror and MirrorGlass triangles, so the direction a placed material reads decides pixels."""
    ms = frame_scene(moving)
    ms.install(gpu, 0.0, 1.0)
    cam, p = frame_camera(moving), frame_params(ms, sampler)
    ref, seg = M.render(ms, cam, p, ("frame", moving))
    assert np.isfinite(ref).all()
    res = variants(gpu, cam, p, build=(12, moving, True))
    for name, (img, st) in res.items():
        bad = differ(img, ref)
        print(f"moving {moving} sampler {sampler} [{name}]: {int(bad.sum())} values differ, segments {st.segments} / {seg}, node tests {st.node_tests}")
        assert not bad.any(), (name, int(bad.sum()))
        assert st.segments == seg
    # the mesh's own tree counts node visits in every variant but the list; the sphere tree adds to them where it is forced
    assert res["list"][1].node_tests == 0 and res["bvh as shipped"][1].node_tests > 0
    assert res["tree, lds nodes"][1].node_tests > res["bvh as shipped"][1].node_tests
    assert res["tree, global nodes"][1].node_tests > res["bvh as shipped"][1].node_tests


def test_the_world_direction_would_give_another_frame(gpu):
    """Hit.r stays local: a restatement that hands the material the world direction differs from the device's frame."""
    ms, wrong = frame_scene(), frame_scene(world_dir=True)
    cam, p = frame_camera(), frame_params(ms, R.SAMPLER_CENTRES)
    ref, _ = M.render(ms, cam, p, ("frame", False))
    other, _ = M.render(wrong, cam, p, ("frame", False))
    assert differ(ref, other).any(axis=2).sum() >= 10
    ms.install(gpu)
    img, _ = gpu.render(cam, p)
    assert not differ(img, ref).any()


def test_row_partition_and_two_contexts_equal_the_unsplit_frame(gpu, rtw):
    ms = frame_scene()
    ms.install(gpu)
    cam, p = frame_camera(), frame_params(ms, R.SAMPLER_ROW)
    p.accel = R.ACCEL_BVH
    whole, _ = gpu.render(cam, p)
    p.accel = R.ACCEL_BRUTE
    assert not differ(gpu.render(cam, p)[0], whole).any()              # tree == list
    p.accel = R.ACCEL_BVH
    parts = []
    for k in range(3):
        q = R.RtwParams.from_buffer_copy(p)
        q.row_block, q.part_index, q.part_count = 2, k, 3
        parts.append(gpu.render(cam, q)[0])
    rows = [[] for _ in range(3)]
    for j in range(H):
        rows[(j // 2) % 3].append(j)
    joined = np.empty_like(whole)
    for k in range(3):
        joined[rows[k]] = parts[k]
    assert not differ(joined, whole).any()
    with rtw.MultiRenderer([0, 0]) as m:
        m.set_scene(ms.scene)
        m.set_triangles(ms.T.pods())
        m.set_mesh_instances(ms.placements)
        out = m.render(cam, p)
    assert not differ(out[0], whole).any()


# ---- 4. lifecycle and refusals -----------------------------------------------------------------------------------------------------------------
def test_set_triangles_and_set_scene_clear_the_placements(gpu, rtw):
    ms = frame_scene()
    cam, p = frame_camera(), frame_params(ms, R.SAMPLER_CENTRES)
    with rtw.Renderer(0) as fresh:                                    # the plain triangle build on a context that never saw a placement
        ms.install(fresh, placements=False)
        plain, st_plain = fresh.render(cam, p)
    ms.install(gpu)
    placed, _ = gpu.render(cam, p)
    assert differ(placed, plain).any()
    for clear in (lambda: gpu.set_triangles(ms.T.pods()), lambda: gpu.set_mesh_instances(None),
                  lambda: (gpu.set_scene(ms.scene), gpu.set_triangles(ms.T.pods()))):
        ms.install(gpu)
        clear()
        again, st = gpu.render(cam, p)
        assert not differ(again, plain).any() and st.segments == st_plain.segments
        with pytest.raises(rtw.RtwError) as e:
            gpu.mesh_instance_hits(M.standard_rays()[:64], M.MINT, M.MAXT)
        assert e.value.status == E_NO_SCENE
    ms.install(gpu)
    assert not differ(gpu.render(cam, p)[0], placed).any()


def test_what_is_not_built_is_refused_and_leaves_the_context_usable(gpu, rtw):
    ms = frame_scene()
    ms.install(gpu)
    cam, p = frame_camera(), frame_params(ms, R.SAMPLER_CENTRES)
    good, _ = gpu.render(cam, p)

    def status(fn):
        with pytest.raises(rtw.RtwError) as e:
            fn()
        return e.value.status

    for integ in (R.INTEGRATOR_GRADIENT, R.INTEGRATOR_BG_COLOR, R.INTEGRATOR_NORMAL, R.INTEGRATOR_FLAG):
        q = R.RtwParams.from_buffer_copy(p)
        q.integrator = integ
        assert status(lambda: gpu.render(cam, q)) == E_INVALID
        assert not differ(gpu.render(cam, p)[0], good).any()
    # the setter: bad placements, too many, a textured mesh, no triangles -- each leaves the placements that were set
    assert status(lambda: gpu.set_mesh_instances([([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])])) == E_INVALID
    assert status(lambda: gpu.set_mesh_instances([([np.nan, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])])) == E_INVALID
    assert not differ(gpu.render(cam, p)[0], good).any()
    textured = ms.T.pods()
    textured[3].pod.tex = 0
    tex_scene = R.Scene([R.Sphere.new((0.0, -60.0, 0.0), 0.5, (0.5, 0.5, 0.5), R.SCATTER_M)], textures=[np.full((2, 2, 3), 0.5, F)])
    gpu.set_scene(tex_scene)
    gpu.set_triangles(textured)
    assert status(lambda: gpu.set_mesh_instances(ms.placements)) == E_INVALID
    gpu.set_mesh_instances(None)
    gpu.set_triangles(None)
    assert status(lambda: gpu.set_mesh_instances(ms.placements)) == E_NO_SCENE
    # instance rotations in the same context
    g = QC.golden()
    qs = QC.fixture_scene(g)
    qs.install(gpu)
    gpu.set_triangles(ms.T.pods())
    gpu.set_mesh_instances(ms.placements)
    assert status(lambda: gpu.render(QC.camera(g, 16, 16), qs.params(16, 16, RUST2, 2))) == E_INVALID
    ms.install(gpu)
    assert not differ(gpu.render(cam, p)[0], good).any()


def test_two_contexts_on_one_gpu_keep_their_own_placements(gpu, rtw):
    ms = frame_scene()
    cam, p = frame_camera(), frame_params(ms, R.SAMPLER_CENTRES)
    ms.install(gpu)
    a, _ = gpu.render(cam, p)
    with rtw.Renderer(0) as other:
        ms.install(other)
        other.set_mesh_instances(ms.placements[:2])
        b, _ = other.render(cam, p)
        assert not differ(gpu.render(cam, p)[0], a).any()
        other.set_mesh_instances(ms.placements)
        assert not differ(other.render(cam, p)[0], a).any()
    assert differ(a, b).any()
