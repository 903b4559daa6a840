"""Rust2's quaternion-rotated instances on the GPU: the query kernel, depth_map and the quaternion build of the render kernels (SPEC 11)
against the restatement of tests/quat_common.py.  Parity is bit for bit (NaN in both counts as equal: a NaN's payload is not part of the
contract); no tolerance anywhere.  The fixture is tests/golden/rust2_rotation_scene.json, Rust2's rotation_test as data."""
import numpy as np
import pytest

import rtw_amd as R
from tests import quat_common as Q
from tests.test_gpu_lights import variants

pytestmark = pytest.mark.gpu
F = np.float32
CAST, BIASED, RUST2 = Q.CAST, Q.BIASED, Q.RUST2
E_INVALID = -1
SPHERE = {"origin": [1.6, -0.4, 4.2], "radius": 0.45, "material": "lambertian", "color": [0.7, 0.5, 0.3], "emitted": [0.0, 0.0, 0.0]}
SPHERE2 = {"origin": [-2.6, 0.9, 5.5], "radius": 0.3, "material": "lambertian", "color": [0.3, 0.6, 0.7], "emitted": [0.0, 0.0, 0.0]}
# an emissive quad outside the box, to its right and above: the box's own faces turned away from it are in its shadow
LIGHT_QUAD = {"origin": [2.0, 2.2, 3.0], "u": [1.0, 0.0, 0.0], "v": [0.0, 0.0, 1.0], "material": "lambertian", "color": [1.0, 1.0, 1.0],
              "emitted": [8.0, 7.0, 6.0]}


def differ(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))


def sphere_field(n=60, seed=4):
    rng = np.random.default_rng(seed)
    return [{"origin": [float(rng.uniform(-4, 3)), float(rng.uniform(-2, 2)), float(rng.uniform(2.5, 8))], "radius": float(rng.uniform(0.1, 0.4)),
             "material": "lambertian", "color": [0.5, 0.5, 0.5], "emitted": [0.0, 0.0, 0.0]} for _ in range(n)]


def query_rays(g, seed=2):
    """4096 random rays about the camera towards the box, and the edge rays: parallel to a face, through a box edge, from inside the box, with a
    -0 direction component, with an infinite origin component."""
    rng = np.random.default_rng(seed)
    c = np.array(g["translation"])
    o = rng.normal(scale=0.5, size=(4096, 3))
    d = (c + rng.normal(scale=1.3, size=(4096, 3)) - o) * rng.uniform(0.2, 3.0, size=(4096, 1))      # not normalised
    q = Q.f32(g["quaternion_wxyz"])
    back = (q * Q.f32([1, -1, -1, -1])).astype(F)                   # a local vector v sits in the world at about rotate(conj q, v)
    world = lambda v: Q.rotate(back, Q.f32(v)).astype(np.float64)
    edge = [
        (c + world([-3, 0.3, 1.0]), world([1, 0, 0])),              # in the plane of the face z = +1, parallel to it
        (c + world([-3, 0.3, 0.5]), world([1, 0, 0])),              # parallel to four faces, through two
        (np.zeros(3), c + world([1, 0.2, 1])),                      # through the edge x = z = 1
        (np.zeros(3), c + world([1, 1, -1])),                       # through a corner
        (c, np.array([0.3, 0.2, 1.0])), (c, np.array([-1.0, 0.0, 0.0])),                       # from inside the box
        (np.zeros(3), np.array([-0.2, -0.0, 1.0])), (np.zeros(3), np.array([-0.0, 0.1, 1.0])),  # a -0 direction component
        (np.array([np.inf, 0.0, 0.0]), np.array([-1.0, 0.0, 0.2])), (np.array([0.0, -np.inf, 0.0]), np.array([-0.2, 1.0, 1.0])),
    ]
    o = np.concatenate([o, np.array([e[0] for e in edge])])
    d = np.concatenate([d, np.array([e[1] for e in edge])])
    return o.astype(F), d.astype(F)


def check_query(gpu, qs, o, d, accel, what):
    ref = qs.closest(o, d)
    t, idx, nrm, st = gpu.scene_hits(np.concatenate([o, d], axis=1), float(qs.mint), float(qs.maxt), accel=accel, normals=True)
    miss = ~ref["found"]
    exp_t = np.where(miss, F(np.inf), ref["t"]).astype(F)
    bad_t, bad_n = differ(t, exp_t), differ(nrm, ref["normal"]).any(axis=1)
    print(f"{what}: {len(o)} rays, {int(ref['found'].sum())} hit ({int((ref['idx'] >= len(qs.spheres) + len(qs.quads)).sum())} an instance), "
          f"{int(bad_t.sum())} t / {int((idx != ref['idx']).sum())} indices / {int(bad_n.sum())} normals differ")
    assert not bad_t.any() and np.array_equal(idx, ref["idx"]) and not bad_n.any()
    assert np.array_equal(idx < 0, miss) and (nrm[miss] == 0).all()
    return ref, st


# ---- 1. the query kernel ----------------------------------------------------------------------------------------------------------------------
def test_query_kernel_fixture_and_edge_rays(gpu):
    g = Q.golden()
    qs = Q.fixture_scene(g)
    qs.install(gpu)
    o, d = query_rays(g)
    ref, _ = check_query(gpu, qs, o, d, R.ACCEL_BRUTE, "fixture")
    assert 0.2 < ref["found"][:4096].mean() < 0.95
    assert ref["found"][4096 + 4] and ref["found"][4096 + 5]          # from inside the box: a face is hit from behind
    assert len(set((~ref["member"][ref["found"]]).tolist())) >= 4     # most faces are seen by some ray
    # without the rotations the same rays see the unturned box
    gpu.set_instance_rotations(None)
    t0, idx0, _ = gpu.scene_hits(np.concatenate([o, d], axis=1), float(qs.mint), float(qs.maxt), accel=R.ACCEL_BRUTE)
    assert (np.isfinite(t0[:4096]) != ref["found"][:4096]).any()


def test_query_kernel_instance_against_the_sphere_tree(gpu):
    g = Q.golden()
    qs = Q.fixture_scene(g, spheres=sphere_field())
    qs.install(gpu)
    o, d = query_rays(g, seed=3)
    gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
    try:
        ref, st = check_query(gpu, qs, o, d, R.ACCEL_BVH, "fixture + 60 spheres, tree forced")
    finally:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    assert st.node_tests > 0
    n_s = len(qs.spheres)
    assert (ref["idx"] == n_s).sum() > 100 and ((ref["idx"] >= 0) & (ref["idx"] < n_s)).sum() > 100      # the instance wins and loses
    check_query(gpu, qs, o, d, R.ACCEL_BRUTE, "fixture + 60 spheres, list")


def test_query_kernel_two_overlapping_instances_general_quaternion(gpu):
    g = Q.golden()
    second = Q.box_instance(g, quat=[0.3, -0.5, 0.7, 0.1])           # unnormalised, all four components
    second["translation"] = [-0.4, 0.3, 5.4]
    second["spheres"] = [{"origin": [0.1, 0.2, -0.1], "radius": 1.35, "material": "lambertian", "color": [0.4] * 3, "emitted": [0.0] * 3}]
    qs = Q.fixture_scene(g, extra_instances=[second])
    qs.install(gpu)
    o, d = query_rays(g, seed=5)
    ref, _ = check_query(gpu, qs, o, d, R.ACCEL_BRUTE, "two instances")
    assert (ref["idx"] == 0).sum() > 100 and (ref["idx"] == 1).sum() > 100
    assert ((ref["idx"] == 1) & (ref["member"] >= 0)).sum() > 20     # the sphere member is hit: its normal is unit(p - c), rotated


# ---- 2. depth_map -----------------------------------------------------------------------------------------------------------------------------
def test_depth_map_of_the_fixture(gpu):
    g = Q.golden()
    qs = Q.fixture_scene(g)
    qs.install(gpu)
    cam = Q.camera(g, 48, 48)
    ref = qs.closest(*Q.depth_rays(cam, 48, 48))
    depth, ids, nrm, _ = gpu.depth_map(cam, 48, 48, float(qs.mint), float(qs.maxt), accel=R.ACCEL_BRUTE, ids=True, normals=True)
    exp = np.where(ref["found"], ref["t"], F(qs.maxt * F(1.6))).astype(F).reshape(48, 48)
    assert not differ(depth, exp).any() and np.array_equal(ids.reshape(-1), ref["idx"]) and not differ(nrm.reshape(-1, 3), ref["normal"]).any()
    assert 0.1 <= ref["found"].mean() <= 0.9


# ---- 3. depth-1 known answer --------------------------------------------------------------------------------------------------------------------
def test_depth_one_known_answer(gpu):
    """INTEGRATOR_RUST2, depth 1, SAMPLER_CENTRES, 4 samples, 48 x 48: a pixel whose four sample rays all hit the box is
    gamma(emitted + background * multiplied) = 0.6 * 0.6, one whose rays all miss is the background -- from the restated hits alone."""
    from tests import lights_common as LC
    g = Q.golden()
    qs = Q.fixture_scene(g)
    qs.install(gpu)
    cam = Q.camera(g, 48, 48)
    p = qs.params(48, 48, RUST2, 1, samples=4)
    rays = [(o, d) for j in range(48) for i in range(48) for o, d, _, _ in LC.pixel_samples(cam, p, i, j)]
    hit = qs.closest(np.array([r[0] for r in rays]), np.array([r[1] for r in rays]))["found"].reshape(48, 48, 4)
    img, st = gpu.render(cam, p)
    bg, col = Q.f32(g["background"]), Q.f32(g["color"])
    one = (Q.f32(g["emitted"]) + (bg * col).astype(F)).astype(F)
    full = (((one + one).astype(F) + one).astype(F) + one).astype(F) / F(4.0)       # the driver's sum of four equal samples from +0, over their number
    sky = (((bg + bg).astype(F) + bg).astype(F) + bg).astype(F) / F(4.0)
    all_hit, all_miss = hit.all(axis=2), ~hit.any(axis=2)
    assert all_hit.sum() > 300 and all_miss.sum() > 300
    assert not differ(img[all_hit], np.broadcast_to(full.astype(F), img[all_hit].shape)).any()
    assert not differ(img[all_miss], np.broadcast_to(sky.astype(F), img[all_miss].shape)).any()
    assert st.segments == 48 * 48 * 4 and st.camera_rays == 48 * 48 * 4


# ---- 4. bounce for bounce, through every kernel of the build -------------------------------------------------------------------------------------
def compare_frames(gpu, qs, cam, p, key, names=None, build=None):
    ref, seg, info = Q.render(qs, cam, p, key=key)
    res = variants(gpu, cam, p, build=build)
    for name, (img, st) in res.items():
        bad = differ(img, ref)
        print(f"{key} integrator {p.integrator} depth {p.depth} flags {p.flags} [{name}]: {int(bad.sum())} values differ, segments {st.segments} / {seg}, "
              f"node tests {st.node_tests}")
        assert not bad.any(), (key, p.integrator, p.depth, name, int(bad.sum()))
        assert st.segments == seg and st.camera_rays == p.width * p.height * 4, (key, name)
    return ref, info, res


def test_fixture_alone_rust2(gpu):
    """The fixture as it is (no top-level sphere: every request walks the list), depths 2 and 6."""
    g = Q.golden()
    qs = Q.fixture_scene(g)
    qs.install(gpu)
    cam = Q.camera(g, 24, 24)
    for depth in (2, 6):
        ref, _, res = compare_frames(gpu, qs, cam, qs.params(24, 24, RUST2, depth), "fixture")
        # a 0.6 box under a 0.6 sky: a sample is 0.6 (miss) or 0.6 * 0.6^k after k hits, so the frame holds the sky and darker box pixels
        assert np.isfinite(ref).all() and ref.max() == F(0.6) and ref.min() < F(0.5) and (ref < F(0.6)).mean() > 0.1
        assert all(st.node_tests == 0 and st.quad_tests > 0 for _, st in res.values())


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("integrator", [RUST2, BIASED, CAST])
def test_bounce_for_bounce(gpu, integrator, moving):
    """The fixture with one emissive quad as a light outside the box and two top-level spheres (so that the tree kernels are reachable and the
    tree has a node; moving: one of them moves, the MOVING kernels): render_brute<MOVING, 11, GEOM> and render_bvh<MOVING, {global, LDS nodes}, 11, GEOM> against the restated
    front-to-back colour, depths 2 and 6.  Some shadow rays must cross the rotated instance, some must reach the light."""
    g = Q.golden()
    sphere = dict(SPHERE, velocity=[0.0, 0.3, 0.0]) if moving else SPHERE
    qs = Q.fixture_scene(g, spheres=[sphere, SPHERE2], quads=[LIGHT_QUAD], lights=[(R.LIGHT_QUAD, 0)])
    qs.install(gpu, 0.0, 1.0)
    cam = Q.camera(g, 24, 24)
    for depth in (2, 6):                                             # (LIGHT_CAST ignores the depth: the same frame twice)
        ref, info, res = compare_frames(gpu, qs, cam, qs.params(24, 24, integrator, depth, seed=7), ("lit", moving), build=(11, moving, True))
        assert np.isfinite(ref).all()
        assert res["list"][1].node_tests == 0 and res["tree, lds nodes"][1].node_tests > 0 and res["tree, global nodes"][1].node_tests > 0
        if integrator != RUST2:
            # shadow rays cross the ROTATED INSTANCE (blocked by it, not only by a sphere), others reach the light
            assert info["blocked_inst"] >= 1 and info["reached"] >= 1, info


@pytest.mark.parametrize("integrator", [BIASED, CAST])
def test_material_pdf_reads_the_instance_local_direction(gpu, integrator):
    """Rust2's Hit carries the ray the MEMBER was hit with (quad.rs:138-143), and Instance::get_hit turns p and n back but not r: material_pdf's
    side test, h.r.direction . h.n >= 0 (material.rs:55), is q(d) . q(n_local) = d . n_local, not d_world . q(n_local).  From the fixture's
    camera no primary ray meets a lit face where the two signs differ (the face with local normal -x lies at world x < 0 there), so this scene
    moves the box to x = +2 and lights that face from the left: for hundreds of lit hits the world direction would give the other side, and
    a pdf of 0 where the reference's is cos / pi."""
    g = dict(Q.golden(), translation=[2.0, 0.0, 5.0])
    light = dict(LIGHT_QUAD, origin=[-3.0, -0.5, 4.5], u=[0.0, 1.0, 0.0], v=[0.0, 0.0, 1.0])
    qs = Q.fixture_scene(g, spheres=[SPHERE2, dict(SPHERE, origin=[-1.5, 1.5, 6.0])], quads=[light], lights=[(R.LIGHT_QUAD, 0)])
    qs.install(gpu)
    ref, info, _ = compare_frames(gpu, qs, Q.camera(g, 24, 24), qs.params(24, 24, integrator, 2, seed=7), "side")
    assert np.isfinite(ref).all() and info["side_differs"] >= 100 and info["reached"] > info["side_differs"], info


def test_bounce_for_bounce_mixed_material(gpu):
    """FLAG_MIXED_MATERIAL with a mixed(exp) box: the flag is read at run time by the quaternion build."""
    g = Q.golden()
    qs = Q.fixture_scene(g, spheres=[SPHERE, SPHERE2], quads=[LIGHT_QUAD], lights=[(R.LIGHT_QUAD, 0)], material=R.mixed(6.0))
    qs.install(gpu)
    cam = Q.camera(g, 24, 24)
    p = qs.params(24, 24, BIASED, 6, seed=9, flags=R.FLAG_MIXED_MATERIAL)
    ref, info, _ = compare_frames(gpu, qs, cam, p, "mixed")
    assert np.isfinite(ref).all() and info["reached"] >= 1
    # without the flag the same box is Lambertian (opacity < 0 selects what it always did): another frame, and the restatement's
    q = qs.params(24, 24, BIASED, 6, seed=9)
    ref0, _, _ = compare_frames(gpu, qs, cam, q, "mixed, flag off")
    assert differ(ref, ref0).any()


# ---- 5. selection and lifecycle ------------------------------------------------------------------------------------------------------------------
def test_rotations_select_the_build_and_set_scene_clears_them(gpu, rtw):
    """RtwStats carries no build name; what shows the build is the frame: with rotations it is the restatement's (the turned box), without them it
    is the frame of a fresh context that never saw a rotation, bit for bit -- after rendering with rotations on the same context."""
    g = Q.golden()
    qs = Q.fixture_scene(g, spheres=[SPHERE])
    cam = Q.camera(g, 24, 24)
    p = qs.params(24, 24, RUST2, 2, seed=5)
    with rtw.Renderer(0) as fresh:
        fresh.set_scene(qs.scene)
        plain, st_plain = fresh.render(cam, p)
    qs.install(gpu)
    turned, st = gpu.render(cam, p)
    ref, seg, _ = Q.render(qs, cam, p, key="select")
    assert not differ(turned, ref).any() and st.segments == seg
    assert differ(turned, plain).any()
    gpu.set_scene(qs.scene)                                          # clears the rotations
    again, st_again = gpu.render(cam, p)
    assert not differ(again, plain).any() and st_again.segments == st_plain.segments
    qs.install(gpu)
    gpu.set_instance_rotations(None)                                 # ... and so does NULL / 0
    assert not differ(gpu.render(cam, p)[0], plain).any()
    # the identity quaternion is a quaternion instance like any other: the frame of the unturned box through the new build
    ident = Q.QuatScene([SPHERE], instances=[Q.box_instance(g, quat=[1, 0, 0, 0])], background=g["background"], mint=g["mint"], maxt=g["maxt"])
    ident.install(gpu)
    ref_i, _, _ = Q.render(ident, cam, p, key="identity")
    assert not differ(gpu.render(cam, p)[0], ref_i).any()


def test_two_contexts_on_one_gpu_equal_the_unsplit_frame(gpu, rtw):
    g = Q.golden()
    qs = Q.fixture_scene(g, spheres=[SPHERE], quads=[LIGHT_QUAD], lights=[(R.LIGHT_QUAD, 0)])
    qs.install(gpu)
    cam = Q.camera(g, 24, 24)
    p = qs.params(24, 24, BIASED, 2, seed=7)
    whole, _ = gpu.render(cam, p)
    with rtw.MultiRenderer([0, 0]) as m:
        m.set_scene(qs.scene)
        m.set_instance_rotations(qs.quats)
        m.set_lights(qs.lights, qs.weight)
        out = m.render(cam, p)
    assert not differ(out[0], whole).any()


def test_what_is_not_built_is_refused(gpu, rtw):
    g = Q.golden()
    qs = Q.fixture_scene(g)
    qs.install(gpu)
    cam = Q.camera(g, 16, 16)

    def status(renderer, p):
        with pytest.raises(rtw.RtwError) as e:
            renderer.render(cam, p)
        return e.value.status

    for integ in (R.INTEGRATOR_GRADIENT, R.INTEGRATOR_BG_COLOR, R.INTEGRATOR_NORMAL, R.INTEGRATOR_FLAG):
        assert status(gpu, qs.params(16, 16, integ, 2)) == E_INVALID
    gpu.set_triangles([R.Triangle.new([0, 0, 9], [1, 0, 0], [0, 1, 0])])
    assert status(gpu, qs.params(16, 16, RUST2, 2)) == E_INVALID
    gpu.set_triangles(None)
    gpu.render(cam, qs.params(16, 16, RUST2, 2))
    # active texture noise: a textured sphere whose texture has noise
    img = np.full((2, 2, 3), 0.5, F)
    tex_sphere = R.Sphere.new_with_texture([0, 0, 9], 0.5, (1.0, 1.0, 1.0), (0.0, 0.0, 1.0), 0)
    inst = R.Instance.new_box([-1, -1, -1], [1, 1, 1], g["color"], (0.0, 0.0, 1.0))
    inst.translation = g["translation"]
    noisy = R.Scene([tex_sphere], textures=[img], background=g["background"], instances=[inst], noise={0: (R.PerlinNoise(1), 1.0)})
    gpu.set_scene(noisy)
    gpu.set_instance_rotations(qs.quats)
    for integ in (RUST2, BIASED, R.INTEGRATOR_GRADIENT):
        assert status(gpu, qs.params(16, 16, integ, 2)) == E_INVALID
    # the setter's own refusals on a context
    qs.install(gpu)
    with pytest.raises(rtw.RtwError) as e:
        gpu.set_instance_rotations([[1, 0, 0, 0], [1, 0, 0, 0]])
    assert e.value.status == E_INVALID
    with pytest.raises(rtw.RtwError) as e:
        gpu.set_instance_rotations([[0, 0, 0, 0]])
    assert e.value.status == E_INVALID
    with rtw.Renderer(0) as r:
        with pytest.raises(rtw.RtwError) as e:
            r.set_instance_rotations(qs.quats)
        assert e.value.status == -6                                  # RTW_E_NO_SCENE
