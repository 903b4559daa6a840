"""RTW_OPT_NODE_FORMAT on the GPU: the f32-plane walk of the 768-thread builds against the f16 walk, in one process on one context.

Every case renders the same frame with the option at 1 (f16 nodes) and at 2 (f32 planes) -- and under 0 where the automatic choice is the
subject -- and asks for EQUAL frame bytes, segments, camera rays, node visits and sphere tests, and for the oracle's frame and segments."""
import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests.test_node_format_cpu import hand_scene
from tests.test_oracle_golden import small_view

pytestmark = pytest.mark.gpu
F32_BUILD, F16_BUILD = "render_bvh<0,1,1,0>", "render_bvh<0,2,1,0>"     # the 768-thread build; the f16 walk with the geometry in LDS


def render_formats(gpu, scene, cam, p, formats=(1, 2), chunk_len=0):
    """{format: (image, stats, build, node format)} with the tree forced (no list walk)."""
    gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
    out = {}
    try:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        gpu.set_option(R.OPT_CHUNK_LEN, chunk_len)
        for f in formats:
            gpu.set_option(R.OPT_NODE_FORMAT, f)
            img, st = gpu.render(cam, p)
            out[f] = (img, st, gpu.last_render_build(), gpu.last_node_format())
    finally:
        gpu.set_option(R.OPT_NODE_FORMAT, 0)
        gpu.set_option(R.OPT_CHUNK_LEN, 0)
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    return out


def assert_same(a, b, what):
    (ia, sa, _, _), (ib, sb, _, _) = a, b
    assert ia.tobytes() == ib.tobytes(), what
    for k in ("segments", "camera_rays", "node_tests", "sphere_tests"):
        assert getattr(sa, k) == getattr(sb, k), (what, k, getattr(sa, k), getattr(sb, k))


def check(gpu, scene, cam, p, what, chunk_len=0, auto_f32=True):
    p.gamma, p.accel = 1.0, R.ACCEL_BVH
    ref, st_ref = O.render(cam, scene, p, threads=16)
    out = render_formats(gpu, scene, cam, p, (1, 2, 0), chunk_len)
    assert out[1][2:] == (F16_BUILD, R.NODE_FORMAT_F16), (what, out[1][2:])
    assert out[2][2:] == (F32_BUILD, R.NODE_FORMAT_F32), (what, out[2][2:])
    # automatic: f32 planes for a tree whose scene the shim serves with the geometry in global memory (every such tree fits); a scene small
    # enough for its geometry to ride in LDS keeps the f16 build it had
    assert out[0][2:] == ((F32_BUILD, R.NODE_FORMAT_F32) if auto_f32 else (F16_BUILD, R.NODE_FORMAT_F16)), (what, out[0][2:])
    assert_same(out[1], out[2], what)
    assert_same(out[0], out[2], what)
    assert out[2][1].segments == st_ref.segments and np.array_equal(out[2][0], ref), what
    return out


def octants(cam, scene, p, step=6):
    """Sign combinations of the directions of the oracle's centre rays through every step-th pixel and of their bounces."""
    seen = set()
    o = np.array(cam.origin[:], np.float32)
    for j in range(0, p.height, step):
        for i in range(0, p.width, step):
            d = np.array(cam.pixel00[:], np.float32) + np.float32(i) * np.array(cam.delta_u[:], np.float32) + np.float32(j) * np.array(cam.delta_v[:], np.float32) - o
            bounces, _ = O.trace_ray(o, d, 0.0, scene, p, pixel=j * p.width + i)
            for v in [d] + [np.array(b.next_dir[:], np.float32) for b in bounces if b.hit]:
                if np.all(v != 0):
                    seen.add(tuple(bool(x < 0) for x in v))
    return seen


def test_book1_small_frame_every_octant(gpu):
    scene, cam, p = small_view(R.SCENE_C2, 64, 48, 8)
    p.depth = 50
    assert len(octants(cam, scene, p)) == 8, "the frame must send rays into all eight octants"
    check(gpu, scene, cam, p, "book1 64x48")


@pytest.mark.parametrize("n_small", [2, 3, 5])
def test_hand_built_trees(gpu, n_small):
    """Root a leaf pair, one inner level, an odd tree: the smallest trees in which a child code in units of a node can go wrong."""
    vp = R.Viewport.new_from_res(48, 32, 4, 12, 1.0, vfov=60.0, origin=(0.0, 0.3, 1.5), direction=(0.0, -0.1, -1.0), lens_radius=0.0)
    check(gpu, hand_scene(n_small), vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW), f"{n_small} spheres", auto_f32=False)


def many_spheres(n_small):
    rng = np.random.default_rng(11)
    sp = [R.Sphere.with_albedo((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), R.SCATTER_M)]
    sp += [R.Sphere.with_albedo((float(rng.uniform(-8, 8)), 0.2, float(rng.uniform(-8, 8))), 0.2, rng.uniform(0.2, 0.9, 3),
                                (R.SCATTER_M, R.METALLIC_M, R.GLASS_M)[k % 3]) for k in range(n_small)]
    return R.Scene(sp)


@pytest.mark.parametrize("n_small,expect", [(513, (F32_BUILD, 2)), (514, ("render_bvh<0,0,1,0>", 0))])
def test_largest_tree_that_lives_in_lds_and_one_more(gpu, n_small, expect):
    """What bounds the f32 planes.  The 16-bit codes would allow 2341 nodes (0x7FFD / 14 + 1), and two workgroups fit a CU's LDS for every
    tree the builder gives f16 nodes, so the limit that binds is the builder's own: 512 inner nodes (RTW_LDS_NODES_MAX).  513 tree spheres
    make the largest such tree and run as f32 planes under the automatic choice; one more has no LDS copy at all and takes the
    global-node build, as it did before.  Both render what the f16 request renders."""
    scene = many_spheres(n_small)
    vp = R.Viewport.new_from_res(32, 24, 2, 10, 1.0, vfov=40.0, origin=(13.0, 2.0, 3.0), direction=(-13.0, -2.0, -3.0), lens_radius=0.0)
    cam, p = vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)
    p.gamma = 1.0
    ref, st_ref = O.render(cam, scene, p, threads=16)
    out = render_formats(gpu, scene, cam, p, (0, 1))
    assert out[0][2:] == expect, out[0][2:]
    assert_same(out[0], out[1], n_small)
    assert out[0][1].segments == st_ref.segments and np.array_equal(out[0][0], ref)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_parallel_rays_with_guarded_reciprocals(gpu, sign):
    """Every camera ray runs down -z with x and y components of +-1e-30 or so: 1/d takes the +-1e20 guard, by the component's sign."""
    vp = R.Viewport.new_from_res(16, 16, 4, 12, 1.0, vfov=60.0, origin=(0.0, 0.0, 2.0), direction=(0.0, 0.0, -1.0), lens_radius=0.0)
    cam, p = vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)
    tiny = sign * 1e-30
    for k in range(3):
        cam.delta_u[k] = tiny if k == 0 else 0.0
        cam.delta_v[k] = tiny if k == 1 else 0.0
        cam.pixel00[k] = (tiny, tiny, 1.0)[k]
    out = check(gpu, hand_scene(5), cam, p, f"parallel rays {sign}", auto_f32=False)
    assert out[2][1].node_tests > 0


def flat_camera(y_plane, y_origin, dy):
    """Every camera ray lies in a plane of constant y: d.y = (y_plane + i * dy + j * dy) - y_origin, with dy a zero."""
    vp = R.Viewport.new_from_res(16, 16, 4, 12, 1.0, vfov=60.0, origin=(0.0, 0.0, 2.0), direction=(0.0, 0.0, -1.0), lens_radius=0.0)
    cam, p = vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)
    for k in range(3):
        cam.origin[k] = (0.0, y_origin, 2.0)[k]
        cam.pixel00[k] = (-0.5, y_plane, 1.0)[k]
        cam.delta_u[k] = (1.0 / 16.0, dy, 0.0)[k]
        cam.delta_v[k] = (0.0, dy, -1.0 / 16.0)[k]
    return cam, p


def test_rays_with_an_exactly_zero_component(gpu):
    """Camera rays whose y component is exactly +0.0 (0.1 - 0.1): 1/d takes the guard, copysign(1e20, d)."""
    cam, p = flat_camera(0.1, 0.1, 0.0)
    out = check(gpu, hand_scene(5), cam, p, "d.y == +0.0", auto_f32=False)
    assert out[2][1].node_tests > 0


def test_negative_zero_component_never_reaches_the_tree_from_a_camera(gpu):
    """d.y == -0.0 needs -0.0 in pixel00.y, delta_u.y and delta_v.y and +0.0 in origin.y ((-0.0) - (+0.0); x - x is +0.0): the pixel plane
    then holds the world's origin, and a BVH request with such a camera walks the list (rtw_ctx_render's gate on the camera).  So the sign
    rule for -0.0 is pinned on the host (test_node_format_cpu.py: 1/d = copysign(1e20, -0.0) reads at offset 0), and here only that no
    format of the tree sees such a camera."""
    cam, p = flat_camera(-0.0, 0.0, -0.0)
    p.gamma, p.accel = 1.0, R.ACCEL_BVH
    scene = hand_scene(5)
    ref, st_ref = O.render(cam, scene, p, threads=16)
    out = render_formats(gpu, scene, cam, p, (1, 2))
    for f in (1, 2):
        assert out[f][2].startswith("render_brute") and out[f][3] == R.NODE_FORMAT_NONE, out[f][2:]
        assert out[f][1].segments == st_ref.segments and np.array_equal(out[f][0], ref)


@pytest.mark.parametrize("samples", [8, 24, 26])
def test_less_than_one_workgroup_of_work_and_one_unit_more(gpu, samples):
    """One 8x8 tile in units of two samples: 4, 12 and 13 units of 64 items -- less than the 768 threads of a workgroup, exactly that, one more."""
    scene, cam, p = small_view(R.SCENE_C2, 8, 8, samples)
    check(gpu, scene, cam, p, f"{samples} samples", chunk_len=2)


def test_option_is_validated(gpu):
    for bad in (-1, 3, 0.5):
        with pytest.raises(R.RtwError):
            gpu.set_option(R.OPT_NODE_FORMAT, bad)
    for ok in (1, 2, 0):
        gpu.set_option(R.OPT_NODE_FORMAT, ok)
