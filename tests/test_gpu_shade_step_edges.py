"""The SHADE step of the two-halves render builds (rtw_kernels.hip render_bvh) at its edges, against the CPU oracle.

The step's lane masks are ballots of single compares met in scalar code, the end of a path is two compares instead of a flag set and
tested again, a lane asks for a work unit by its flag word alone, and d.d's range test is one integer compare.  None of
that touches a rounded operation or the order in which units are handed out, so every frame must be the oracle's bit for bit and the
path counters -- camera rays, segments, NaN pixels, rows, quad tests -- the oracle's exactly.  Every case renders once through the
768-thread build (f32 planes) and once through a 256-thread build (f16 nodes, geometry in LDS), and says which build ran.

Shapes: the smallest at which a rewritten block can still go wrong -- a frame with hit, miss and glass lanes in one wave; one row of
96 pixels (units of 64 items: waves start with fewer units than lanes and refill inside the step); depth 1 and 2 (every hit ends on the
depth test; the bounce count in the flag word); glass spheres hit on both faces; rays with a direction component exactly 0; a frame
of sky alone (every lane misses, banks and starts a path in the same step); and two seeds in one context, then the first again."""
import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests.test_gpu_large_block_budget import book1
from tests.test_node_format_cpu import hand_scene

pytestmark = pytest.mark.gpu
PATH_COUNTERS = ("camera_rays", "segments", "nan_pixels", "rows", "quad_tests")
# (OPT_NODE_FORMAT, the build a static scene without textures gets under it, the format it reads from LDS, threads per workgroup)
BUILDS = {"768 threads": (2, "render_bvh<0,1,1,0>", R.NODE_FORMAT_F32), "256 threads": (1, "render_bvh<0,2,1,0>", R.NODE_FORMAT_F16)}
THREADS = 16


def _view(scene, w, h, spp, depth, **cam):
    vp = R.Viewport.new_from_res(w, h, spp, depth, 1.0, **cam)
    return scene, vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)


def book1_frame():
    return book1()


def book1_row():
    scene, cam, p = book1()
    p.row_block, p.part_index, p.part_count = 1, 37, 64          # 64 rows in one-row blocks: part 37 of 64 is row 37
    return scene, cam, p


def book1_depth(depth):
    def make():
        scene, cam, p = book1()
        p.depth = depth
        return scene, cam, p
    return make


def glass_spheres():
    """Glass alone above a diffuse ground: a ray that enters a sphere meets its back face from inside, one between two spheres both."""
    sp = [R.Sphere.with_albedo((0.0, -100.5, -1.0), 100.0, (0.5, 0.5, 0.5), R.SCATTER_M)]
    for k, (x, y, z, r) in enumerate(((0.0, 0.0, -1.2, 0.5), (-1.0, -0.1, -1.6, 0.4), (1.0, -0.1, -1.6, 0.4), (0.3, -0.3, -0.5, 0.2), (-0.4, 0.5, -2.2, 0.6))):
        sp.append(R.Sphere.with_albedo((x, y, z), r, (1.0, 1.0, 1.0) if k % 2 else (0.9, 1.0, 0.9), R.GLASS_M))
    return _view(R.Scene(sp), 64, 64, 8, 12, vfov=60.0, origin=(0.0, 0.2, 1.0), direction=(0.0, -0.1, -1.0), lens_radius=0.0)


TINY = 2.0 ** -149           # the smallest f32


def along_an_axis():
    """Every camera ray runs down -z: pixel00 = (0, 0, -1), delta_u.x = delta_v.y = 2^-149.  d.x = 0 + 2^-149 * jx is exactly +0 where the
    jittered column jx < 0.5 (half the samples of column 0; likewise d.y in row 0) and a few 2^-149 elsewhere, so every ray takes the
    reciprocal guard, by a zero or by a denormal.  (A camera whose rays ALL have a zero component has the world's origin in its pixel
    plane, and a BVH request with such a camera walks the list: this plane is z = -1.)  The lens spreads the origins over the glass
    sphere in the middle and past its rim."""
    scene, cam, p = _view(hand_scene(5), 64, 32, 8, 8, vfov=60.0, origin=(0.0, 0.1, 1.5), direction=(0.0, 0.0, -1.0), lens_radius=0.35)
    for k, (p00, du, dv) in enumerate(((0.0, TINY, 0.0), (0.0, 0.0, TINY), (-1.0, 0.0, 0.0))):
        cam.pixel00[k], cam.delta_u[k], cam.delta_v[k] = p00, du, dv
    return scene, cam, p


def sky_only():
    """The camera looks up and away from every sphere: each path is one segment."""
    return _view(hand_scene(3), 64, 32, 8, 8, vfov=60.0, origin=(0.0, 0.3, 1.5), direction=(0.0, 1.0, 1.0), lens_radius=0.0)


def other_seed():
    scene, cam, p = book1()
    p.seed = p.seed + 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF
    return scene, cam, p


CASES = {"book1": book1_frame, "book1 one row": book1_row, "book1 depth 1": book1_depth(1), "book1 depth 2": book1_depth(2),
         "glass spheres": glass_spheres, "along an axis": along_an_axis, "sky only": sky_only, "book1 other seed": other_seed}
_made, _oracle = {}, {}


def case(name):
    if name not in _made:
        scene, cam, p = CASES[name]()
        p.gamma, p.accel = 1.0, R.ACCEL_BVH
        _made[name] = (scene, cam, p)
    return _made[name]


def oracle_frame(name):
    """The oracle's frame and counters of a case: rendered once, shared, never written."""
    if name not in _oracle:
        scene, cam, p = case(name)
        ref, st = O.render(cam, scene, p, threads=THREADS)
        ref.setflags(write=False)
        _oracle[name] = (ref, {k: getattr(st, k) for k in PATH_COUNTERS})
    return _oracle[name]


def render(gpu, name, build, set_scene=True):
    """One render of a case through a build: (frame, path counters); asserts the build and the node format that ran."""
    fmt, tag, node_format = BUILDS[build]
    scene, cam, p = case(name)
    if set_scene:
        gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
    try:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        gpu.set_option(R.OPT_NODE_FORMAT, fmt)
        img, st = gpu.render(cam, p)
        assert gpu.last_render_build() == tag and gpu.last_node_format() == node_format, (name, build, gpu.last_render_build(), gpu.last_node_format())
    finally:
        gpu.set_option(R.OPT_NODE_FORMAT, 0)
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    assert st.node_tests > 0, (name, build)
    return img, {k: getattr(st, k) for k in PATH_COUNTERS}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", [n for n in CASES if n != "book1 other seed"])
def test_frame_and_path_counters_are_the_oracle_s(gpu, name, build):
    ref, counters = oracle_frame(name)
    img, got = render(gpu, name, build)
    print(name, build, got, "pixels that differ:", int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum()) if img.shape == ref.shape else "shape")
    assert got == counters, (name, build, got, counters)
    assert same_bits(img, ref), (name, build)


def test_the_cases_are_what_they_say():
    """The conditions the cases are there for, on the oracle's side."""
    _, sky = oracle_frame("sky only")
    assert sky["segments"] == sky["camera_rays"] == 64 * 32 * 8                     # every path ends on its first query
    _, d1 = oracle_frame("book1 depth 1")
    _, d2 = oracle_frame("book1 depth 2")
    _, full = oracle_frame("book1")
    assert d1["segments"] == d1["camera_rays"] < d2["segments"] < full["segments"]   # depth 1: one query per path, hit or miss
    assert oracle_frame("book1 one row")[0].shape == (1, 96, 3)
    scene, cam, p = case("along an axis")
    assert cam.pixel00[0] == 0.0 and cam.delta_u[0] == TINY > 0.0 and cam.delta_v[0] == 0.0      # d.x = (0 + 2^-149 * jx) + 0 * jy
    assert np.float32(cam.delta_u[0]) * np.float32(0.49) == 0.0 and np.float32(cam.delta_u[0]) * np.float32(63.5) < 1e-20
    _, ax = oracle_frame("along an axis")
    assert ax["camera_rays"] < ax["segments"] < 8 * ax["camera_rays"]               # some of these rays hit, and not all end at the depth limit
    scene, cam, p = case("glass spheres")
    bounces, _ = O.trace_ray((0.0, 0.2, 1.0), (0.0, -0.17, -1.0), 0.0, scene, p)    # through the middle sphere
    faces = [b.front_face for b in bounces if b.hit]
    assert 1 in faces and 0 in faces, faces


@pytest.mark.parametrize("build", list(BUILDS))
def test_two_seeds_in_one_context_then_the_first_again(gpu, build):
    """The second frame must not find anything of the first in the bank or the queue, nor the third of the second."""
    (ref_a, cnt_a), (ref_b, cnt_b) = oracle_frame("book1"), oracle_frame("book1 other seed")
    assert not same_bits(ref_a, ref_b)
    for k, (name, ref, cnt) in enumerate((("book1", ref_a, cnt_a), ("book1 other seed", ref_b, cnt_b), ("book1", ref_a, cnt_a))):
        img, got = render(gpu, name, build, set_scene=k == 0)          # (one scene, set once: the three renders share the context's buffers)
        assert got == cnt and same_bits(img, ref), (name, build, got, cnt)
