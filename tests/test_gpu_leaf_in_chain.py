"""Leaf tests that run inside the chain of bursts of the 768-thread render builds (rtw_kernels.hip render_bvh, Sched.leaf_rule).

In those builds the bursts of node visits follow one another while 13 or more lanes traverse, and since this change the lanes that wait
at a leaf are tested and popped inside that chain when more of them wait than traverse.  Scheduling decides WHEN a
lane's steps run, never what they compute: every frame must be the CPU oracle's bit for bit, and camera rays, segments, node visits
and sphere tests those of the same render through the f16 256-thread build (RTW_OPT_NODE_FORMAT = 1), whose loop has no such step.
Every render asserts the build that ran and its workgroup size (last_render_build, last_queue_plan).  A leaf step in the chain that
forgot its hi_lim update would visit nodes behind the hit it found (node_tests, sphere_tests), one that forgot to pop a lane whose
leaf test missed would test that sphere again (sphere_tests) -- both mutants were built and run against this file: 7 and 9 of its
10 tests fail.

No process is started and nothing waits: the kernel's own valve (RTW_MAX_TRIPS) bounds its loop, and a wave that hits it fails the render.

Shapes, each the smallest at which the step can still go wrong:
  book1 mixed       Book-1 scene, 64 x 48, 4 spp, depth 8: mixed waves, leaf steps inside a chain with 13 or more lanes traversing
  book1 one wave    Book-1 scene, 8 x 8, 13 spp: one tile; most waves of the workgroup are DEAD from the start and the drain runs with a partial wave
  three equal       three equal small spheres and the ground, tree forced, 16 x 16, 2 spp: a tree of two inner nodes, every query is at a
                    leaf right after its root visit, so many lanes wait at a leaf with few left in TRAVERSE
  three alike       the same scene with camera rays all alike (pixel deltas of 2^-149): all 64 lanes reach their leaf in the same burst,
                    64 at a leaf and none traversing -- the chain must leave after the leaf step
  line of 257       257 spheres on a line seen along it, 32 x 8, 2 spp: several leaf steps inside one chain, stacks popped to the sentinel
  book1 mixed under RTW_OPT_BLOCKS_PER_CU = 1, and as three row partitions (part_count = 3)."""
import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O

pytestmark = pytest.mark.gpu
LARGE_BUILDS = {"render_bvh<0,1,1,0>", "render_bvh<0,1,2,0>", "render_bvh<0,1,3,0>"}     # the builds whose workgroup is 768 threads
TREE_COUNTERS = ("camera_rays", "segments", "node_tests", "sphere_tests")
THREADS = 16
TINY = 2.0 ** -149           # the smallest f32


def _view(scene, w, h, spp, depth, **cam):
    vp = R.Viewport.new_from_res(w, h, spp, depth, 1.0, **cam)
    return scene, vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)


def book1(w, h, spp, depth):
    """The Book-1 scene in its default framing, w x h pixels wide apart (as tests/test_gpu_large_block_budget.py book1)."""
    def make():
        scene = R.Scene.generate(R.SCENE_C2, 42)
        cam, p = R.default_view(R.SCENE_C2)
        f = p.width / w
        for k in range(3):
            cam.pixel00[k] = cam.pixel00[k] - 0.5 * (cam.delta_u[k] + cam.delta_v[k]) + 0.5 * f * (cam.delta_u[k] + cam.delta_v[k])
            cam.delta_u[k] *= f
            cam.delta_v[k] *= f
        p.width, p.height, p.samples, p.depth = w, h, spp, depth
        return scene, cam, p
    return make


def book1_part(index):
    def make():
        scene, cam, p = book1(64, 48, 4, 8)()
        p.row_block, p.part_index, p.part_count = 8, index, 3          # six blocks of eight rows: two per part
        return scene, cam, p
    return make


def three_equal_scene():
    sp = [R.Sphere.with_albedo((0.0, -100.5, -1.5), 100.0, (0.5, 0.5, 0.5), R.SCATTER_M)]        # the ground: outside the tree
    sp += [R.Sphere.with_albedo((x, 0.1, -1.5), 0.3, (0.7, 0.4, 0.3), m) for x, m in ((-0.8, R.SCATTER_M), (0.0, R.SCATTER_M), (0.8, R.METALLIC_M))]
    return R.Scene(sp)


def three_equal():
    return _view(three_equal_scene(), 16, 16, 2, 8, vfov=60.0, origin=(0.0, 0.1, 1.5), direction=(0.0, 0.0, -1.0), lens_radius=0.0)


def three_alike():
    """Every camera ray is (0, 0, -1) from one origin, up to a few 2^-149 in x and y (tests/test_gpu_shade_step_edges.py along_an_axis),
    and meets the middle sphere: 64 lanes walk the same two nodes in step."""
    scene, cam, p = three_equal()
    for k, (p00, du, dv) in enumerate(((0.0, TINY, 0.0), (0.0, 0.0, TINY), (-1.0, 0.0, 0.0))):
        cam.pixel00[k], cam.delta_u[k], cam.delta_v[k] = p00, du, dv
    return scene, cam, p


def line_of_257():
    sp = [R.Sphere.with_albedo((0.0, -100.5, -1.5), 100.0, (0.5, 0.5, 0.5), R.SCATTER_M)]
    # (radius 0.1 at y = +-0.15, seen from a point on the line's axis: a ray along the axis passes between the spheres and through every inner box)
    sp += [R.Sphere.with_albedo((0.45 * k, 0.15 if k % 2 else -0.15, -1.5), 0.1, (0.3 + 0.002 * k, 0.5, 0.8 - 0.002 * k), (R.SCATTER_M, R.METALLIC_M)[k % 2])
           for k in range(257)]
    return _view(R.Scene(sp), 32, 8, 2, 8, vfov=6.0, origin=(-1.0, 0.0, -1.5), direction=(1.0, 0.0, 0.0), lens_radius=0.0)


# name: (maker, options beside the forced tree)
CASES = {"book1 mixed": (book1(64, 48, 4, 8), {}), "book1 one wave": (book1(8, 8, 13, 8), {}), "three equal": (three_equal, {}),
         "three alike": (three_alike, {}), "line of 257": (line_of_257, {}),
         "book1 mixed, one workgroup per CU": (book1(64, 48, 4, 8), {R.OPT_BLOCKS_PER_CU: 1}),
         "book1 part 0 of 3": (book1_part(0), {}), "book1 part 1 of 3": (book1_part(1), {}), "book1 part 2 of 3": (book1_part(2), {})}
_made, _oracle = {}, {}


def case(name):
    if name not in _made:
        scene, cam, p = CASES[name][0]()
        p.gamma, p.accel = 1.0, R.ACCEL_BVH
        _made[name] = (scene, cam, p)
    return _made[name]


def oracle_frame(name):
    """The oracle's frame and path counters of a case: rendered once, shared, never written."""
    if name not in _oracle:
        scene, cam, p = case(name)
        ref, st = O.render(cam, scene, p, threads=THREADS)
        ref.setflags(write=False)
        _oracle[name] = (ref, {k: getattr(st, k) for k in ("camera_rays", "segments")})
    return _oracle[name]


def render(gpu, name, fmt):
    """One render of a case under RTW_OPT_NODE_FORMAT = fmt with the tree forced: (frame, counters, build, workgroup size)."""
    scene, cam, p = case(name)
    gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
    opts = dict(CASES[name][1])
    try:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        gpu.set_option(R.OPT_NODE_FORMAT, fmt)
        for k, v in opts.items():
            gpu.set_option(k, v)
        img, st = gpu.render(cam, p)
        build, block = gpu.last_render_build(), gpu.last_queue_plan()["block"]
    finally:
        for k in opts:
            gpu.set_option(k, 0)
        gpu.set_option(R.OPT_NODE_FORMAT, 0)
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    return img, {k: getattr(st, k) for k in TREE_COUNTERS}, build, block


@pytest.mark.parametrize("name", list(CASES))
def test_frame_is_the_oracle_s_and_counters_the_f16_walk_s(gpu, name):
    ref, path = oracle_frame(name)
    img, got, build, block = render(gpu, name, 2)
    img16, want, build16, block16 = render(gpu, name, 1)
    differ = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum()) if img.shape == ref.shape else "shape"
    print(name, build, block, got, "| f16 walk:", build16, block16, want, "| oracle:", path, "| pixels that differ:", differ)
    assert build in LARGE_BUILDS and block == 768, (name, build, block)
    assert build16 not in LARGE_BUILDS and build16.startswith("render_bvh") and block16 == 256, (name, build16, block16)
    assert got["node_tests"] > 0 and got["sphere_tests"] > 0, (name, got)
    assert got == want, (name, got, want)
    assert {k: got[k] for k in path} == path, (name, got, path)
    assert img16.tobytes() == ref.tobytes(), name             # (the yardstick itself)
    assert img.shape == ref.shape and img.dtype == ref.dtype and img.tobytes() == ref.tobytes(), name


def test_the_cases_are_what_they_say(gpu):
    """The conditions the cases are there for, from the scenes and the counters."""
    _, eq, _, _ = render(gpu, "three equal", 2)
    assert 0 < eq["node_tests"] <= 2 * eq["segments"]                        # a tree of two inner nodes: at most two visits per query
    scene, cam, p = case("three alike")
    assert cam.pixel00[0] == 0.0 and cam.delta_u[0] == TINY > 0.0 and cam.delta_v[1] == TINY and cam.pixel00[2] == -1.0
    assert np.float32(TINY) * np.float32(15.99) < 1e-40                      # every camera ray is (0, 0, -1) up to denormals
    bounces, _ = O.trace_ray((0.0, 0.1, 1.5), (0.0, 0.0, -1.0), 0.0, scene, p)
    assert bounces[0].hit                                                    # ... and meets the middle sphere
    _, al, _, _ = render(gpu, "three alike", 2)
    assert al["segments"] > al["camera_rays"] == 16 * 16 * 2
    _, ln, _, _ = render(gpu, "line of 257", 2)
    assert ln["node_tests"] > 8 * ln["segments"] and ln["sphere_tests"] > ln["segments"]     # a walk of a deep tree with more than one leaf per query
    parts = [oracle_frame("book1 part %d of 3" % k) for k in range(3)]
    whole = oracle_frame("book1 mixed")
    assert sum(f.shape[0] for f, _ in parts) == 48 and sum(c["segments"] for _, c in parts) == whole[1]["segments"]
