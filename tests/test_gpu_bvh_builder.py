"""The trees of the sweep + reinsertion builder on the GPU: each render through the tree (RTW_OPT_LIST_WALK_MAX = 0, node_tests > 0) must be the
brute-force kernel's image bit for bit -- 64 x 64, 8 spp, depth 10 -- and one 8-row block of the bench frame must be the oracle's."""
import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests.test_bvh_builder_cpu import S, field, geometric, LDS_NODES_MAX

pytestmark = pytest.mark.gpu


def oversized_130():
    rng = np.random.default_rng(5)
    sp = [S(0, -1000, 0, 1000)]
    sp += [S(rng.uniform(-6, 6), 0.2, rng.uniform(-6, 6), 0.2) for _ in range(126)]
    sp += [S(-3, 1.5, 0, 1.5), S(0, 2.0, -2, 2.0), S(3, 1.0, 1, 1.0)]
    return R.Scene(sp)


def view(origin, direction, vfov, shutter=0.0):
    cam, _ = O.viewport_new(64, np.float32(1.0), origin=origin, direction=direction, vfov=vfov)
    cam.shutter = shutter
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth = 64, 64, 8, 10
    p.gamma, p.mint, p.maxt = 1.0, 0.001, 100000.0
    p.integrator, p.sampler, p.seed = R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW, 1
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    return cam, p


FIELD_VIEW = ((13.0, 2.0, 3.0), (-0.9636, -0.1482, -0.2224), 40.0)
CASES = {
    "bench_shape_483_lds": (lambda: field(480, 3, ground=True), FIELD_VIEW, 0, 0.0),
    "bench_shape_483_global": (lambda: field(480, 3, ground=True), FIELD_VIEW, R.FLAG_GLOBAL_NODES, 0.0),
    "oversized_130": (oversized_130, ((9.0, 2.5, 4.0), (-0.9, -0.2, -0.4), 50.0), 0, 0.0),
    "geometric": (lambda: geometric(200), ((6.0, 0.3, 2.0), (0.3, -0.03, -1.0), 80.0), 0, 0.0),
    "moving": (lambda: field(300, 3, ground=True, moving=True), FIELD_VIEW, 0, 1.0 / 30.0),
    "one_node_over_lds": (lambda: field(LDS_NODES_MAX + 2, 0, ground=True), FIELD_VIEW, 0, 0.0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tree_render_equals_brute_force(gpu, name):
    make, (origin, direction, vfov), flags, shutter = CASES[name]
    scene = make()
    cam, p = view(origin, direction, vfov, shutter)
    gpu.set_scene(scene, 0.0, shutter)
    gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
    try:
        p.accel, p.flags = R.ACCEL_BRUTE, 0
        ref, st_ref = gpu.render(cam, p)
        p.accel, p.flags = R.ACCEL_BVH, flags
        img, st = gpu.render(cam, p)
    finally:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    assert st_ref.node_tests == 0 and st.node_tests > 0
    assert st.segments == st_ref.segments and st.segments > st.camera_rays
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_bench_frame_block_against_the_oracle(gpu):
    """The bench frame (Book-1 final, 1920 x 1080, depth 50) at 4 spp: rows 600..607, through the sphere field, bit for bit against the oracle."""
    scene = R.Scene.generate(R.SCENE_C2)
    cam, p = R.default_view(R.SCENE_C5)
    cam.shutter = 0.0
    p.samples = 4
    p.row_block, p.part_index, p.part_count = 8, 75, 135
    p.gamma = 1.0
    ref, st_ref = O.render(cam, scene, p, threads=16)
    gpu.set_scene(scene)
    img, st = gpu.render(cam, p)
    assert st.rows == 8 and st.camera_rays == 8 * 1920 * 4 and st.segments == st_ref.segments and st.node_tests > 0
    assert np.array_equal(img, ref)
