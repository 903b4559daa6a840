"""The 768-thread render builds with one ds_read_b64 per plane pair of a node visit (rtw_kernels.hip trav_node_lds32).

How the pairs are fetched touches no rounded operation, so a frame of such a build and every counter of its launch must be what the f16
walk (RTW_OPT_NODE_FORMAT = 1) gives, and frame, camera rays and segments what the list walk (ACCEL_BRUTE) gives.  Every case renders twice
in one context: the second launch finds the context's buffers in place, copies the nodes into LDS again and runs, like the first, as two
workgroups of 768 threads per CU.  Each frame is also rendered as a single row (one part of 64 with one-row blocks): 96 pixels in units
of 64 items, so waves start with fewer units than lanes."""
import numpy as np
import pytest

import rtw_amd as R
from tests.test_node_format_cpu import hand_scene

pytestmark = pytest.mark.gpu
LARGE_BUILDS = {"render_bvh<0,1,1,0>", "render_bvh<0,1,2,0>", "render_bvh<0,1,3,0>"}     # the builds whose workgroup is RTW_BLOCK_LARGE threads
TREE_COUNTERS = ("camera_rays", "segments", "sphere_tests", "node_tests", "nan_pixels", "rows", "quad_tests")
PATH_COUNTERS = ("camera_rays", "segments", "nan_pixels", "rows", "quad_tests")       # what a list walk counts the way a tree walk does
W, H, SPP, DEPTH = 96, 64, 16, 50


def book1():
    scene = R.Scene.generate(R.SCENE_C2, 42)
    cam, p = R.default_view(R.SCENE_C2)
    f = p.width / W
    for k in range(3):
        cam.pixel00[k] = cam.pixel00[k] - 0.5 * (cam.delta_u[k] + cam.delta_v[k]) + 0.5 * f * (cam.delta_u[k] + cam.delta_v[k])
        cam.delta_u[k] *= f
        cam.delta_v[k] *= f
    p.width, p.height, p.samples, p.depth = W, H, SPP, DEPTH
    return scene, cam, p


def three_spheres():
    vp = R.Viewport.new_from_res(W, H, SPP, DEPTH, 1.0, vfov=60.0, origin=(0.0, 0.3, 1.5), direction=(0.0, -0.1, -1.0), lens_radius=0.0)
    return hand_scene(2), vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)      # the ground and two spheres: a root over two leaves


SCENES = {"book1": book1, "three spheres": three_spheres}
PARTS = {"whole frame": (8, 0, 1), "one row": (1, 37, 64)}       # (row_block, part_index, part_count); 64 rows: part 37 of 64 is row 37


def counters(st, names):
    return {k: getattr(st, k) for k in names}


@pytest.fixture(scope="module")
def renders(gpu):
    """{(scene, part): {"f32": [first, second], "f16": one, "list": one}}, each an (image, stats, build, node format); rendered once."""
    out = {}
    try:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        for sname, make in SCENES.items():
            scene, cam, p = make()
            p.gamma = 1.0
            gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
            for pname, (row_block, index, count) in PARTS.items():
                q = R.RtwParams.from_buffer_copy(p)
                q.row_block, q.part_index, q.part_count = row_block, index, count

                def once(accel, fmt):
                    q.accel = accel
                    gpu.set_option(R.OPT_NODE_FORMAT, fmt)
                    img, st = gpu.render(cam, q)
                    return img, st, gpu.last_render_build(), gpu.last_node_format()

                out[sname, pname] = {"f32": [once(R.ACCEL_BVH, 2), once(R.ACCEL_BVH, 2)], "f16": once(R.ACCEL_BVH, 1), "list": once(R.ACCEL_BRUTE, 0)}
    finally:
        gpu.set_option(R.OPT_NODE_FORMAT, 0)
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    return out


CASES = [(s, p) for s in SCENES for p in PARTS]


@pytest.mark.parametrize("sname,pname", CASES)
def test_the_build_is_a_768_thread_one(renders, sname, pname):
    r = renders[sname, pname]
    for img, st, build, fmt in r["f32"]:
        assert build in LARGE_BUILDS and fmt == R.NODE_FORMAT_F32, (build, fmt)
        assert st.node_tests > 0 and st.segments > st.camera_rays > 0
    assert r["f16"][2] not in LARGE_BUILDS and r["f16"][2].startswith("render_bvh") and r["f16"][3] == R.NODE_FORMAT_F16, r["f16"][2:]
    assert r["list"][2].startswith("render_brute"), r["list"][2]


@pytest.mark.parametrize("sname,pname", CASES)
def test_two_renders_in_one_context_agree(renders, sname, pname):
    (ia, sa, _, _), (ib, sb, _, _) = renders[sname, pname]["f32"]
    assert ia.tobytes() == ib.tobytes()
    assert counters(sa, TREE_COUNTERS) == counters(sb, TREE_COUNTERS)


@pytest.mark.parametrize("sname,pname", CASES)
def test_frame_and_counters_are_the_f16_walk_s(renders, sname, pname):
    r = renders[sname, pname]
    for img, st, _, _ in r["f32"]:
        assert img.tobytes() == r["f16"][0].tobytes()
        assert counters(st, TREE_COUNTERS) == counters(r["f16"][1], TREE_COUNTERS)


@pytest.mark.parametrize("sname,pname", CASES)
def test_frame_and_counters_are_the_list_walk_s(renders, sname, pname):
    r = renders[sname, pname]
    for img, st, _, _ in r["f32"]:
        assert img.tobytes() == r["list"][0].tobytes()
        assert counters(st, PATH_COUNTERS) == counters(r["list"][1], PATH_COUNTERS)


@pytest.mark.parametrize("sname", list(SCENES))
def test_the_row_is_the_frame_s_row(renders, sname):
    whole, row = renders[sname, "whole frame"]["f32"][0], renders[sname, "one row"]["f32"][0]
    assert row[0].shape == (1, W, 3) and row[1].rows == 1
    assert row[0][0].tobytes() == whole[0][PARTS["one row"][1]].tobytes()
