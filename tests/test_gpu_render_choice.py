"""What rtw_render_choice says is what a launch ran.

The smallest scenes that take each branch of the choice -- a root over two leaves, five leaves, the same with a moving sphere (the MOVING
builds, none of them a 768-thread one) and with a quad (the GEOM builds: no sphere geometry in LDS) -- rendered as 16 x 8 pixels under both
closest-hit strategies, RTW_FLAG_GLOBAL_NODES, and every value of RTW_OPT_NODE_FORMAT and RTW_OPT_LDS_GEOM.  The entry point gets the
tree's facts from rtw_bvh_dump and must name the build and the node format the context reports after the render."""
import itertools

import pytest

import rtw_amd as R
from tests import builds_common as B
from tests.test_bvh_builder_cpu import dump
from tests.test_node_format_cpu import hand_scene

pytestmark = pytest.mark.gpu


def with_moving():
    s = hand_scene(5)
    s.pod.spheres[2].velocity[1] = 0.25
    return s


def with_quad():
    s = hand_scene(5)
    return R.Scene([s.pod.spheres[i] for i in range(s.pod.n_spheres)], quads=[R.Quad.new((-1.0, -0.4, -3.0), (2.0, 0.0, 0.0), (0.0, 1.5, 0.0), R.SCATTER_M, (0.8, 0.3, 0.3))])


SCENES = {"two leaves": lambda: hand_scene(2), "five leaves": lambda: hand_scene(5), "a moving sphere": with_moving, "a quad": with_quad}


@pytest.mark.parametrize("name", list(SCENES))
def test_the_entry_point_names_the_launch(gpu, name):
    scene = SCENES[name]()
    vp = R.Viewport.new_from_res(16, 8, 1, 2, 1.0, vfov=60.0, origin=(0.0, 0.3, 1.5), direction=(0.0, -0.1, -1.0), lens_radius=0.0)
    cam, p = vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)
    d = dump(scene, cam.time0, cam.time0 + cam.shutter)
    f16 = int(d["nodes16"].any())
    tree = R.RtwTreeFacts(n_nodes=len(d["nodes"]), depth=d["depth"], n_spheres=scene.pod.n_spheres, has_f16=f16, has_planes=f16)
    moving = name == "a moving sphere"
    ran = set()
    try:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
        for accel, flags, fmt, lds_geom in itertools.product((R.ACCEL_BVH, R.ACCEL_BRUTE), (0, R.FLAG_GLOBAL_NODES), (0, 1, 2), (-1, 0, 1)):
            gpu.set_option(R.OPT_NODE_FORMAT, fmt)
            gpu.set_option(R.OPT_LDS_GEOM, lds_geom)
            p.accel, p.flags = accel, flags
            img, st = gpu.render(cam, p)
            facts = R.RtwRenderFacts(integrator=p.integrator, sampler=p.sampler, depth=p.depth, flags=flags, n_quads=scene.pod.n_quads)
            said = R.render_choice(facts, tree, lds_geom=lds_geom, node_format=fmt, moving=moving, accel=accel)
            assert (said["build"], said["node_format"]) == (gpu.last_render_build(), gpu.last_node_format()), (name, accel, flags, fmt, lds_geom, said)
            assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
            ran.add(said["build"])
    finally:
        gpu.set_option(R.OPT_NODE_FORMAT, 0)
        gpu.set_option(R.OPT_LDS_GEOM, -1)
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    # ... and the cases took every NODES outcome of the scene's SPEC (the common configuration; with a quad its GEOM build)
    assert ran == (B.family(2, True, moving=(moving,)) if name == "a quad" else B.family(1, False, moving=(moving,))), ran
