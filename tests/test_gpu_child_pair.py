"""The 768-thread render builds choosing the nearer child with one select (rtw_kernels.hip trav_descend, the f32 plane format's child
pair stored in both orders).

Which of the two stored orders a lane takes is the decision the rotate made before, so a frame of such a build must be the CPU oracle's bit
for bit, and frame, node visits and sphere tests what the f16 walk (RTW_OPT_NODE_FORMAT = 1) gives -- the two formats make the same
decisions by construction.  Small shapes: the bench scene at 64 x 48 x 4 spp, depth 50, through the bench camera and from inside the
sphere field looking along -x, along -z and along +x +z, so that camera rays alone cover every sign octant of 1/d (checked on the host
from the cameras' own pixel rays); and two coincident spheres, whose boxes are entered at the same distance: the `<=` tie of the descend."""
import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O

pytestmark = pytest.mark.gpu
LARGE_BUILDS = {"render_bvh<0,1,1,0>", "render_bvh<0,1,2,0>", "render_bvh<0,1,3,0>"}
W, H, SPP, DEPTH = 64, 48, 4, 50
INSIDE = {"along -x": (-1.0, -0.15, 0.0), "along -z": (0.0, -0.15, -1.0), "along +x +z": (1.0, -0.15, 1.0)}
EYE = (2.0, 0.55, 1.5)          # above the small spheres (tops at 0.4), 2.5 from the centres of the nearest large ones (radius 1)


def bench_view():
    scene = R.Scene.generate(R.SCENE_C2, 42)
    cam, p = R.default_view(R.SCENE_C2)
    f = p.width / W
    for k in range(3):
        cam.pixel00[k] = cam.pixel00[k] - 0.5 * (cam.delta_u[k] + cam.delta_v[k]) + 0.5 * f * (cam.delta_u[k] + cam.delta_v[k])
        cam.delta_u[k] *= f
        cam.delta_v[k] *= f
    p.width, p.height, p.samples, p.depth = W, H, SPP, DEPTH
    return scene, cam, p


def inside_view(direction):
    look_at = tuple(e + d for e, d in zip(EYE, direction))              # (the viewport's `direction` is the point the camera looks at)
    vp = R.Viewport.new_from_res(W, H, SPP, DEPTH, 1.0, vfov=100.0, origin=EYE, direction=look_at, lens_radius=0.0)
    return R.Scene.generate(R.SCENE_C2, 42), vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)


def coincident_spheres():
    """The ground (outside the tree) and two spheres with equal centres and radii: one inner node over two leaves with the same box."""
    sp = [R.Sphere.with_albedo((0.0, -100.5, -1.0), 100.0, (0.5, 0.5, 0.5), R.SCATTER_M),
          R.Sphere.with_albedo((0.0, 0.0, -1.5), 0.5, (0.9, 0.2, 0.1), R.SCATTER_M),
          R.Sphere.with_albedo((0.0, 0.0, -1.5), 0.5, (0.1, 0.3, 0.9), R.METALLIC_M)]
    vp = R.Viewport.new_from_res(W, H, SPP, DEPTH, 1.0, vfov=60.0, origin=(0.3, 0.3, 0.5), direction=(0.0, 0.0, -1.5), lens_radius=0.0)
    return R.Scene(sp), vp.camera(), vp.params(R.INTEGRATOR_GRADIENT, R.SAMPLER_ROW)


VIEWS = {"bench camera": bench_view, "coincident spheres": coincident_spheres, **{k: (lambda d=d: inside_view(d)) for k, d in INSIDE.items()}}


def test_the_inside_cameras_cover_every_octant():
    seen = set()
    for d in INSIDE.values():
        _, cam, p = inside_view(d)
        i, j = np.meshgrid(np.arange(p.width), np.arange(p.height))
        rays = (np.array(cam.pixel00[:]) + i[..., None] * np.array(cam.delta_u[:]) + j[..., None] * np.array(cam.delta_v[:]) - np.array(cam.origin[:])).reshape(-1, 3)
        rays = rays[(rays != 0).all(axis=1)]
        seen |= {tuple(s) for s in np.unique(np.signbit(rays), axis=0)}
    assert len(seen) == 8


@pytest.fixture(scope="module")
def renders(gpu):
    """{view: {"oracle": (image, stats), "f32": (image, stats, build, format), "f16": the same}}: each rendered once."""
    out = {}
    try:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
        for name, make in VIEWS.items():
            scene, cam, p = make()
            p.gamma, p.accel = 1.0, R.ACCEL_BVH
            gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)

            def once(fmt):
                gpu.set_option(R.OPT_NODE_FORMAT, fmt)
                img, st = gpu.render(cam, p)
                return img, st, gpu.last_render_build(), gpu.last_node_format()

            # (the bench scene as shipped, format 0; the three-sphere scene would ride the all-in-LDS f16 build: f32 planes asked for)
            out[name] = {"oracle": O.render(cam, scene, p, threads=8), "f32": once(2 if name == "coincident spheres" else 0), "f16": once(1)}
    finally:
        gpu.set_option(R.OPT_NODE_FORMAT, 0)
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
    return out


@pytest.mark.parametrize("name", list(VIEWS))
def test_the_build_is_the_768_thread_one(renders, name):
    _, st, build, fmt = renders[name]["f32"]
    assert build == "render_bvh<0,1,1,0>" and fmt == R.NODE_FORMAT_F32, (build, fmt)
    assert st.node_tests > 0 and st.segments > st.camera_rays == W * H * SPP
    f16 = renders[name]["f16"]
    assert f16[2] not in LARGE_BUILDS and f16[2].startswith("render_bvh") and f16[3] == R.NODE_FORMAT_F16, f16[2:]


@pytest.mark.parametrize("name", list(VIEWS))
def test_frame_is_the_oracle_s(renders, name):
    ref, st_ref = renders[name]["oracle"]
    img, st, _, _ = renders[name]["f32"]
    assert st.segments == st_ref.segments and st.camera_rays == st_ref.camera_rays
    assert img.tobytes() == ref.tobytes(), f"max |diff| {np.abs(img - ref).max()}"


@pytest.mark.parametrize("name", list(VIEWS))
def test_frame_and_visits_are_the_f16_walk_s(renders, name):
    img, st, _, _ = renders[name]["f32"]
    img16, st16, _, _ = renders[name]["f16"]
    assert img.tobytes() == img16.tobytes()
    assert (st.node_tests, st.sphere_tests, st.segments) == (st16.node_tests, st16.sphere_tests, st16.segments)


def test_the_coincident_boxes_are_both_entered(renders):
    """Every ray that hits the pair's box hits both boxes at one distance: the walk visits the root, then BOTH leaves (nearer first by the
    tie's rule, the other from the stack), so the tree's sphere tests -- beside one test of the ground per query -- are twice the hits."""
    _, st, _, _ = renders["coincident spheres"]["f32"]
    tree_tests = st.sphere_tests - st.segments           # one big sphere (the ground) is tested by every query
    assert tree_tests > 0 and tree_tests % 2 == 0 and st.node_tests == st.segments
