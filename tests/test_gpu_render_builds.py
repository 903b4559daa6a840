"""The render-kernel builds no other enumeration walks, each against the CPU oracle: SPEC 4, 5, 6 (the demo, Rust2 and serial
configurations) without quads or instances -- render_brute and render_bvh at NODES 0, 1, 2 --, and the GEOM builds of SPEC 0, 2, 4, 5, 6 --
render_brute and render_bvh at NODES 0, 1 --, each static and MOVING: 54 kernels.

A case declares its build (BUILDS is the table tests/test_render_builds_cpu.py holds against the library's own list), renders ONE frame
through the request that selects it, and asserts that Renderer.last_render_build() is that build, that segments and camera rays are the
oracle's, that node_tests > 0 exactly when the tree kernel ran, and that the frame is the oracle's bit for bit at gamma 1 (a NaN in both
counts as equal) -- every pixel, no tolerance: the oracle renders with the device's texel choice (RTW_ORACLE_FLAG_DEVICE_UV).  The scenes,
the cases and the conditions on them: tests/render_builds_common.py, tests/test_render_builds_cpu.py."""
import numpy as np
import pytest

import rtw_amd as R
from tests import builds_common as B
from tests import render_builds_common as RB
from tests.mesh_inst_common import same_nan

pytestmark = pytest.mark.gpu

BUILDS = frozenset(c[1] for c in RB.CASES)


@pytest.mark.parametrize("tag,geom,moving,cfg,nodes", [pytest.param(*c[1:], id=c[0]) for c in RB.CASES])
def test_build_against_the_oracle(gpu, tag, geom, moving, cfg, nodes):
    scene, cam = RB.view(geom, moving, cfg)
    ref, st_ref = RB.oracle_frame(geom, moving, cfg)
    p = RB.params(geom, moving, cfg)
    gpu.set_scene(scene, cam.time0, cam.time0 + cam.shutter)
    try:
        if nodes is None:
            p.accel = R.ACCEL_BRUTE
        else:
            p.accel = R.ACCEL_BVH
            gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
            gpu.set_option(R.OPT_LDS_GEOM, 1 if nodes == 2 else 0)
            if nodes == 0:
                p.flags |= R.FLAG_GLOBAL_NODES
        img, st = gpu.render(cam, p)
    finally:
        gpu.set_option(R.OPT_LIST_WALK_MAX, 48)
        gpu.set_option(R.OPT_LDS_GEOM, -1)
    B.ran(gpu, tag)
    assert st.segments == st_ref.segments and st.camera_rays == st_ref.camera_rays, (tag, st.segments, st_ref.segments, st.camera_rays)
    assert (st.node_tests > 0) == (nodes is not None), (tag, st.node_tests)
    same = same_nan(img, ref)
    assert img.shape == ref.shape and same.all(), (tag, f"{int((~same.all(axis=2)).sum())} pixels differ, first {np.argwhere(~same.all(axis=2))[:3].tolist()}")


def test_last_render_build_of_banded_partitioned_and_chunk_sums_renders(rtw):
    """RTW_E_INVALID before a context's first render; then the tag of a render cut into several bands of tile rows, of a row partition and
    of a RTW_FLAG_CHUNK_SUMS render (which leaves the specialised build for the generic one, or for SPEC 3 without textures)."""
    demo, common = RB.SPHERE_CONFIGS[0], RB.GEOM_CONFIGS[0]
    scene, cam = RB.view(False, False, demo)
    plain = R.Scene([scene._spheres[i] for i in range(1, scene.n_spheres)])            # (without the textured ground)
    with rtw.Renderer(0) as r:
        with pytest.raises(R.RtwError) as e:
            r.last_render_build()
        assert e.value.status == -1
        r.set_scene(scene)
        r.set_option(R.OPT_LIST_WALK_MAX, 0)
        r.set_option(R.OPT_LDS_GEOM, 1)
        p = RB.params(False, False, demo)
        whole, st = r.render(cam, p)
        B.ran(r, B.bvh(False, 2, 4, False), "whole")
        r.set_option(R.OPT_SAMPLE_BANK_GB, 0.0001)                 # a tile row's bank is 14 tiles x 4 samples x 768 bytes: 2 of the 8 tile rows per band
        banded, st_b = r.render(cam, p)
        B.ran(r, B.bvh(False, 2, 4, False), "banded")
        assert np.array_equal(banded.view(np.uint32), whole.view(np.uint32)) and st_b.segments == st.segments
        r.set_option(R.OPT_SAMPLE_BANK_GB, 48)
        p.row_block, p.part_index, p.part_count = 8, 1, 3
        part, _ = r.render(cam, p)
        B.ran(r, B.bvh(False, 2, 4, False), "partition")
        assert np.array_equal(part.view(np.uint32), whole[[j for j in range(RB.HEIGHT) if (j // 8) % 3 == 1]].view(np.uint32))
        p = RB.params(False, False, common)
        p.flags = R.FLAG_CHUNK_SUMS
        r.render(cam, p)
        B.ran(r, B.bvh(False, 2, 0, False), "chunk sums, textured")
        p.accel = R.ACCEL_BRUTE
        r.render(cam, p)
        B.ran(r, B.brute(False, 0, False), "chunk sums, textured, list walk")
        r.set_scene(plain)
        p.accel = R.ACCEL_BVH
        r.render(cam, p)
        B.ran(r, B.bvh(False, 2, 3, False), "chunk sums")
        p.flags = 0
        r.render(cam, p)
        B.ran(r, B.bvh(False, 2, 1, False), "common configuration")
