"""The any-hit host forms (rtw_triangle_occluded, rtw_mesh_instance_occluded: the source of rtw_ctx_scene_occluded's triangle and placement
groups, compiled for the host) against the existing closest-hit host forms, exactly -- and the conditions the GPU tests put on their inputs,
checked with the oracle and the existing host forms alone.  No GPU here."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import occluded_common as OC
from tests import query_edges_common as QE
from tests import refit_common as RC
from tests.test_gpu_scene_hits import oracle_hits

F = np.float32
E_INVALID = -1


# ---- conditions on the inputs of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.FULL_SCENES)
def test_the_full_scenes_exercise_both_outcomes(oracle, name):
    s = OC.share(OC.scene_reference(oracle, name))
    print(f"\n{name}: {s:.1%} of the rays are occluded")
    assert 0.2 <= s <= 0.8, (name, s)


@pytest.mark.parametrize("group", OC.GROUPS)
def test_each_group_decides_on_its_own(oracle, group):
    occ = OC.scene_reference(oracle, group)
    print(f"\n{group}: {int(occ.sum())} of {len(occ)} rays occluded")
    assert occ.sum() >= 20 and (~occ).sum() >= 20, (group, int(occ.sum()))


def test_a_short_range_turns_occluded_rays_free(oracle):
    far, near = OC.scene_reference(oracle, "field"), OC.scene_reference(oracle, "field, short range")
    print(f"\nfield: {OC.share(far):.1%} occluded at maxt 1e30, {OC.share(near):.1%} at {OC.SHORT_MAXT}")
    assert (far & ~near).sum() >= 20 and not (near & ~far).any()


def test_the_segments_exercise_both_outcomes(oracle):
    p, q = OC.segment_pairs()
    assert len(p) == 512
    occ = OC.occluded_of(oracle_hits(oracle, QE.field_scene(), OC.segment_rays(p, q), 0.0, OC.SEG_LO, OC.SEG_HI)[1])
    print(f"\nsegments: {OC.share(occ):.1%} of the pairs are occluded")
    assert 0.2 <= OC.share(occ) <= 0.8


@pytest.mark.parametrize("name", ["standard", "grid8"])
def test_the_placements_exercise_both_outcomes(name):
    s = OC.share(OC.placement_reference(name))
    print(f"\n{name}: {s:.1%} of the rays are occluded")
    assert 0.2 <= s <= 0.8


# ---- triangles -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.MESHES))
def test_triangle_occluded_equals_triangle_hits(name):
    tris, v, f = OC.mesh_triangles(name)
    tris = list(tris)
    rays = OC.mesh_rays(v, f)
    assert (np.sum(rays[:, 3:] == 0.0, axis=1) >= 1).sum() > 50            # exactly-zero direction components
    assert (~QE.tri_ordinary(rays, MI.MAXT)).sum() > 50                    # rays tri_ray_ordinary refuses
    assert np.isnan(rays).any(axis=1).sum() >= 3
    t, idx = R.triangle_hits(tris, rays, MI.MINT, MI.MAXT)
    want = OC.occluded_of(idx)
    assert want.sum() >= 20 and (~want).sum() >= 20, (name, int(want.sum()))
    occ, st = R.triangle_occluded(tris, rays, MI.MINT, MI.MAXT)
    OC.assert_same(occ, want, name)
    assert st.segments == len(rays) and st.quad_tests > 0
    assert st.node_tests > 0                                               # the tree is in use (a single leaf is a node too)
    # the range edges about a known hit: its t as mint, as maxt, and the next f32 on either side
    k = int(np.flatnonzero(want & np.isfinite(t) & QE.tri_ordinary(rays, MI.MAXT))[0])
    tk = float(t[k])
    seen = set()
    for mint, maxt in ((tk, MI.MAXT), (QE.above(tk), MI.MAXT), (QE.below(tk), MI.MAXT), (MI.MINT, tk), (MI.MINT, QE.below(tk)), (MI.MINT, QE.above(tk)),
                       (tk, tk), (MI.MAXT, MI.MINT)):
        w = OC.occluded_of(R.triangle_hits(tris, rays, mint, maxt)[1])
        OC.assert_same(R.triangle_occluded(tris, rays, mint, maxt)[0], w, (name, mint, maxt))
        seen.add((mint, maxt, bool(w[k])))
    assert (tk, tk, True) in seen and (MI.MAXT, MI.MINT, False) in seen
    # a range the tree does not serve (maxt = +inf, NaN mint): the list, the same answer
    for mint, maxt in ((MI.MINT, float("inf")), (float("nan"), MI.MAXT)):
        occ2, st2 = R.triangle_occluded(tris, rays, mint, maxt)
        OC.assert_same(occ2, OC.occluded_of(R.triangle_hits(tris, rays, mint, maxt)[1]), (name, mint, maxt))
        assert st2.node_tests == 0


# ---- placements ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.PLACEMENTS)
def test_mesh_instance_occluded_equals_mesh_instance_hits(name):
    pods, pl, rays = OC.placement_case(name)
    pods = list(pods)
    want = OC.placement_reference(name)
    assert want.any() and not want.all()
    occ, st = R.mesh_instance_occluded(pods, pl, rays, MI.MINT, MI.MAXT)
    OC.assert_same(occ, want, name)
    # counters: an any-hit walk is a prefix of the closest-hit walk
    tree = R.mesh_instance_hits_tree(pods, pl, rays, MI.MINT, MI.MAXT, normals=False)[4]
    print(f"\n{name}: node visits {st.node_tests} any-hit / {tree.node_tests} closest-hit, triangle tests {st.quad_tests} / {tree.quad_tests}")
    assert 0 < st.node_tests <= tree.node_tests and st.quad_tests <= tree.quad_tests
    if name == "grid8":
        assert st.node_tests < tree.node_tests and st.quad_tests < tree.quad_tests
    if name == "refused":
        finite = np.isfinite(rays).all(axis=1)
        far = finite & (np.abs(rays[:, :3]).max(axis=1) > 2.0 ** 38)
        assert far.sum() > 50 and (~finite).sum() > 50 and (finite & ~rays[:, 3:].any(axis=1)).sum() > 50


# ---- order independence and statuses -----------------------------------------------------------------------------------------------------------
def test_the_answer_does_not_depend_on_the_order_of_the_rays():
    pods, pl, rays = OC.placement_case("grid8")
    pods = list(pods)
    want = OC.placement_reference("grid8")
    tris, v, f = OC.mesh_triangles("terrain12")
    trays = OC.mesh_rays(v, f)
    twant = R.triangle_occluded(list(tris), trays, MI.MINT, MI.MAXT)[0]
    for perm in (np.arange(len(rays))[::-1], np.random.default_rng(5).permutation(len(rays))):
        OC.assert_same(R.mesh_instance_occluded(pods, pl, np.ascontiguousarray(rays[perm]), MI.MINT, MI.MAXT)[0], want[perm], "placements")
        OC.assert_same(R.triangle_occluded(list(tris), np.ascontiguousarray(trays[perm]), MI.MINT, MI.MAXT)[0], twant[perm], "triangles")


def test_statuses():
    L = R.lib()
    pods, pl, rays = OC.placement_case("standard")
    arr, n = R._triangle_array(list(pods))
    parr, pn = R._placement_array(pl)
    r4 = np.ascontiguousarray(rays[:4])
    rp = r4.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(4, np.uint8)
    a = (MI.MINT, MI.MAXT)
    assert L.rtw_triangle_occluded(arr, n, rp, 4, *a, out.ctypes.data, None) == R.RTW_OK
    assert L.rtw_triangle_occluded(None, n, rp, 4, *a, out.ctypes.data, None) == E_INVALID
    assert L.rtw_triangle_occluded(arr, n, None, 4, *a, out.ctypes.data, None) == E_INVALID
    assert L.rtw_triangle_occluded(arr, n, rp, 4, *a, None, None) == E_INVALID
    assert L.rtw_triangle_occluded(arr, n, rp, 0, *a, out.ctypes.data, None) == E_INVALID
    assert L.rtw_mesh_instance_occluded(arr, n, parr, pn, rp, 4, *a, out.ctypes.data, None) == R.RTW_OK
    assert L.rtw_mesh_instance_occluded(arr, n, parr, pn, None, 4, *a, out.ctypes.data, None) == E_INVALID
    assert L.rtw_mesh_instance_occluded(arr, n, parr, pn, rp, 4, *a, None, None) == E_INVALID
    assert L.rtw_mesh_instance_occluded(arr, n, parr, pn, rp, 0, *a, out.ctypes.data, None) == E_INVALID
    assert L.rtw_mesh_instance_occluded(arr, n, None, 0, rp, 4, *a, out.ctypes.data, None) == E_INVALID
    assert L.rtw_mesh_instance_occluded(None, n, parr, pn, rp, 4, *a, out.ctypes.data, None) == E_INVALID
    # the same statuses as the hit forms
    t, i = np.zeros(4, F), np.zeros(4, np.int32)
    assert L.rtw_triangle_hits(arr, n, rp, 0, *a, t.ctypes.data_as(C.POINTER(C.c_float)), i.ctypes.data_as(C.POINTER(C.c_int32))) == E_INVALID
    # an empty triangle list occludes nothing
    assert L.rtw_triangle_occluded(None, 0, rp, 4, *a, out.ctypes.data, None) == R.RTW_OK and not out.any()
