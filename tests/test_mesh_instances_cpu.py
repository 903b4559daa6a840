"""Mesh placements on the host (rtw_mesh_instance_hits, rtw_mesh_instances_validate; no GPU) against the numpy f32 restatement of
tests/mesh_inst_common.py.  Every comparison is on the bits (a NaN in both counts as equal); no tolerance anywhere."""
import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as M

F = np.float32
OK, E_INVALID, E_NO_SCENE = 0, -1, -6


@pytest.fixture(scope="module")
def standard():
    T, pl, rays = M.standard_mesh(), M.standard_placements(), M.standard_rays()
    return T, pl, rays, M.placement_hits(T, pl, rays[:, :3], rays[:, 3:])


def test_the_standard_rays_meet_the_input_conditions(standard):
    T, pl, rays, want = standard
    assert len(rays) == 4096 and T.k == 80 and len(pl) == 6
    M.assert_input_quality(want)
    d = rays[:, 3:]
    assert ((d == 0).any(axis=1) & want["found"]).sum() >= 20          # zero direction components that hit
    assert np.isnan(rays[-2]).any() and (rays[-1, 3:] == 0).all()
    # a tie between placements (the coincident pair answers the same t: the earlier keeps it) and a strictly-closer replacement (the
    # earlier of the pair takes over from the third, which the same ray hits farther away)
    only = lambda k: M.placement_hits(T, [pl[k]], rays[:, :3], rays[:, 3:])
    third, pair = only(2), only(4)
    both = third["found"] & pair["found"]
    assert (both & (pair["t"] < third["t"]) & (want["placement"] == 4)).sum() >= 5
    assert (both & (pair["t"] > third["t"]) & (want["placement"] == 2)).sum() >= 5


def test_host_form_equals_the_restatement(standard):
    T, pl, rays, want = standard
    got = R.mesh_instance_hits(T.pods(), pl, rays, M.MINT, M.MAXT)
    M.assert_hits_equal(got, M.as_outputs(want), "host form against the restatement")
    assert np.isnan(got[0][-2]) and got[1][-2] == 0 and got[2][-2] == 0   # the NaN ray: every test accepts it, the first in order keeps it
    assert got[1][-1] == -1 and np.isposinf(got[0][-1])                 # the zero direction: |n . d| <= 1e-8 everywhere


def test_host_form_without_normals(standard):
    T, pl, rays, want = standard
    got = R.mesh_instance_hits(T.pods(), pl, rays[:256], M.MINT, M.MAXT, normals=False)
    assert len(got) == 3
    M.assert_hits_equal(got, tuple(x[:256] for x in M.as_outputs(want)[:3]), "no normals")


def test_identity_placement_is_the_triangle_group(standard):
    """q = (1, 0, 0, 0) at the origin: q.rotate(v) gives v back except for the sign of a zero, so for rays without zero components t and the
    triangle are rtw_triangle_hits'."""
    T, pl, rays, _ = standard
    plain = rays[(rays != 0).all(axis=1) & ~np.isnan(rays).any(axis=1)]
    assert len(plain) > 3000
    t, p, tri = R.mesh_instance_hits(T.pods(), [([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])], plain, M.MINT, M.MAXT, normals=False)
    t0, tri0 = R.triangle_hits(T.pods(), plain, M.MINT, M.MAXT)
    assert (tri0 >= 0).sum() >= 100
    assert np.array_equal(t.view(np.uint32), t0.view(np.uint32)) and np.array_equal(tri, tri0) and np.array_equal(p, np.where(tri0 >= 0, 0, -1))


def test_every_status_of_validate(standard):
    T, pl, _, _ = standard
    tris = T.pods()
    v = R.mesh_instances_validate
    assert v(tris, pl) == OK
    assert v(tris, None) == OK                                           # NULL / 0 clears
    assert v(None, pl) == E_NO_SCENE and v([], None) == E_NO_SCENE       # no triangles
    assert v(tris, [([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])]) == E_INVALID             # len == 0
    assert v(tris, [([0.0, 0.0, 0.0], [3e38, 3e38, 0.0, 0.0])]) == E_INVALID           # len overflows
    assert v(tris, [([0.0, 0.0, 0.0], [1e-30, 0.0, 0.0, 0.0])]) == E_INVALID           # len underflows to 0
    for bad in (np.nan, np.inf, -np.inf):
        assert v(tris, [([0.0, bad, 0.0], [1.0, 0.0, 0.0, 0.0])]) == E_INVALID
        assert v(tris, [pl[0], ([0.0, 0.0, 0.0], [1.0, 0.0, bad, 0.0])]) == E_INVALID
    textured = T.pods()
    textured[7].pod.tex = 0
    assert v(textured, pl) == E_INVALID and v(textured, None) == OK
    L = R.lib()
    arr, n = R._triangle_array(tris)
    parr, pn = R._placement_array(pl)
    assert L.rtw_mesh_instances_validate(arr, n, None, 3) == E_INVALID    # a NULL / n mismatch, either way
    assert L.rtw_mesh_instances_validate(arr, n, parr, 0) == E_INVALID
    assert L.rtw_mesh_instances_validate(None, n, parr, pn) == E_INVALID
    big = (R.RtwMeshInstance * (R.MAX_MESH_INSTANCES + 1))()
    for k in range(len(big)):
        big[k].quat[0] = 1.0
    assert L.rtw_mesh_instances_validate(arr, n, big, R.MAX_MESH_INSTANCES + 1) == E_INVALID
    assert L.rtw_mesh_instances_validate(arr, n, big, R.MAX_MESH_INSTANCES) == OK


def test_host_form_refuses_bad_arguments(standard):
    T, pl, rays, _ = standard
    with pytest.raises(R.RtwError):
        R.mesh_instance_hits(T.pods(), None, rays[:4], M.MINT, M.MAXT)
    with pytest.raises(R.RtwError):
        R.mesh_instance_hits(T.pods(), [([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])], rays[:4], M.MINT, M.MAXT)
