"""The refit of the triangle tree on the host (rtw_triangle_bvh_dump, rtw_triangle_bvh_refit: the functions and the schedule the device
runs, compiled for the host): identity with the builder, the restated boxes, list_walk, statuses.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import refit_common as RC

E_INVALID = -1


@pytest.mark.parametrize("name", list(RC.MESHES))
def test_tree_shapes_are_the_tables(name):
    v, f, nodes, depth = RC.mesh(name)
    dump, order, dp, lw = R.triangle_bvh_dump(R.Triangle.from_mesh(v, f))
    assert (len(dump), dp, lw) == (nodes, depth, 0)
    assert sorted(order.tolist()) == list(range(len(f)))
    assert R.triangle_bvh_validate(R.Triangle.from_mesh(v, f)) == (0, nodes, depth, 0)


@pytest.mark.parametrize("name", list(RC.MESHES))
def test_refit_to_the_same_vertices_is_the_builders_tree(name):
    v, f, _, _ = RC.mesh(name)
    tris = R.Triangle.from_mesh(v, f)
    dump, _, _, _ = R.triangle_bvh_dump(tris)
    nodes, lw = R.triangle_bvh_refit(tris, R.mesh_ouv(v, f))
    assert lw == 0
    assert RC.same_bytes(nodes, dump)


@pytest.mark.parametrize("name", list(RC.MESHES))
def test_refit_to_the_sine_wave_equals_the_restated_boxes(name):
    v, f, _, _ = RC.mesh(name)
    tris = R.Triangle.from_mesh(v, f)
    dump, order, _, _ = R.triangle_bvh_dump(tris)
    ouv = R.mesh_ouv(RC.sine_wave(v, f), f)
    nodes, lw = R.triangle_bvh_refit(tris, ouv)
    assert lw == 0
    want = RC.expected_nodes(dump, order, ouv)
    assert np.array_equal(nodes["skip"], dump["skip"]) and np.array_equal(nodes["leaf"], dump["leaf"])
    assert RC.same_bytes(nodes, want)
    assert not RC.same_bytes(nodes, dump)
    # ... and the restatement is the builder's arithmetic: on the undeformed mesh it gives the builder's own bytes
    assert RC.same_bytes(RC.expected_nodes(dump, order, R.mesh_ouv(v, f)), dump)


@pytest.mark.parametrize("name", list(RC.DEFORMATIONS))
def test_list_walk_follows_the_deformation_and_a_fresh_build(name):
    v, f, _, _ = RC.mesh("icosphere2")
    deform, walk = RC.DEFORMATIONS[name]
    tris = R.Triangle.from_mesh(v, f)
    w = deform(v, f)
    _, lw = R.triangle_bvh_refit(tris, R.mesh_ouv(w, f))
    assert lw == walk
    assert R.triangle_bvh_dump(R.Triangle.from_mesh(w, f))[3] == walk          # what set_triangles of the moved mesh says
    # back to the sane vertices: the tree may be used again (every refit starts from the builder's tree: the topology never changes)
    assert R.triangle_bvh_refit(R.Triangle.from_mesh(w, f), R.mesh_ouv(v, f))[1] == 0


def test_refit_boxes_contain_the_moved_triangles_whatever_the_old_shape():
    """Refit a tree built for one shape to another: every leaf box holds its triangles' restated boxes, every node its children."""
    v, f, _, _ = RC.mesh("terrain12")
    tris = R.Triangle.from_mesh(v, f)
    dump, order, _, _ = R.triangle_bvh_dump(tris)
    rng = np.random.default_rng(3)
    w = (v + rng.normal(scale=0.8, size=v.shape)).astype(np.float32)
    ouv = R.mesh_ouv(w, f)
    nodes, lw = R.triangle_bvh_refit(tris, ouv)
    assert lw == 0
    lo, hi = RC.tri_boxes(ouv)
    for i in range(len(nodes)):
        if nodes["leaf"][i]:
            first, cnt = int(nodes["leaf"][i]) >> 3, int(nodes["leaf"][i]) & 7
            for t in order[first:first + cnt]:
                assert (nodes["lo"][i] <= lo[t]).all() and (hi[t] <= nodes["hi"][i]).all()
        else:
            for c in (i + 1, int(nodes["skip"][i + 1])):
                assert (nodes["lo"][i] <= nodes["lo"][c]).all() and (nodes["hi"][c] <= nodes["hi"][i]).all()


def test_statuses():
    L = R.lib()
    v, f, n_nodes, _ = RC.mesh("row5")
    tris = R.Triangle.from_mesh(v, f)
    ouv = R.mesh_ouv(v, f)
    fp = ouv.ctypes.data_as(C.POINTER(C.c_float))
    nodes = np.zeros(n_nodes, R.TOP_NODE)
    nn = C.c_uint32()
    assert L.rtw_triangle_bvh_dump(None, 5, None, 0, None, None, None, None) == E_INVALID
    assert L.rtw_triangle_bvh_dump(tris.arr, 0, None, 0, None, None, None, None) == E_INVALID
    assert L.rtw_triangle_bvh_dump(tris.arr, 5, nodes.ctypes.data, n_nodes - 1, None, None, None, None) == E_INVALID
    assert L.rtw_triangle_bvh_dump(tris.arr, 5, None, 0, C.byref(nn), None, None, None) == 0 and nn.value == n_nodes      # sizes alone
    assert L.rtw_triangle_bvh_refit(None, 5, fp, None, 0, None, None) == E_INVALID
    assert L.rtw_triangle_bvh_refit(tris.arr, 0, fp, None, 0, None, None) == E_INVALID
    assert L.rtw_triangle_bvh_refit(tris.arr, 5, None, None, 0, None, None) == E_INVALID
    assert L.rtw_triangle_bvh_refit(tris.arr, 5, fp, nodes.ctypes.data, n_nodes - 1, None, None) == E_INVALID
    nn.value = 0
    assert L.rtw_triangle_bvh_refit(tris.arr, 5, fp, None, 0, C.byref(nn), None) == 0 and nn.value == n_nodes
    with pytest.raises(ValueError):
        R.triangle_bvh_refit(tris, ouv[:4])


def test_mesh_ouv_is_from_meshs_arithmetic():
    for name in RC.MESHES:
        v, f, _, _ = RC.mesh(name)
        w = RC.sine_wave(v, f)
        arr = R.Triangle.from_mesh(w, f)
        rec = np.frombuffer(arr.arr, dtype=np.float32).reshape(len(f), -1)
        ouv = R.mesh_ouv(w, f)
        assert ouv.shape == (len(f), 9) and ouv.dtype == np.float32
        assert RC.same_bytes(ouv, np.ascontiguousarray(rec[:, :9]))
    with pytest.raises(ValueError):
        R.mesh_ouv(np.zeros((3, 3), np.float32), [[0, 1, 3]])
