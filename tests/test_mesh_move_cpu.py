"""The refit of the top-level tree over mesh placements on the host (rtw_mesh_top_refit: the functions and the schedule the device runs,
compiled for the host): against the builder's bytes, against a numpy float64 restatement of the boxes, the invalid-pose rule, the reach, tiny
and huge quaternions, statuses.  Bits everywhere, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import mesh_move_common as MM

F = np.float32
E_INVALID, E_NO_SCENE = -1, -6

CASES = MM.cases()


@pytest.fixture(scope="module")
def built():
    """name -> (mesh pods, placements, mesh_top_dump's answer, the mesh tree's root)."""
    out = {}
    for name, (T, pl) in CASES.items():
        pods = T.pods()
        out[name] = (pods, pl, R.mesh_top_dump(pods, pl), R.triangle_bvh_dump(pods)[0][0])
    return out


# ---- the same poses: the builder's bytes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_refit_to_the_same_poses_returns_the_builders_bytes(built, name):
    pods, pl, (nodes, order, depth, lw), root = built[name]
    assert lw == 0
    got, rows, list_walk, bad = R.mesh_top_refit(pods, pl, MM.as_array(pl))
    assert (list_walk, bad) == (0, 0)
    assert MM.same_bytes(got, nodes), name
    assert MM.same_bytes(rows, MM.rows_of(MM.as_array(pl))), name           # mesh_rows' rows, restated
    # ... and with nothing given: the boxes are formed again from the rows the list gave
    again = R.mesh_top_refit(pods, pl)
    assert MM.same_bytes(again[0], nodes) and MM.same_bytes(again[1], rows)


def test_the_outlier_chain_has_leaves_at_very_uneven_depths(built):
    _, pl, (nodes, order, depth, _), _ = built["outliers20"]
    assert len(nodes) == 2 * len(pl) - 7 and depth >= 10
    h = MM.heights(nodes)
    assert h[0] == depth and (h[nodes["leaf"] != 0] == 0).all()


# ---- the motions: the restatement's boxes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", list(MM.MOTIONS))
@pytest.mark.parametrize("name", list(CASES))
def test_every_node_box_equals_the_restatement(built, name, motion):
    pods, pl, (nodes, order, _, _), root = built[name]
    moved = MM.MOTIONS[motion](MM.as_array(pl))
    got, rows, list_walk, bad = R.mesh_top_refit(pods, pl, moved)
    assert (list_walk, bad) == (0, 0)
    assert MM.same_bytes(rows, MM.rows_of(moved))
    want = MM.expected_nodes(nodes, order, root, rows)
    assert MM.same_bytes(got, want), (name, motion, int((got["lo"] != want["lo"]).sum()), int((got["hi"] != want["hi"]).sum()))
    assert np.array_equal(got["skip"], nodes["skip"]) and np.array_equal(got["leaf"], nodes["leaf"])       # the topology is untouched
    if motion == "turn_and_shift":
        assert not MM.same_bytes(got, nodes)


# ---- the mesh moves too ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid5", "grid64"])
def test_with_ouv_the_boxes_follow_the_refitted_root(built, name):
    pods, pl, (nodes, order, _, _), root = built[name]
    T = CASES[name][0]
    ouv, moved_T = MM.sine_ouv(T)
    moved = MM.turn_and_shift(MM.as_array(pl))
    got, rows, list_walk, bad = R.mesh_top_refit(pods, pl, moved, ouv)
    assert (list_walk, bad) == (0, 0)
    new_root = R.triangle_bvh_refit(pods, ouv)[0][0]
    assert not MM.same_bytes(new_root, root)
    assert MM.same_bytes(got, MM.expected_nodes(nodes, order, new_root, rows))
    # where the topology coincides -- the leaves' boxes are a function of their placements alone -- the tree built for the moved mesh under the
    # moved poses holds the same boxes
    fresh, forder, _, flw = R.mesh_top_dump(moved_T.pods(), MM.as_list(moved))
    assert flw == 0
    box = {tuple(sorted(order[(l >> 3):(l >> 3) + (l & 7)].tolist())): (lo.tobytes(), hi.tobytes())
           for l, lo, hi in zip(got["leaf"], got["lo"], got["hi"]) if l}
    shared = 0
    for l, lo, hi in zip(fresh["leaf"], fresh["lo"], fresh["hi"]):
        key = tuple(sorted(forder[(l >> 3):(l >> 3) + (l & 7)].tolist())) if l else None
        if key in box:
            shared += 1
            assert box[key] == (lo.tobytes(), hi.tobytes()), key
    assert MM.same_bytes(got[0:1]["lo"], fresh[0:1]["lo"]) and MM.same_bytes(got[0:1]["hi"], fresh[0:1]["hi"])    # the root bounds the same set
    print(f"\n[mesh move] {name}: {shared} leaves hold the same placements in both trees")
    # ouv alone: the rows stay, the boxes follow the root
    got2, rows2, _, _ = R.mesh_top_refit(pods, pl, None, ouv)
    assert MM.same_bytes(rows2, MM.rows_of(MM.as_array(pl)))
    assert MM.same_bytes(got2, MM.expected_nodes(nodes, order, new_root, rows2))


# ---- invalid poses -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid5", "grid64", "outliers20"])
def test_an_invalid_pose_keeps_its_old_rows_and_the_others_move(built, name):
    pods, pl, _, _ = built[name]
    n = len(pl)
    old = MM.as_array(pl)
    moved = MM.turn_and_shift(old)
    where = [0, n // 2, n - 1]
    bad_list = MM.spoil(moved, where)
    subst = moved.copy()
    subst[where] = old[where]
    got, rows, list_walk, bad = R.mesh_top_refit(pods, pl, bad_list)
    want, wrows, wlw, wbad = R.mesh_top_refit(pods, pl, subst)
    assert bad == 3 and wbad == 0 and list_walk == wlw == 0
    assert MM.same_bytes(got, want) and MM.same_bytes(rows, wrows)
    assert MM.same_bytes(rows[where], MM.rows_of(old)[where])
    # an all-valid list afterwards
    assert R.mesh_top_refit(pods, pl, moved)[3] == 0


# ---- reach -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_position_beyond_the_reach_sets_bit_1_and_a_move_back_clears_it(built):
    pods, pl, (nodes, order, _, _), root = built["grid64"]
    far = MM.as_array(pl)
    far[17, 0] = F(2.0 ** 39)
    got, rows, list_walk, bad = R.mesh_top_refit(pods, pl, far)
    assert (list_walk, bad) == (2, 0)
    assert MM.placement_boxes(root, rows)[2].tolist() == [k == 17 for k in range(64)]
    # (the host form refits the tree built for `placements`, so "back" is the refit of the far list's tree to the near poses)
    back, brows, blw, bbad = R.mesh_top_refit(pods, MM.as_list(far), MM.as_array(pl))
    far_nodes, far_order, _, flw = R.mesh_top_dump(pods, MM.as_list(far))
    assert flw == 1 and (blw, bbad) == (0, 0)
    assert MM.same_bytes(back, MM.expected_nodes(far_nodes, far_order, root, brows))


# ---- tiny and huge quaternions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0 ** -60, 2.0 ** -70, 2.0 ** 60])
def test_rows_of_tiny_and_huge_quaternions_are_mesh_rows_bytes(built, scale):
    """At 2^-70 the squares of the components are f32 denormals (2^-140 and below): the len is formed from them, or from zeros where they are
    flushed.  The rows must be mesh_rows' bytes, or the pose refused exactly where mesh_rows refuses."""
    pods, pl, _, _ = built["grid64"]
    moved = MM.as_array(pl)
    moved[:, 3:] = (moved[:, 3:] * F(scale)).astype(F)
    sq = (moved[:, 3:].astype(np.float64) ** 2)
    if scale == 2.0 ** -70:
        assert ((sq > 0) & (sq < 2.0 ** -126)).any(), "no denormal square among the inputs"
    got, rows, list_walk, bad = R.mesh_top_refit(pods, pl, moved)
    old_rows = MM.rows_of(MM.as_array(pl))
    refused = np.array([R.mesh_instances_validate(pods, [p]) != 0 for p in MM.as_list(moved)])
    assert bad == int(refused.sum())
    want = np.where(refused[:, None], old_rows, MM.rows_of(moved))
    assert MM.same_bytes(rows, want)
    # the host's own rows for the accepted poses: a list of them alone, through the builder
    keep = [p for p, r in zip(MM.as_list(moved), refused) if not r]
    assert len(keep) >= 32
    assert MM.same_bytes(R.mesh_top_refit(pods, keep)[1], rows[~refused])


# ---- statuses --------------------------------------------------------------------------------------------------------------------------------------
def test_statuses(built):
    L = R.lib()
    pods, pl, (nodes, _, _, _), _ = built["grid5"]
    arr, n = R._triangle_array(pods)
    parr, pn = R._placement_array(pl)
    mv = MM.as_array(pl)
    nn = C.c_uint32()
    buf = np.zeros(2 * pn, R.TOP_NODE)
    assert L.rtw_mesh_top_refit(arr, 0, parr, pn, mv.ctypes.data, None, None, 0, C.byref(nn), None, None, None) == E_NO_SCENE
    assert L.rtw_mesh_top_refit(arr, n, parr, 0, mv.ctypes.data, None, None, 0, C.byref(nn), None, None, None) == E_INVALID
    assert L.rtw_mesh_top_refit(arr, n, None, pn, mv.ctypes.data, None, None, 0, C.byref(nn), None, None, None) == E_INVALID
    assert L.rtw_mesh_top_refit(arr, n, parr, pn, mv.ctypes.data, None, None, 0, C.byref(nn), None, None, None) == 0 and nn.value == len(nodes)
    assert L.rtw_mesh_top_refit(arr, n, parr, pn, mv.ctypes.data, None, buf.ctypes.data, len(nodes) - 1, None, None, None, None) == E_INVALID
    assert L.rtw_mesh_top_refit(arr, n, parr, pn, mv.ctypes.data, None, buf.ctypes.data, len(nodes), None, None, None, None) == 0
    assert MM.same_bytes(buf[:len(nodes)], nodes)
    bad = [(p, [0.0, 0.0, 0.0, 0.0]) for p, _ in pl]                      # the list itself must be one set_mesh_instances accepts
    barr, bn = R._placement_array(bad)
    assert L.rtw_mesh_top_refit(arr, n, barr, bn, mv.ctypes.data, None, None, 0, C.byref(nn), None, None, None) == E_INVALID
    with pytest.raises(ValueError):
        R.mesh_top_refit(pods, pl, mv[:4])
    with pytest.raises(ValueError):
        R.mesh_top_refit(pods, pl, None, np.zeros((3, 9), F))
    assert R.OPT_MESH_CLIMB == 13
    for name in ("rtw_ctx_move_mesh_instances", "rtw_ctx_mesh_top_dump", "rtw_mesh_top_refit"):
        assert hasattr(L, name)


def test_the_motions_keep_the_hit_share_of_the_standard_rays():
    """The inputs of the GPU tests (tests/test_gpu_mesh_move.py), checked here on the host list walk: between 0.2 and 0.8 of the 4096 rays hit
    after every motion but "shrink to a point", which is exempt -- it leaves one spot to hit."""
    for n in (6, 64):
        T, pl = MI.standard_mesh(), (MI.standard_placements() if n == 6 else MM.grid_n(n))
        rays = MI.standard_rays(placements=pl)
        for motion, fn in MM.MOTIONS.items():
            moved = MM.as_list(fn(MM.as_array(pl)))
            share = float((R.mesh_instance_hits(T.pods(), moved, rays, MI.MINT, MI.MAXT)[1] >= 0).mean())
            print(f"\n[mesh move] {n} placements, {motion}: {share:.3f} of the rays hit")
            if motion != "shrink_to_a_point":
                assert 0.2 <= share <= 0.8, (n, motion, share)
