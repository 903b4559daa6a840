"""The top-level tree over mesh placements on the host (rtw_mesh_top_dump, rtw_mesh_instance_hits_tree; no GPU): its structure, its boxes, and
its walk -- the source the kernels compile -- against the list walk of rtw_mesh_instance_hits.  Every comparison of hits is on the bits."""
import numpy as np
import pytest

import rtw_amd as R
from tests import mesh_inst_common as M
from tests import mesh_top_common as MT
from tests import quat_common as QC

F = np.float32


def tree(T, pl, rays):
    return R.mesh_instance_hits_tree(T.pods(), pl, rays, M.MINT, M.MAXT)


def assert_tree_equals_list(T, pl, rays, what):
    want = R.mesh_instance_hits(T.pods(), pl, rays, M.MINT, M.MAXT)
    t, p, tri, nrm, st = tree(T, pl, rays)
    M.assert_hits_equal((t, p, tri, nrm), want, what)
    return want, st


# ---- structure -------------------------------------------------------------------------------------------------------------------------------
def stretched_mesh():
    """The standard mesh stretched 4 x 1 x 0.25 and moved 2.5 along x: off-centre, so that a turn of +pi/2 about y and one of -pi/2 put it in
    different places (the icosphere itself is symmetric, and the two boxes of a centred copy would coincide)."""
    S = M.standard_mesh()
    s = np.array([4.0, 1.0, 0.25], F)
    tris = [{"origin": (F(2.5) * np.array([1, 0, 0], F) + s * S.origin[k]).astype(F).tolist(), "u": (s * S.u[k]).astype(F).tolist(),
             "v": (s * S.v[k]).astype(F).tolist(), "material": "lambertian", "color": [0.5, 0.5, 0.5], "emitted": [0.0, 0.0, 0.0]} for k in range(S.k)]
    return M.TriSet(tris)


def turned_placements(n):
    """The first n positions of the 32 x 32 grid: even placements turned pi/2 about y (un-normalised: scaled), odd ones by the grid's quaternion."""
    turn = QC.from_axis(np.pi / 2, (0.0, 1.0, 0.0))
    return [(pos, (turn * F(1 + k % 3)).astype(F).tolist() if k % 2 == 0 else q) for k, (pos, q) in enumerate(MT.grid(32)[:n])]


@pytest.fixture(scope="module")
def dumps():
    T = stretched_mesh()
    return T, {n: (turned_placements(n), R.mesh_top_dump(T.pods(), turned_placements(n))) for n in MT.SIZES}


@pytest.mark.parametrize("n", MT.SIZES)
def test_structure_of_the_dump(dumps, n):
    _, (pl, (nodes, order, depth, list_walk)) = dumps[0], dumps[1][n]
    assert list_walk == 0 and len(order) == n and 1 <= len(nodes) <= 2 * n - 1
    assert sorted(order.tolist()) == list(range(n))                      # every placement in exactly one leaf slot ...
    covered = np.zeros(n, int)
    for i, nd in enumerate(nodes):
        assert i < nd["skip"] <= len(nodes)                              # skip links strictly increasing, ending at n_nodes
        if nd["leaf"]:
            first, cnt = int(nd["leaf"]) >> 3, int(nd["leaf"]) & 7
            assert 1 <= cnt <= 4 and first + cnt <= n and nd["skip"] == i + 1
            covered[first:first + cnt] += 1
        else:
            left, right = i + 1, int(nodes[i + 1]["skip"])
            assert right < len(nodes) and nodes[right]["skip"] == nd["skip"]
            for c in (left, right):                                      # every child box inside its parent
                assert (nodes[c]["lo"] >= nd["lo"]).all() and (nodes[c]["hi"] <= nd["hi"]).all(), (i, c)
    assert (covered == 1).all() and nodes[0]["skip"] == len(nodes)        # ... and every slot in exactly one leaf
    assert depth <= 48 and (n <= 4) == (len(nodes) == 1)


@pytest.mark.parametrize("n", MT.SIZES)
def test_leaf_boxes_hold_the_conjugate_image_of_the_mesh(dumps, n):
    T, (pl, (nodes, order, _, _)) = dumps[0], dumps[1][n]
    v = MT.vertices(T)
    for nd in nodes[nodes["leaf"] != 0]:
        first, cnt = int(nd["leaf"]) >> 3, int(nd["leaf"]) & 7
        lo, hi = nd["lo"].astype(np.float64), nd["hi"].astype(np.float64)
        for k in order[first:first + cnt]:
            w = MT.placed64(pl[k], v)
            assert (w >= lo).all() and (w <= hi).all(), (n, int(k))
    # the assertion can tell the two turns apart: placement 0 is turned pi/2 about y, and the box of its mesh turned by q instead of conj(q)
    # -- the reference's Instance::get_aabb -- does not hold where the mesh stands
    right, wrong = MT.placed64(pl[0], v), MT.placed64(pl[0], v, conj=False)
    outside = ((right < wrong.min(axis=0)) | (right > wrong.max(axis=0))).any(axis=1)
    assert outside.sum() >= len(v) // 2


@pytest.mark.parametrize("n", [8, 12, 20])
def test_a_chain_of_outliers_needs_more_nodes_than_placements(n):
    """Identity placements of a one-triangle mesh at x = 4^k: SAH splits the farthest one off at every level, so the tree holds 2 n - 7 nodes
    -- more than n.  2 n - 1 is the bound rtw.h states (every leaf holds a placement), and the dump fits a buffer of that size."""
    tri = M.TriSet([{"origin": [0.0, 0.0, 0.0], "u": [1.0, 0.0, 0.0], "v": [0.0, 1.0, 0.0], "material": "lambertian", "color": [0.5, 0.5, 0.5],
                     "emitted": [0.0, 0.0, 0.0]}])
    pl = [([4.0 ** k, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]) for k in range(n)]
    nodes, order, depth, list_walk = R.mesh_top_dump(tri.pods(), pl)
    assert list_walk == 0 and sorted(order.tolist()) == list(range(n))
    assert n < len(nodes) <= 2 * n - 1 and len(nodes) == 2 * n - 7, len(nodes)
    assert nodes[0]["skip"] == len(nodes) and all(i < nd["skip"] <= len(nodes) for i, nd in enumerate(nodes))
    # the C call: the count alone, a buffer of exactly that size, one node too few
    L, C = R.lib(), R.C
    arr, nt = R._triangle_array(tri.pods())
    parr, pn = R._placement_array(pl)
    nn = C.c_uint32()
    assert L.rtw_mesh_top_dump(arr, nt, parr, pn, None, 0, C.byref(nn), None, None, None) == 0 and nn.value == len(nodes)
    buf = np.zeros(nn.value, R.TOP_NODE)
    assert L.rtw_mesh_top_dump(arr, nt, parr, pn, buf.ctypes.data, nn.value, None, None, None, None) == 0 and buf.tobytes() == nodes.tobytes()
    assert L.rtw_mesh_top_dump(arr, nt, parr, pn, buf.ctypes.data, nn.value - 1, None, None, None, None) == -1
    # ... and the walk over such a tree is the list's
    rays = np.array([[4.0 ** (k % n) + 0.2, 0.3, -3.0, 0.01 * (k % 7 - 3), 0.0, 1.0] for k in range(256)], F)
    want, _ = assert_tree_equals_list(tri, pl, rays, "chain of outliers")
    assert (want[1] >= 0).sum() >= 100


def test_two_dumps_of_the_same_input_are_byte_equal(dumps):
    T, d = dumps
    for n in (5, 1024):
        pl, (nodes, order, depth, lw) = d[n]
        again = R.mesh_top_dump(T.pods(), pl)
        assert again[0].tobytes() == nodes.tobytes() and again[1].tobytes() == order.tobytes() and again[2:] == (depth, lw)


# ---- tree == list ------------------------------------------------------------------------------------------------------------------------------
def test_tree_equals_list_on_the_standard_inputs():
    T, pl, rays = M.standard_mesh(), M.standard_placements(), M.standard_rays()
    M.assert_input_quality(M.placement_hits(T, pl, rays[:, :3], rays[:, 3:]))
    want, st = assert_tree_equals_list(T, pl, rays, "standard inputs")
    assert (want[1] == 4).sum() >= 20 and (want[1] == 5).sum() == 0       # the coincident pair ties: the earlier keeps every hit
    assert st.node_tests > 0


@pytest.mark.parametrize("g", [8, 32])
def test_tree_equals_list_on_the_grids(g):
    T, pl, rays, want = MT.grid_case(g)
    t, p, tri, nrm, st = tree(T, pl, rays)
    M.assert_hits_equal((t, p, tri, nrm), want, f"grid {g}")


def test_the_grid_of_8_meets_the_input_conditions():
    """From the restatement, the placements evaluated one at a time (the group's answer is their least t, the lowest index of equals)."""
    T, pl, rays, want = MT.grid_case(8)
    one = [M.placement_hits(T, [pl[k]], rays[:, :3], rays[:, 3:]) for k in range(len(pl))]
    accepted = np.sum([h["found"] for h in one], axis=0)
    hit = float((accepted >= 1).mean())
    assert 0.25 <= hit <= 0.75, hit
    share = float((accepted >= 2).mean())
    print(f"g = 8: {hit:.1%} of the rays hit, {share:.1%} are accepted by two or more placements")
    assert share >= 0.05, share
    with np.errstate(all="ignore"):
        t = np.stack([np.where(h["found"] & ~np.isnan(h["t"]), h["t"], F(np.inf)) for h in one])
    winner = np.where(np.isfinite(t.min(axis=0)), t.argmin(axis=0), -1)
    plain = MT.ordinary(rays)
    assert np.array_equal(winner[plain], want[1][plain])                  # (the host list form agrees with the restatement)
    wins = np.bincount(winner[winner >= 0], minlength=len(pl))
    assert (wins >= 1).all(), wins


def test_the_grid_of_32_meets_the_input_conditions():
    _, pl, rays, want = MT.grid_case(32)
    hit = float((want[1] >= 0).mean())
    assert 0.25 <= hit <= 0.75, hit
    assert len(np.unique(want[1][want[1] >= 0])) >= 512


def test_thirty_two_coincident_placements_answer_the_first():
    T = M.standard_mesh()
    pl = [([0.5, 0.2, 4.0], [1.0, 0.0, 0.0, 0.0])] * 32
    rays = M.standard_rays(placements=pl[:1])
    want, _ = assert_tree_equals_list(T, pl, rays, "32 coincident placements")
    assert (want[1] >= 0).sum() >= 500 and (want[1][want[1] >= 0] == 0).all()
    # ... in whatever order the tree meets them: the same placements listed backwards still answer the lowest index
    t, p, _, _, _ = tree(T, pl[::-1], rays)
    assert (p[p >= 0] == 0).all() and np.array_equal(t.view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("far", [1e4, 1e5])
def test_tree_equals_list_far_from_the_origin(far):
    """Positions of magnitude 1e4 / 1e5, rays from 1e3 away: the f32 rounding of o - position (6e-5 / 4e-3 ... 8e-3) is comparable to the
    mesh's features, so hits near a silhouette exist only through the rounding the bound has to cover."""
    T = M.standard_mesh()
    pl = MT.grid(8, offset=(far, -0.5 * far, 0.25 * far))
    rng = np.random.default_rng(3)
    centres = np.array([p[0] for p in pl], np.float64)
    rays = np.empty((4096, 6), np.float64)
    for k in range(len(rays)):
        c = centres[k % len(centres)]
        o = c + 1e3 * QC.unit3(rng.normal(size=3).astype(F)).astype(np.float64)
        rays[k, :3], rays[k, 3:] = o, (c + rng.normal(scale=0.6, size=3) - o) * rng.uniform(0.5, 2.0) / 1e3
    want, st = assert_tree_equals_list(T, pl, rays.astype(F), f"positions of {far:g}")
    assert 0.2 <= float((want[1] >= 0).mean()) <= 0.9 and st.node_tests > 0


def test_zero_direction_components_through_identity_placements():
    T = M.standard_mesh()
    pl = MT.grid(8, general=False)
    rng = np.random.default_rng(11)
    rays = []
    for k in range(2048):
        c = np.array(pl[k % len(pl)][0], np.float64)
        axis = k % 3
        d = np.zeros(3)
        d[axis] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
        if k % 2:                                                        # one zero component, else two
            d[(axis + 1) % 3] = rng.normal(scale=0.3)
        rays.append(np.concatenate([c - 20.0 * d / np.linalg.norm(d) + rng.uniform(-0.8, 0.8, 3) * (d == 0), d]))
    rays = np.array(rays, F)
    assert ((rays[:, 3:] == 0).sum(axis=1) == 2).sum() == 1024 and ((rays[:, 3:] == 0).sum(axis=1) == 1).sum() == 1024
    want, st = assert_tree_equals_list(T, pl, rays, "zero components")
    assert (want[1] >= 0).sum() >= 500
    assert st.node_tests < len(rays) * len(pl)                           # such rays still prune: no fall back to every placement


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
REFUSED = {
    "NaN origin": [np.nan, 0.0, -5.0, 0.0, 0.0, 1.0],
    "NaN direction": [0.0, 0.0, -5.0, 0.0, np.nan, 1.0],
    "zero direction": [0.0, 0.0, -5.0, 0.0, 0.0, 0.0],
    "|o| beyond the reach": [2.0 ** 39, 0.0, 6.0, -1.0, 0.0, 0.0],
}


@pytest.mark.parametrize("kind", list(REFUSED))
def test_refused_rays_walk_the_placements_as_a_list(kind):
    """A ray the top-level tree refuses meets every placement in list order: the list's bits, no top-level visit.  (NaN rays fail
    tri_ray_ordinary in every frame: no node visit at all, every triangle tested.  The far origin and the zero direction are ordinary in a
    placement's frame -- they visit the mesh's root there, once per placement, and nothing else -- which is what the list order costs.)"""
    T, pl, _, _ = MT.grid_case(8)
    rays = np.array([REFUSED[kind]] * 4, F)
    want, st = assert_tree_equals_list(T, pl, rays, kind)
    if "NaN" in kind:
        assert st.node_tests == 0 and st.quad_tests == len(rays) * len(pl) * T.k
    else:
        assert st.node_tests == len(rays) * len(pl)                      # the mesh's root, per placement: what the list order costs


def test_a_placement_beyond_the_reach_refuses_the_context():
    T, pl, rays, _ = MT.grid_case(8)
    far = pl + [([1e30, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])]
    nodes, order, depth, list_walk = R.mesh_top_dump(T.pods(), far)
    assert list_walk == 1 and len(order) == len(far)
    want, st = assert_tree_equals_list(T, far, rays[:512], "a placement at 1e30")
    plain = MT.ordinary(rays[:512])
    assert st.node_tests >= plain.sum() * len(pl)                        # list order: the mesh's root in every placement within reach
    assert R.mesh_top_dump(T.pods(), pl)[3] == 0


# ---- pruning -----------------------------------------------------------------------------------------------------------------------------------
def test_the_tree_prunes_on_the_grid_of_32():
    T, pl, rays, _ = MT.grid_case(32)
    n = len(pl)
    st = tree(T, pl, rays)[4]
    print(f"g = 32: {st.node_tests / len(rays):.1f} node visits and {st.quad_tests / len(rays):.1f} triangle tests per ray through the tree")
    assert st.node_tests / len(rays) < n / 4
    # the list order's price on the same rays: the context refused (one placement out of reach, far from every ray) walks them as a list
    far = pl + [([1e30, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])]
    st_list = tree(T, far, rays)[4]                                      # the same 4096 rays
    assert st_list.node_tests >= MT.ordinary(rays).sum() * n             # at least one node visit per placement and ordinary ray


def test_the_python_option_surface():
    assert R.OPT_MESH_LIST_MAX == 12
    assert R.MESH_LIST_MAX_DEFAULT == R.lib().rtw_mesh_list_max_default() >= 7      # the Python copy is the library's default
    assert hasattr(R.lib(), "rtw_mesh_top_dump") and hasattr(R.lib(), "rtw_mesh_instance_hits_tree")
