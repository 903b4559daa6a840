"""rtw_ctx_scene_hits / rtw_ctx_depth_map (csrc/rtw_query.hip) where test_gpu_scene_hits.py leaves them unpinned: the camera kernel through
the sphere tree, the range edges through the tree, rays on either side of every per-ray fall-back bound, the shim's whole-call fall-backs,
and the independence of a ray's bits from its wave-mates.  Expected values are the frozen oracle's (query_edges_common.py caches them per
session); every comparison is on the bits, a NaN in both counting as equal.  test_query_edges_cpu.py proves that each input set does what
its test here needs."""
import numpy as np
import pytest

import rtw_amd as R
from tests import query_edges_common as Q
from tests.query_edges_common import MAXT, MINT, TIME, assert_same_nan, forced_tree  # noqa: F401  (forced_tree: a fixture)

pytestmark = pytest.mark.gpu

ACCELS = [R.ACCEL_BRUTE, R.ACCEL_BVH]


def check_map(gpu, ref, accel, normals, what):
    """depth_map against the oracle's answer for the map's rays; with `normals`, ids and normals too."""
    scene, cam, w, h, time, want = ref
    want_depth = Q.as_depth(want[0], MAXT, h, w)
    if normals:
        depth, ids, nrm, st = gpu.depth_map(cam, w, h, MINT, MAXT, time=time, accel=accel, ids=True, normals=True)
        assert_same_nan((depth, ids, nrm), (want_depth, want[1], want[2]), what)
    else:
        depth, st = gpu.depth_map(cam, w, h, MINT, MAXT, time=time, accel=accel)
        assert_same_nan((depth,), (want_depth,), what)
    assert st.segments == w * h
    return st


# ---- A. the depth map through the sphere tree ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("accel", ACCELS)
def test_book1_depth_map_through_the_tree_equals_the_oracle(gpu, oracle, accel, normals):
    """Pins scene_hits_kernel<CAM = true, NORMALS = 1 / 0, TREE = true, MOVING = false> -- two of the four CAM x TREE instantiations -- and
    their TREE = false twins to the oracle: the Book-1 scene (485 spheres, the ground kept outside the tree in the n_big list) as a 65 x 33
    map, whose last wave is ragged and whose pixel count is no multiple of the block."""
    ref = Q.map_reference(oracle, "book1")
    gpu.set_scene(ref[0])
    st = check_map(gpu, ref, accel, normals, f"book 1 map, accel {accel}, normals {normals}")
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
    if accel == R.ACCEL_BRUTE:
        assert st.sphere_tests == ref[0].n_spheres * Q.BOOK1_W * Q.BOOK1_H


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("accel", ACCELS)
def test_moving_spheres_depth_map_through_the_tree_equals_the_oracle(forced_tree, oracle, accel, normals):
    """Pins scene_hits_kernel<CAM = true, NORMALS = 1 / 0, TREE = true, MOVING = true> -- the other two CAM x TREE instantiations -- to the
    oracle: forty spheres, ten of them moving, at time 0.37 of [0, 1], the tree forced."""
    gpu = forced_tree
    ref = Q.map_reference(oracle, "forty")
    gpu.set_scene(ref[0], 0.0, 1.0)
    st = check_map(gpu, ref, accel, normals, f"forty spheres map, accel {accel}, normals {normals}")
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)


# ---- B. range edges through the tree -----------------------------------------------------------------------------------------------------

def check_range_edges(gpu, oracle, which):
    scene, time, rays, cases, _ = Q.range_reference(oracle, which)
    for mint, maxt, want, j in cases:
        for accel in ACCELS:
            t, idx, nrm, st = gpu.scene_hits(rays, mint, maxt, time=time, accel=accel, normals=True)
            what = f"{which}: range [{mint!r}, {maxt!r}] about ray {j}, accel {accel}"
            assert_same_nan((t, idx, nrm), want, what)
            assert (st.node_tests > 0) == (accel == R.ACCEL_BVH), what          # without this the request may go through the list again


def test_range_edges_through_the_forced_tree(forced_tree, oracle):
    """Pins the TREE's own tie rule at the edges of the range -- q_sphere<.., LIST = false> takes x == best_t with best == -1, best_t starting at
    maxt, so a root EXACTLY at maxt is a hit -- together with the tau padding of lo_lim / hi_lim (a root exactly at mint or maxt must not be
    pruned), mint == maxt, maxt = +inf, mint > maxt (the first pop is the sentinel) and negative / zero mint: 8 rays into the forty spheres,
    each with its own cases about its first hit and about the root or sphere behind it, all rays under every case."""
    gpu = forced_tree
    gpu.set_scene(Q.forty_scene(), 0.0, 1.0)
    check_range_edges(gpu, oracle, "forty")


def test_range_edges_on_the_ground_sphere_outside_the_tree(gpu, oracle):
    """The same edges for a ray that ends on Book-1's ground -- one of the n_big spheres the tree keeps outside and tests first, by the tree's
    tie rule -- and for one that ends on a small sphere, the scene as shipped."""
    gpu.set_scene(Q.book1_scene())
    check_range_edges(gpu, oracle, "book1")


# ---- C. rays out of the ordinary, either side of every bound ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", list(Q.RANGES))
@pytest.mark.parametrize("accel", ACCELS)
def test_rays_either_side_of_every_bound_equal_the_oracle(forced_tree, oracle, accel, cls):
    """Pins both per-ray fall-backs in a mixed wave -- q_ray_ordinary sends a lane to the sphere list while its mates walk the tree with their
    stacks in LDS, tri_ray_ordinary does the same for the triangles -- and the tree's paddings (rho, tau, v_rcp, v_rsq, the 1e-20 clamp on
    1 / d) for the rays just INSIDE the bounds, which still hit in the oracle: each kind of query_edges_common.edge_kinds alone in a short
    launch, and all kinds of a range class scattered through a batch of ordinary rays."""
    gpu = forced_tree
    scene = Q.field_scene()
    gpu.set_scene(scene)
    mint, maxt, cuts, row, batch, pos, want_row, want_batch = Q.edge_reference(oracle)[cls]
    for name, sl in cuts:
        t, idx, nrm, st = gpu.scene_hits(row[sl], mint, maxt, accel=accel, normals=True)
        print(f"{cls} / {name} alone, accel {accel}: {sl.stop - sl.start} rays, {st.sphere_tests} sphere, {st.node_tests} node, {st.quad_tests} quad + triangle tests")
        assert_same_nan((t, idx, nrm), tuple(w[sl] for w in want_row), f"{cls} / {name} alone, accel {accel}")
    t, idx, nrm, st = gpu.scene_hits(batch, mint, maxt, accel=accel, normals=True)
    for name, sl in cuts:
        p = pos[sl]
        assert_same_nan((t[p], idx[p], nrm[p]), tuple(w[p] for w in want_batch), f"{cls} / {name} scattered, accel {accel}")
    assert_same_nan((t, idx, nrm), want_batch, f"{cls}: the whole batch, accel {accel}")
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)


def test_whole_call_fallbacks_walk_the_list_and_equal_the_oracle(forced_tree, oracle):
    """Pins scene_query's whole-call fall-backs: a `time` outside [t_begin, t_end] when spheres move (the tree's boxes do not cover them there),
    a NaN mint, maxt or time -- the list is walked (node_tests == 0 under RTW_ACCEL_BVH) and the answer is the oracle's."""
    gpu = forced_tree
    scene, rays, inside, cases = Q.fallback_reference(oracle)
    gpu.set_scene(scene, 0.0, 1.0)
    t, idx, nrm, st = gpu.scene_hits(rays, MINT, Q.FALLBACK_MAXT, time=TIME, accel=R.ACCEL_BVH, normals=True)
    assert st.node_tests > 0                                   # inside the range the tree is walked
    assert_same_nan((t, idx, nrm), inside, "inside the time range")
    for name, (time, mint, maxt, want) in cases.items():
        for accel in ACCELS:
            t, idx, nrm, st = gpu.scene_hits(rays, mint, maxt, time=time, accel=accel, normals=True)
            assert st.node_tests == 0 and st.sphere_tests == scene.n_spheres * len(rays), (name, accel)
            assert_same_nan((t, idx, nrm), want, f"{name}, accel {accel}")


# ---- D. a ray's bits do not depend on its wave-mates ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", ACCELS)
def test_ordinary_rays_equal_the_oracle_in_any_order(forced_tree, oracle, accel):
    """The baseline of the spoiled launches: 1024 ordinary rays equal the oracle, and the same rays reversed and shuffled (other wave-mates,
    other lanes) give the permuted answer."""
    gpu = forced_tree
    gpu.set_scene(Q.field_scene())
    base, want, _ = Q.wave_reference(oracle)
    orders = {"as built": np.arange(len(base)), "reversed": np.arange(len(base))[::-1], "shuffled": np.random.default_rng(5).permutation(len(base))}
    for name, order in orders.items():
        t, idx, nrm, st = gpu.scene_hits(base[order], Q.D_MINT, Q.D_MAXT, accel=accel, normals=True)
        assert_same_nan((t, idx, nrm), tuple(w[order] for w in want), f"{name}, accel {accel}")
        assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)


@pytest.mark.parametrize("kind", list(Q.spoiler_rays()))
@pytest.mark.parametrize("accel", ACCELS)
def test_one_spoiler_lane_per_wave_changes_no_other_lane(forced_tree, oracle, accel, kind):
    """Pins each ballot-switched sequence in a MIXED wave: every wave of 64 holds one spoiler at a varying lane (0, 31, 32, 63, ...), and the
    63 ordinary lanes must keep their bits (t, index, normal) -- the oracle's -- while the spoiler answers what the oracle answers.
      dd outside [2^-20, 2^20]   a_plain: sphere_root's div_plain / sqrt_plain against the generic expansion
      tangent, disc < 2^-60      sphere_root's `plain` ballot, at the sphere the spoiler grazes
      zero direction component   any_zero in q_tri_tree, and unit()'s generic path for the normal (half of the spoilers end on a sphere whose
                                 centre has their x: the normal's x is exactly zero); unit() of the DIRECTION is the depth-map test's, below
      refused by q_ray_ordinary  the lane walks the sphere list while its mates walk the tree (dd < 1e-30 also spoils a_plain; a far origin is
                                 also refused by tri_ray_ordinary: no ray is refused by q_ray_ordinary alone)
      refused by tri_ray_ordinary  the lane walks the triangle list while its mates walk the triangles' tree
      NaN                        both fall-backs and every generic sequence at once"""
    gpu = forced_tree
    gpu.set_scene(Q.field_scene())
    base, want, kinds = Q.wave_reference(oracle)
    launch, pos, want_spoilers = kinds[kind]
    t, idx, nrm, st = gpu.scene_hits(launch, Q.D_MINT, Q.D_MAXT, accel=accel, normals=True)
    mates = np.setdiff1d(np.arange(len(base)), pos)
    assert len(mates) == len(base) - 16
    assert_same_nan((t[mates], idx[mates], nrm[mates]), tuple(w[mates] for w in want), f"{kind}: the 63 ordinary lanes, accel {accel}")
    assert_same_nan((t[pos], idx[pos], nrm[pos]), want_spoilers, f"{kind}: the spoilers, accel {accel}")
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)


@pytest.mark.parametrize("accel", ACCELS)
def test_depth_map_with_one_zero_column_equals_the_oracle(gpu, oracle, accel):
    """The same property in the depth map's own form: an axis-aligned camera whose centre column has d.x == 0 exactly, so every wave of the map
    mixes zero-component lanes (unit()'s generic path, any_zero in q_tri_tree) with ordinary ones."""
    scene, cam, rays, want = Q.mixed_reference(oracle)
    gpu.set_scene(scene)
    w, h = Q.MIXED_W, Q.MIXED_H
    depth, ids, nrm, st = gpu.depth_map(cam, w, h, MINT, MAXT, accel=accel, ids=True, normals=True)
    assert_same_nan((depth, ids, nrm), (Q.as_depth(want[0], MAXT, h, w), want[1], want[2]), f"mixed map, accel {accel}")
    t, idx, n2, _ = gpu.scene_hits(rays, MINT, MAXT, accel=accel, normals=True)
    assert_same_nan((t, idx, n2), want, f"mixed map's rays, accel {accel}")
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)       # the triangles' tree (three spheres walk the list)
