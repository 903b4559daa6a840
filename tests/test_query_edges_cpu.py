"""The inputs of test_gpu_query_edges.py do what those tests need -- shown with the oracle and numpy alone, no GPU: the hit shares of the
maps, the flips at the range edges, the side of its bound every out-of-the-ordinary ray lies on (d.d, |o|_1, the reach product, the triangle
tree's bound and the discriminant recomputed in f32), the spoilers' lanes, and the map with one zero column."""
import numpy as np
import pytest

from tests import query_edges_common as Q
from tests.query_edges_common import F, MAXT, MINT


# ---- A ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["book1", "forty"])
def test_the_maps_exercise_hits_and_misses(oracle, which):
    scene, cam, w, h, time, want = Q.map_reference(oracle, which)
    idx = want[1]
    assert (w * h) % 64 != 0 and (w * h) % 256 != 0               # a ragged last wave
    assert 0.2 <= Q.hit_share(idx) <= 0.8
    if which == "book1":
        assert scene.n_spheres > 48                               # as shipped an RTW_ACCEL_BVH request goes through the tree
        assert len(set(idx[idx >= 0].tolist())) >= 15
        assert np.any(idx == 0)                                   # the ground, which the tree keeps outside
    else:
        assert any(i % 4 == 1 for i in idx[idx >= 0].tolist())    # a moving sphere is an answer
        still = Q.oracle_hits(oracle, scene, Q.R.depth_rays(cam, w, h), 0.0, MINT, MAXT)
        assert np.any(Q.bits(still[0]) != Q.bits(want[0]))        # ... and `time` matters to the map


# ---- B ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["forty", "book1"])
def test_the_range_cases_flip_the_oracles_answer(oracle, which):
    scene, time, rays, cases, (t_near, first) = Q.range_reference(oracle, which)
    assert np.all(first >= 0) and np.all(first < scene.n_spheres)
    assert len(cases) >= (64 if which == "forty" else 20)
    seen = [set() for _ in rays]
    at_maxt = at_mint = 0
    for mint, maxt, want, j in cases:
        seen[j].add(int(want[1][j]))
        at_maxt += int(want[1][j] >= 0 and want[0][j] == F(maxt))
        at_mint += int(want[1][j] >= 0 and want[0][j] == F(mint))
    assert at_maxt >= len(rays) and at_mint >= len(rays)          # hits EXACTLY at maxt (the tree's tie with best == -1) and exactly at mint
    for j in range(len(rays)):
        assert {int(first[j]), -1} <= seen[j]                     # this sphere and a miss
    if which == "forty":
        assert sum(len(s - {-1}) >= 2 for s in seen) >= 3         # ... and another sphere, for several rays
    else:
        assert first[0] == 0                                      # the ground


# ---- C ------------------------------------------------------------------------------------------------------------------------------------

def test_the_field_scene_has_a_real_tree_and_all_four_groups():
    scene = Q.field_scene()
    g = Q.geom_scene()
    assert scene.n_spheres == 63 > 48
    assert (scene.n_quads, scene.n_instances, scene.n_triangles) == (g.n_quads, g.n_instances, g.n_triangles) and scene.n_triangles > 48


def test_every_kind_lies_on_its_side_of_its_bound(oracle):
    scene = Q.field_scene()
    span = Q.scene_span(scene)
    names = set()
    for name, cls, rays, (what, expect) in Q.edge_kinds():
        mint, maxt = Q.RANGES[cls]
        t_bound = max(abs(mint), abs(maxt))
        names.add(name)
        dd, no = Q.dd_of(rays), Q.l1(rays[:, :3])
        if what == "a_plain":
            assert np.all(Q.a_plain(rays) == expect), name
            assert np.all((dd > F(2.0 ** -22)) & (dd < F(2.0 ** 22)))
            assert np.all(Q.q_ordinary(rays, span)) and np.all(Q.tri_ordinary(rays, t_bound))      # nothing else is out of the ordinary
        elif what == "q_ordinary":
            assert np.all(Q.q_ordinary(rays, span) == expect), name
            if name.startswith("dd="):                            # ... and d.d is what decides
                lo, hi = (F(1e-30), F(1e30))
                assert np.all(((dd >= lo) & (dd <= hi)) == expect) and np.all(Q.reach_product(rays, span) <= F(1e18)), name
                assert np.all(no + Q.l1(rays[:, 3:]) < F(2.0 ** 60))
        elif what == "l1o<2^60":
            assert np.all((no < F(2.0 ** 60)) == expect), name
            assert np.all((no + Q.l1(rays[:, 3:])).astype(F) == no)                                # |d| adds nothing at that size
            assert not np.any(Q.q_ordinary(rays, span))           # (the reach product refuses either side: 2 * 2^60 > 1e18)
        elif what == "reach<=1e18":
            assert np.all((Q.reach_product(rays, span) <= F(1e18)) == expect), name
            assert np.all((dd >= F(1e-30)) & (dd <= F(1e30))) and np.all(Q.q_ordinary(rays, span) == expect)
        elif what == "tri_ordinary":
            assert np.all(Q.tri_ordinary(rays, t_bound) == expect), name
            assert np.all(Q.q_ordinary(rays, span))               # the sphere tree takes them either way
            if name != "tri far origin":
                assert np.all(np.abs(rays[:, 3:]).max(axis=1) == (F(2.0 ** 20) if expect else F(Q.above(2.0 ** 20))))
        elif what == "tiny":
            d = np.abs(rays[:, 3:])
            assert np.all((d < F(2.0 ** -126)).sum(axis=1) >= 1) and np.all(d.max(axis=1) >= 1.0)
            if expect:                                            # denormal, most of them so small that 1 / d overflows
                assert np.all(((d > 0) & (d < F(2.0 ** -126))).sum(axis=1) == 1) and np.sum((d > 0) & (d < F(2.0 ** -127))) >= 32
                assert np.any(d == F(2.0 ** -127)) and np.any(np.signbit(rays[:, 3:]) & (d > 0) & (d < F(2.0 ** -126)))
            else:
                assert np.all((d == 0).sum(axis=1) >= 1) and np.any(np.signbit(rays[:, 3:]) & (d == 0)) and np.any(~np.signbit(rays[:, 3:]) & (d == 0))
            assert np.all(Q.q_ordinary(rays, span)) and np.all(Q.tri_ordinary(rays, t_bound)) and np.all(Q.a_plain(rays))
        elif what == "tangent":
            discs = np.array([Q.sphere_disc(r, *s)[2] for r, s in zip(rays, Q.tangent_rays()[1])], F)
            assert len(rays) >= 9 and np.all(discs[:-1] > 0) and np.all(discs[:-1] < F(2.0 ** -60))
            assert discs[-1] == 0 and not np.signbit(discs[-1])   # exactly +0: -0 cannot come out of b * b - a * c
            assert np.all(Q.q_ordinary(rays, span)) and np.all(Q.a_plain(rays))
    assert {"zero direction", "NaN components", "inf components"} <= names
    kinds = {name: rays for name, _, rays, _ in Q.edge_kinds()}
    assert not kinds["zero direction"][:, 3:].any()
    assert sorted(np.isnan(kinds["NaN components"]).sum(axis=1)) == [1, 1, 2, 2, 3, 3]
    inf = np.isinf(kinds["inf components"])
    assert inf[:, :3].any() and inf[:, 3:].any() and (kinds["inf components"] == -np.inf).any()


def test_the_rays_inside_the_bounds_still_hit(oracle):
    """The ordinary-but-extreme rays must produce hits in the oracle: a set of misses would prove nothing about pruning."""
    span = Q.scene_span(Q.field_scene())
    ref = Q.edge_reference(oracle)
    for cls, (mint, maxt, cuts, row, batch, pos, want_row, want_batch) in ref.items():
        assert 0.2 <= Q.hit_share(want_batch[1]) <= 0.9
        tree_walkers = Q.q_ordinary(row, span)
        for name, sl in cuts:
            hits = int(np.sum(want_row[1][sl] >= 0))
            if np.all(tree_walkers[sl]) and name != "tri far origin":
                assert hits >= (sl.stop - sl.start) // 2, (cls, name, hits)
                assert np.sum((want_row[1][sl] >= 0) & (want_row[1][sl] < Q.field_scene().n_spheres)) >= 1, (cls, name)       # spheres among them (the tree's candidates)
        # scattered: the same rays at the recorded positions, each among ordinary wave-mates
        assert np.array_equal(batch[pos].view(np.uint32), row.view(np.uint32)) and len(set(pos.tolist())) == len(row)
        others = np.setdiff1d(np.arange(len(batch)), pos)
        assert len(others) >= 64 and np.all(Q.q_ordinary(batch[others], span)) and np.all(Q.a_plain(batch[others]))
        for w in range(len(batch) // 64):
            lanes = np.arange(64 * w, 64 * w + 64)
            assert np.intersect1d(lanes, others).size > 0         # every wave holds ordinary lanes
    assert set(ref) == set(Q.RANGES)


def test_the_whole_call_fallbacks_change_the_oracles_answer(oracle):
    scene, rays, inside, cases = Q.fallback_reference(oracle)
    assert 0.2 <= Q.hit_share(inside[1]) <= 0.8
    assert any(scene._spheres[k].velocity[0] != 0.0 for k in range(scene.n_spheres))
    for name, (time, mint, maxt, want) in cases.items():
        assert np.any(~Q.same_nan(want[0], inside[0])), name      # each case is a different question
    assert np.isnan(cases["NaN time"][3][0]).any()                # NaN roots pass the reference's range tests


# ---- D ------------------------------------------------------------------------------------------------------------------------------------

def test_the_spoilers_spoil_what_they_are_meant_to(oracle):
    scene = Q.field_scene()
    span = Q.scene_span(scene)
    base, want, kinds = Q.wave_reference(oracle)
    t_bound = max(abs(Q.D_MINT), abs(Q.D_MAXT))
    # the baseline is ordinary in every respect, and balanced
    assert len(base) == 1024 and 0.2 <= Q.hit_share(want[1]) <= 0.8
    assert np.all(Q.q_ordinary(base, span)) and np.all(Q.tri_ordinary(base, t_bound)) and np.all(Q.a_plain(base)) and np.all(Q.unit_plain(base[:, 3:]))
    on_sphere = (want[1] >= 0) & (want[1] < scene.n_spheres)
    assert np.all(np.abs(want[2][on_sphere]).min(axis=1) >= F(2.0 ** -30))       # ... and so are the sphere normals unit() makes
    groups = [np.sum((want[1] >= 0) & (want[1] < scene.n_spheres)), np.sum(want[1] >= scene.n_spheres + scene.n_quads + scene.n_instances)]
    assert min(groups) > 20, groups                               # spheres and triangles are answers
    assert sorted(Q.LANES[:4]) == [0, 31, 32, 63] and len(set(Q.LANES)) >= 8 and all(0 <= v < 64 for v in Q.LANES)
    for name, (launch, pos, want_spoilers) in kinds.items():
        assert [int(p) // 64 for p in pos] == list(range(16)) and [int(p) % 64 for p in pos] == Q.LANES      # one per wave
        mates = np.setdiff1d(np.arange(1024), pos)
        assert np.array_equal(launch[mates].view(np.uint32), base[mates].view(np.uint32))
        sp = launch[pos]
        q, tri, ap = Q.q_ordinary(sp, span), Q.tri_ordinary(sp, t_bound), Q.a_plain(sp)
        if name.startswith("dd outside"):
            assert not ap.any() and q.all() and tri.all()
        elif name.startswith("tangent"):
            rays, sph = Q.tangent_rays()
            lookup = {r.tobytes(): s for r, s in zip(rays, sph)}
            discs = np.array([Q.sphere_disc(r, *lookup[r.tobytes()])[2] for r in sp], F)
            assert np.all((discs > 0) & (discs < F(2.0 ** -60))) and ap.all() and q.all() and tri.all()
        elif name.startswith("zero"):
            assert np.all(sp[:, 3] == 0) and ap.all() and q.all() and tri.all()
            on_sphere = (want_spoilers[1] >= 0) & (want_spoilers[1] < scene.n_spheres)
            assert np.sum(on_sphere & (want_spoilers[2][:, 0] == 0)) >= 4      # sphere normals with an exactly-zero x: unit()'s generic path
        elif "dd < 1e-30" in name:
            assert not q.any() and tri.all() and np.all(Q.dd_of(sp) < F(1e-30))
        elif "far origin" in name:
            assert not q.any() and np.all(Q.reach_product(sp, span) > F(1e18)) and ap.all()
        elif name.startswith("refused by tri"):
            assert q.all() and ap.all() and not tri.any() and np.all(Q.unit_plain(sp[:, 3:]))
        else:
            assert np.all(np.isnan(sp).sum(axis=1) == 1) and not q.any() and not tri.any()
    assert len(kinds) == 7


def test_the_mixed_map_has_exactly_one_zero_column(oracle):
    scene, cam, rays, want = Q.mixed_reference(oracle)
    w, h = Q.MIXED_W, Q.MIXED_H
    zero_x = (rays[:, 3] == 0).reshape(h, w)
    cols = np.flatnonzero(zero_x.any(axis=0))
    assert list(cols) == [w // 2] and zero_x[:, w // 2].all()     # the whole centre column, no other
    for first in range(0, w * h, 64):
        lanes = zero_x.reshape(-1)[first:first + 64]
        assert lanes.any() and not lanes.all()                    # every wave mixes zero and non-zero lanes
    assert (w * h) % 64 != 0
    assert 0.2 <= Q.hit_share(want[1]) <= 0.9
    base = scene.n_spheres + scene.n_quads + scene.n_instances
    centre = want[1].reshape(h, w)[:, w // 2]
    assert np.any(centre >= base)                                 # the zero column meets triangles (any_zero in the triangles' tree)
