"""rtw_ctx_scene_hits / rtw_ctx_depth_map on the GPU against the CPU oracle, bit for bit.

Expected values: for every ray a depth-1 rtw_oracle_trace_ray under an RNG-free integrator (record 0: hit, top-level index, t, normal);
where the scene has triangles, combined with rtw_oracle_triangle_hits by the strict-less rule (the triangles come last and replace the
result so far only when strictly closer), the triangle's normal from rtw_oracle_triangle_derived.  Every comparison is on the bits."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import lights_common as LC

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_NO_SCENE = -1, -6
MINT, MAXT = 0.001, 1000.0
TIME = 0.37


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(got, want, what):
    """(t, idx[, normals]) against (t, idx[, normals]), on the bits."""
    for name, g, w in zip(("t", "idx", "normal"), got, want):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w) if name == "idx" else np.flatnonzero(bits(g) != bits(w))
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def oracle_params(mint, maxt):
    p = R.RtwParams()
    p.width, p.height, p.samples, p.depth = 1, 1, 1, 1
    p.gamma, p.mint, p.maxt = 1.0, mint, maxt
    p.integrator, p.sampler, p.accel = R.INTEGRATOR_NORMAL, R.SAMPLER_NO_RAND, R.ACCEL_BRUTE
    p.seed = 1
    p.row_block, p.part_index, p.part_count = 8, 0, 1
    return p


def oracle_hits(O, scene, rays, time, mint=MINT, maxt=MAXT):
    """(t [n] f32, +inf on a miss; idx [n] i32, -1 on a miss; normal [n][3] f32, 0 on a miss) of the oracle."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    n = len(rays)
    t = np.full(n, np.inf, F)
    idx = np.full(n, -1, np.int32)
    nrm = np.zeros((n, 3), F)
    p = oracle_params(mint, maxt)
    for k in range(n):
        b, _ = O.trace_ray(rays[k, :3], rays[k, 3:], time, scene, p, cap=2)
        assert len(b) == 1
        if b[0].hit:
            t[k], idx[k], nrm[k] = b[0].t, b[0].sphere, list(b[0].normal)
    if scene.n_triangles:
        tris = [scene.triangles[i] for i in range(scene.n_triangles)]
        tt, ti = O.triangle_hits(tris, rays, mint, maxt)
        der = O.triangle_derived(tris)
        base = scene.n_spheres + scene.n_quads + scene.n_instances
        take = (ti >= 0) & ((idx < 0) | (t > tt))
        t[take] = tt[take]
        idx[take] = base + ti[take]
        nrm[take] = der[ti[take], :3]
    return t, idx, nrm


def assert_balanced(idx):
    hit = float(np.mean(np.asarray(idx).reshape(-1) >= 0))
    assert 0.2 <= hit <= 0.8, f"the oracle reports {hit:.2%} hits: the rays do not exercise both outcomes"


# ---- scenes and rays (built once per session, never modified) -----------------------------------------------------------------

def forty_spheres(duplicate=False):
    """40 spheres in a box, some overlapping, 10 of them moving; sphere 20 sits at the origin, where half of the rays start (inside it: their
    near root lies behind mint).  duplicate: sphere 17 is sphere 3 again."""
    rng = np.random.default_rng(7)
    sp = []
    for k in range(40):
        c = rng.uniform((-4.0, -2.0, -4.0), (4.0, 2.0, 4.0))
        r = float(rng.uniform(0.3, 0.9))
        if k == 20:
            c, r = np.zeros(3), 0.6
        if k % 4 == 1:
            sp.append(R.Sphere.new_moving(tuple(c), r, (0.5, 0.5, 0.5), R.SCATTER_M, tuple(rng.uniform(-0.8, 0.8, 3))))
        else:
            sp.append(R.Sphere.new(tuple(c), r, (0.5, 0.5, 0.5), R.SCATTER_M))
    if duplicate:
        sp[17] = R.Sphere(R.RtwSphere.from_buffer_copy(sp[3].pod))
    return R.Scene(sp)


def centre_of(scene, k, time=0.0):
    s = scene._spheres[k]
    return np.array(list(s.center), np.float64) + np.array(list(s.velocity), np.float64) * time


def forty_rays(scene, n=2048, seed=11):
    """Half from inside sphere 20, half from a point outside the field; directions of length 0.5 .. 2: a third aimed at sphere centres,
    the rest random."""
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), F)
    for k in range(n):
        inside = k % 2 == 0
        o = rng.uniform(-0.25, 0.25, 3) if inside else np.array([0.0, 3.0, 9.0]) + rng.uniform(-0.3, 0.3, 3)
        if k % 3 == 0 and not inside:
            d = centre_of(scene, int(rng.integers(0, 40)), TIME) + rng.normal(0, 0.3, 3) - o
        else:
            d = rng.normal(0, 1, 3)
        d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        rays[k, :3], rays[k, 3:] = o, d
    return rays


FORTY_MAXT = 7.0      # the far root of sphere 20 is 0.175 .. 1.7 away in t; the spheres beyond 7 |d| are misses


@pytest.fixture(scope="module")
def forty(oracle):
    scene = forty_spheres()
    rays = forty_rays(scene)
    want = oracle_hits(oracle, scene, rays, TIME, MINT, FORTY_MAXT)
    return scene, rays, want


COPLANAR = ((-2.9, 0.4, -6.0), (1.2, 0.0, 0.0), (0.0, 1.0, 0.0))      # origin, u, v of the triangle that lies in quad 0


def geom_scene(medium=False):
    """A few spheres, two top-level quads, a rotated and translated box, an instance of two spheres, an icosphere of triangles and one
    triangle coplanar with quad 0 and inside it.  medium: a constant-density box in front of everything, FIRST in the instance list."""
    sp = [R.Sphere.new((0.0, -0.4, -3.0), 0.5, (0.5, 0.5, 0.5), R.SCATTER_M),
          R.Sphere.new((0.5, -0.2, -3.4), 0.6, (0.5, 0.5, 0.5), R.METALLIC_M),
          R.Sphere.new((-2.4, 1.6, -4.0), 0.4, (0.5, 0.5, 0.5), R.GLASS_M)]
    quads = [R.Quad.new((-3.0, -3.0, -6.0), (6.0, 0.0, 0.0), (0.0, 4.5, 0.0)),
             R.Quad.new((-3.0, -1.5, -6.0), (6.0, 0.0, 0.0), (0.0, 0.0, 5.0))]
    box = R.Instance.new_box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (0.7, 0.7, 0.7), R.SCATTER_M)
    box.rotate((0.0, 0.5, 0.0))
    box.translate((1.6, 0.0, -3.0))
    pair = R.Instance.new_sphere([R.Sphere.new((0.0, 0.0, 0.0), 0.5, (0.5, 0.5, 0.5), R.SCATTER_M),
                                  R.Sphere.new((0.6, 0.3, 0.0), 0.3, (0.5, 0.5, 0.5), R.SCATTER_M)])
    pair.rotate((0.2, 0.0, 0.1))
    pair.translate((-1.6, -0.6, -3.0))
    inst = [box, pair]
    if medium:
        fog = R.Instance.new_box((-2.5, -1.4, -0.5), (2.5, 2.5, 0.5), (1.0, 1.0, 1.0), R.SCATTER_M)
        fog.translate((0.0, 0.0, -1.5))
        fog.const_density(0.7)
        inst = [fog] + inst
    vtx, faces = R.mesh_icosphere(1, centre=(0.0, 1.3, -3.5), radius=0.7)
    vtx = np.asarray(vtx, F)
    faces = np.asarray(faces, np.int64)
    o = vtx[faces[:, 0]]
    u, v = vtx[faces[:, 1]] - o, vtx[faces[:, 2]] - o
    o = np.concatenate([o, [COPLANAR[0]]]).astype(F)                  # coplanar with quad 0 (z = -6), inside it
    u = np.concatenate([u, [COPLANAR[1]]]).astype(F)
    v = np.concatenate([v, [COPLANAR[2]]]).astype(F)
    return R.Scene(sp, quads=quads, instances=inst, triangles=R.TriangleArray(o, u, v))


def geom_rays(n=2048, seed=5):
    """From around the camera point (0, 0.3, 1.5): a cone that covers the objects and the sky around the wall, non-unit directions; one in
    eight aims at the coplanar triangle."""
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), F)
    for k in range(n):
        o = np.array([0.0, 0.3, 1.5]) + rng.uniform(-0.2, 0.2, 3)
        if k % 8 == 0:
            a, b = rng.uniform(0.02, 0.98, 2)
            if a + b > 1.0:
                a, b = 1.0 - a, 1.0 - b
            target = np.array(COPLANAR[0]) + a * np.array(COPLANAR[1]) + b * np.array(COPLANAR[2])
        else:
            target = np.array([rng.uniform(-5.5, 5.5), rng.uniform(-3.5, 5.5), -6.0])
        d = target - o
        d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        rays[k, :3], rays[k, 3:] = o, d
    return rays


@pytest.fixture(scope="module")
def geom(oracle):
    scene = geom_scene()
    rays = geom_rays()
    want = oracle_hits(oracle, scene, rays, 0.0)
    return scene, rays, want


@pytest.fixture()
def forced_tree(gpu):
    """RTW_OPT_LIST_WALK_MAX = 0 for the test (scenes of 48 spheres or fewer then go through the tree), the default again afterwards."""
    gpu.set_option(R.OPT_LIST_WALK_MAX, 0)
    yield gpu
    gpu.set_option(R.OPT_LIST_WALK_MAX, 48)


# ---- 1. spheres, list walk -------------------------------------------------------------------------------------------------------

def test_spheres_list_walk_equals_the_oracle(gpu, forty):
    scene, rays, want = forty
    assert_balanced(want[1])
    far = [k for k in range(0, len(rays), 2) if want[1][k] == 20]
    assert len(far) > 100                                   # rays from inside sphere 20 that end on its far side
    assert len({int(i) for i in want[1] if i >= 0}) > 15    # many different spheres are the answer, moving ones among them
    assert any(int(i) % 4 == 1 for i in want[1] if i >= 0)
    gpu.set_scene(scene, 0.0, 1.0)
    t, idx, nrm, st = gpu.scene_hits(rays, MINT, FORTY_MAXT, time=TIME, accel=R.ACCEL_BRUTE, normals=True)
    assert_same((t, idx, nrm), want, "40 spheres, list")
    assert st.segments == len(rays) and st.sphere_tests == 40 * len(rays) and st.node_tests == 0 and st.quad_tests == 0
    assert st.kernel_ms > 0.0
    # the moving spheres are where `time` puts them: at time 0 the answer differs
    t0, idx0, _ = gpu.scene_hits(rays, MINT, FORTY_MAXT, time=0.0, accel=R.ACCEL_BRUTE)
    assert np.any(bits(t0) != bits(t))


# ---- 2. tree equals list ---------------------------------------------------------------------------------------------------------

def book1_rays(scene, n=4096, seed=3):
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), F)
    o = np.array([13.0, 2.0, 3.0])
    for k in range(n):
        if k % 2 == 0:
            d = centre_of(scene, int(rng.integers(1, scene.n_spheres))) + rng.normal(0, 0.25, 3) - o
        else:
            d = rng.normal(0, 1, 3)
        d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        rays[k, :3], rays[k, 3:] = o + rng.uniform(-0.1, 0.1, 3), d
    return rays


def test_tree_equals_list_on_the_book1_scene(gpu, oracle):
    scene = R.Scene.generate(R.SCENE_C2)
    rays = book1_rays(scene)
    want = oracle_hits(oracle, scene, rays, 0.0)
    assert_balanced(want[1])
    gpu.set_scene(scene)
    lt, li, ln, lst = gpu.scene_hits(rays, MINT, MAXT, accel=R.ACCEL_BRUTE, normals=True)
    bt, bi, bn, bst = gpu.scene_hits(rays, MINT, MAXT, accel=R.ACCEL_BVH, normals=True)
    assert_same((lt, li, ln), want, "book 1, list")
    assert_same((bt, bi, bn), (lt, li, ln), "book 1, tree against list")
    assert lst.node_tests == 0 and bst.node_tests > 0
    assert bst.sphere_tests < lst.sphere_tests == scene.n_spheres * len(rays)
    assert np.any(li == 0)                                  # the ground, which the tree keeps outside, is the answer for some rays


def forty_rays_4096(scene, seed=29):
    """4096 rays into the 40-sphere field: half aimed at sphere centres (where they are at TIME) plus jitter, half random; every fourth
    starts inside sphere 20, the others outside the field; directions of length 0.5 .. 2."""
    rng = np.random.default_rng(seed)
    rays = np.empty((4096, 6), F)
    for k in range(len(rays)):
        o = rng.uniform(-0.25, 0.25, 3) if k % 4 == 1 else np.array([0.0, 3.0, 9.0]) + rng.uniform(-0.3, 0.3, 3)
        if k % 2 == 0:
            d = centre_of(scene, int(rng.integers(0, 40)), TIME) + rng.normal(0, 0.3, 3) - o
        else:
            d = rng.normal(0, 1, 3)
        d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        rays[k, :3], rays[k, 3:] = o, d
    return rays


def test_tree_equals_list_on_forty_spheres_when_forced(forced_tree, forty, oracle):
    gpu = forced_tree
    scene = forty[0]
    rays = forty_rays_4096(scene)
    want = oracle_hits(oracle, scene, rays, TIME, MINT, 12.0)
    assert_balanced(want[1])
    gpu.set_scene(scene, 0.0, 1.0)
    lt, li, ln, lst = gpu.scene_hits(rays, MINT, 12.0, time=TIME, accel=R.ACCEL_BRUTE, normals=True)
    bt, bi, bn, bst = gpu.scene_hits(rays, MINT, 12.0, time=TIME, accel=R.ACCEL_BVH, normals=True)
    assert lst.node_tests == 0 and bst.node_tests > 0
    assert_same((lt, li, ln), want, "40 spheres, 4096 rays, list")
    assert_same((bt, bi, bn), (lt, li, ln), "40 spheres, 4096 rays, forced tree against list")
    # ... and the rays of case 1
    scene, rays, want = forty
    bt, bi, bn, bst = gpu.scene_hits(rays, MINT, FORTY_MAXT, time=TIME, accel=R.ACCEL_BVH, normals=True)
    assert bst.node_tests > 0
    assert_same((bt, bi, bn), want, "40 spheres, forced tree")


def test_as_shipped_a_small_scene_walks_the_list_under_bvh(gpu, forty):
    scene, rays, want = forty
    gpu.set_scene(scene, 0.0, 1.0)
    bt, bi, bst = gpu.scene_hits(rays, MINT, FORTY_MAXT, time=TIME, accel=R.ACCEL_BVH)
    assert bst.node_tests == 0
    assert_same((bt, bi), want[:2], "40 spheres, BVH request as shipped")


def test_the_lower_index_wins_a_tie_under_both_accels(forced_tree, oracle):
    gpu = forced_tree
    scene = forty_spheres(duplicate=True)
    rng = np.random.default_rng(23)
    n = 4096
    rays = np.empty((n, 6), F)
    o = np.array([0.0, 3.0, 9.0])
    for k in range(n):
        if k % 2 == 0:
            d = centre_of(scene, 3) + rng.normal(0, 0.5, 3) - o
        else:
            d = rng.normal(0, 1, 3)
        d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        rays[k, :3], rays[k, 3:] = o + rng.uniform(-0.3, 0.3, 3), d
    want = oracle_hits(oracle, scene, rays, 0.0, MINT, 30.0)
    assert_balanced(want[1])
    assert np.sum(want[1] == 3) > 200 and not np.any(want[1] == 17)
    gpu.set_scene(scene, 0.0, 1.0)
    for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
        t, idx, nrm, st = gpu.scene_hits(rays, MINT, 30.0, accel=accel, normals=True)
        assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)
        assert_same((t, idx, nrm), want, f"duplicate sphere, accel {accel}")


# ---- 3. all four groups ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_all_four_groups_equal_the_combined_oracle(gpu, geom, accel):
    scene, rays, want = geom
    assert_balanced(want[1])
    ns, nq, ni = scene.n_spheres, scene.n_quads, scene.n_instances
    idx = want[1]
    groups = [np.sum((idx >= 0) & (idx < ns)), np.sum((idx >= ns) & (idx < ns + nq)), np.sum((idx >= ns + nq) & (idx < ns + nq + ni)),
              np.sum(idx >= ns + nq + ni)]
    assert min(groups) > 20, groups                         # every group is the answer for some rays
    assert np.sum(idx == ns + nq) > 5 and np.sum(idx == ns + nq + 1) > 5      # both instances
    # the coplanar triangle (the last one) never wins against quad 0, although rays go through it
    last = ns + nq + ni + scene.n_triangles - 1
    aimed = np.arange(0, len(rays), 8)
    assert not np.any(idx == last) and np.sum(idx[aimed] == ns) > 100
    gpu.set_scene(scene)
    t, gi, nrm, st = gpu.scene_hits(rays, MINT, MAXT, accel=accel, normals=True)
    assert_same((t, gi, nrm), want, f"four groups, accel {accel}")
    assert st.quad_tests > 0 and st.sphere_tests >= 3 * len(rays)
    assert (st.node_tests > 0) == (accel == R.ACCEL_BVH)     # the triangles' tree (three spheres walk the list)
    # without normals: the same t and indices
    t2, gi2, _ = gpu.scene_hits(rays, MINT, MAXT, accel=accel)
    assert_same((t2, gi2), (t, gi), "four groups, no normals")


def zero_component_rays(n=1024, seed=17):
    """Rays with one or two direction components EXACTLY zero (the centre column of a depth map of an axis-aligned camera has them): a slab
    test divides by them."""
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), F)
    for k in range(n):
        o = np.array([rng.uniform(-3.5, 3.5), rng.uniform(-2.0, 4.5), 1.5])
        s = rng.uniform(0.5, 2.0)
        d = [(0.0, 0.0, -s), (0.0, rng.uniform(-0.3, 0.3), -s), (rng.uniform(-0.3, 0.3), 0.0, -s), (0.0, -s, -0.0)][k % 4]
        if k % 4 == 3:
            o = np.array([rng.uniform(-1.0, 1.0), 4.0, rng.uniform(-4.5, -2.5)])         # straight down onto the icosphere and the floor
        rays[k, :3], rays[k, 3:] = o, d
    return rays


@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_rays_with_zero_direction_components(gpu, oracle, geom, accel):
    scene = geom[0]
    rays = zero_component_rays()
    assert np.all(np.sum(rays[:, 3:] == 0.0, axis=1) >= 1)
    want = oracle_hits(oracle, scene, rays, 0.0)
    assert_balanced(want[1])
    base = scene.n_spheres + scene.n_quads + scene.n_instances
    assert np.sum(want[1] >= base) > 20                      # triangles are the answer for some of them
    gpu.set_scene(scene)
    t, idx, nrm, st = gpu.scene_hits(rays, MINT, MAXT, accel=accel, normals=True)
    assert_same((t, idx, nrm), want, f"zero components, accel {accel}")
    if accel == R.ACCEL_BVH:                                 # the tree still prunes for such rays: far fewer tests than the list walk's
        assert 0 < st.node_tests and st.quad_tests < (scene.n_quads + 12 + scene.n_triangles // 2) * len(rays)


# ---- 4. media are skipped ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_a_constant_density_instance_is_skipped(gpu, geom, accel):
    scene_b, rays, want = geom
    scene_a = geom_scene(medium=True)
    assert scene_a.n_instances == scene_b.n_instances + 1
    gpu.set_scene(scene_a)
    ta, ia, na, _ = gpu.scene_hits(rays, MINT, MAXT, accel=accel, normals=True)
    slot = scene_a.n_spheres + scene_a.n_quads              # the medium is instance 0
    assert not np.any(ia == slot)
    mapped = np.where(ia > slot, ia - 1, ia)
    assert_same((ta, mapped, na), want, f"medium skipped, accel {accel}")
    assert np.any(ia > slot)


# ---- 5. range edges ----------------------------------------------------------------------------------------------------------------

def test_range_edges_follow_the_oracle(gpu, oracle):
    """The range edges through the LIST walk: with one sphere both accel values walk the list (node_tests == 0).  The same edges through the
    tree, its tie rule at x == maxt included, are test_gpu_query_edges.py's (test_range_edges_through_the_forced_tree)."""
    scene = R.Scene([R.Sphere.new((0.0, 0.0, -5.0), 1.0, (0.5, 0.5, 0.5), R.SCATTER_M)],
                    quads=[R.Quad.new((2.0, -1.0, -7.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))])
    rays = np.array([[0, 0, 0, 0, 0, -1.25],            # the sphere: roots 3.2 and 4.8
                     [0, 0, 0, 3.0, 0, -7.0],           # the quad at t = 1
                     [0, 0, 0, 0, 1.0, 0]], F)          # nothing
    gpu.set_scene(scene)
    base = oracle_hits(oracle, scene, rays, 0.0, MINT, MAXT)
    assert list(base[1]) == [0, 1, -1]
    t_near, t_quad = base[0][0], base[0][1]
    t_far = oracle_hits(oracle, scene, rays[:1], 0.0, float(np.nextafter(t_near, F(np.inf))), MAXT)[0][0]
    assert t_far > t_near
    cases = [(MINT, MAXT),
             (MINT, float(np.nextafter(t_near, F(0)))), (MINT, float(t_near)),                   # maxt just below / exactly at the sphere's hit
             (MINT, float(np.nextafter(t_quad, F(0)))), (MINT, float(t_quad)),                   # ... the quad's
             (float(np.nextafter(t_near, F(np.inf))), MAXT),                                     # mint just above the near root: the far root
             (float(t_near), MAXT),                                                              # mint exactly at it: the near root
             (float(np.nextafter(t_near, F(np.inf))), float(np.nextafter(t_far, F(0)))),         # ... and the far root out of range too
             (float(t_near), float(t_near)), (float(t_quad), float(t_quad)),                     # mint == maxt at a hit
             (2.0, 2.0)]                                                                         # mint == maxt where nothing is
    seen = set()
    for mint, maxt in cases:
        want = oracle_hits(oracle, scene, rays, 0.0, mint, maxt)
        seen.add(tuple(int(i) for i in want[1]))
        for accel in (R.ACCEL_BRUTE, R.ACCEL_BVH):
            t, idx, nrm, st = gpu.scene_hits(rays, mint, maxt, accel=accel, normals=True)
            assert_same((t, idx, nrm), want, f"range [{mint!r}, {maxt!r}], accel {accel}")
            assert st.node_tests == 0
    assert {(0, 1, -1), (-1, 1, -1), (0, -1, -1), (-1, -1, -1)} <= seen          # the edges do flip hits into misses
    far = oracle_hits(oracle, scene, rays, 0.0, cases[5][0], MAXT)
    assert far[1][0] == 0 and far[0][0] == t_far


# ---- 6. tails and bounds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 257, 1000])
def test_tails_write_nothing_outside_their_arrays(gpu, forty, n_rays):
    """Device buffers with 64 guard elements on either side, filled with a canary: the kernel writes them directly."""
    import torch
    scene, rays, want = forty
    gpu.set_scene(scene, 0.0, 1.0)
    G = 64
    dev = torch.device("cuda:0")
    d_rays = torch.from_numpy(rays[:n_rays].copy()).to(dev)
    d_t = torch.full((n_rays + 2 * G,), -7.5, dtype=torch.float32, device=dev)
    d_i = torch.full((n_rays + 2 * G,), -77, dtype=torch.int32, device=dev)
    d_n = torch.full((3 * n_rays + 2 * G,), -7.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    st = R.RtwStats()
    rc = R.lib().rtw_ctx_scene_hits(gpu._h, d_rays.data_ptr(), n_rays, TIME, MINT, FORTY_MAXT, R.ACCEL_BRUTE, d_t.data_ptr() + 4 * G,
                                    d_i.data_ptr() + 4 * G, d_n.data_ptr() + 4 * G, C.byref(st))
    assert rc == R.RTW_OK
    t, i, n = d_t.cpu().numpy(), d_i.cpu().numpy(), d_n.cpu().numpy()
    for a, canary in ((t, F(-7.5)), (i, -77), (n, F(-7.5))):
        assert np.all(a[:G] == canary) and np.all(a[-G:] == canary)
    assert_same((t[G:-G], i[G:-G], n[G:-G].reshape(-1, 3)), tuple(w[:n_rays] for w in want), f"{n_rays} rays")
    assert st.segments == n_rays and st.sphere_tests == 40 * n_rays
    # and through host memory (staged), without normals
    ht, hi, _ = gpu.scene_hits(rays[:n_rays], MINT, FORTY_MAXT, time=TIME, accel=R.ACCEL_BRUTE)
    assert_same((ht, hi), tuple(w[:n_rays] for w in want[:2]), f"{n_rays} rays, host buffers")


# ---- 7. depth map -------------------------------------------------------------------------------------------------------------------

def depth_camera(which, width, height):
    if which == "light":
        _, g = LC.golden()
        return LC.camera(g, width, height)
    return R.camera2_new(width / height, (0.0, 0.3, 1.5), (0.0, 1.0, 0.0), (0.0, -0.1, -1.0), 75.0, 0.0)


@pytest.fixture(scope="module")
def depth_reference(oracle, geom):
    """Per scene: (scene, camera, rays, the oracle's answer) of the 33 x 17 map."""
    out = {}
    for which in ("light", "geom"):
        scene = LC.golden()[0].scene if which == "light" else geom[0]
        cam = depth_camera(which, 33, 17)
        rays = R.depth_rays(cam, 33, 17)
        out[which] = (scene, cam, rays, oracle_hits(oracle, scene, rays, 0.0))
    return out


@pytest.mark.parametrize("which", ["light", "geom"])
@pytest.mark.parametrize("accel", [R.ACCEL_BRUTE, R.ACCEL_BVH])
def test_depth_map_equals_scene_hits_of_depth_rays_and_the_oracle(gpu, depth_reference, which, accel):
    scene, cam, rays, want = depth_reference[which]
    W, H = 33, 17
    if which == "geom":
        assert_balanced(want[1])
    else:
        assert len({int(i) for i in want[1]}) >= 4           # the walls, floor and light of the box: several quads are the answer
    gpu.set_scene(scene)
    t, idx, nrm, _ = gpu.scene_hits(rays, MINT, MAXT, accel=accel, normals=True)
    assert_same((t, idx, nrm), want, f"{which}: scene_hits of depth_rays")
    miss = F(MAXT) * F(1.6)
    want_depth = np.where(np.isinf(t), miss, t).astype(F).reshape(H, W)
    depth, ids, normals, st = gpu.depth_map(cam, W, H, MINT, MAXT, accel=accel, ids=True, normals=True)
    assert depth.shape == (H, W) and ids.shape == (H, W) and normals.shape == (H, W, 3)
    assert np.array_equal(bits(depth), bits(want_depth))
    assert np.array_equal(ids, idx.reshape(H, W)) and np.array_equal(bits(normals), bits(nrm.reshape(H, W, 3)))
    assert st.segments == W * H and st.kernel_ms > 0.0
    # each output on its own, and none
    d0, st0 = gpu.depth_map(cam, W, H, MINT, MAXT, accel=accel)
    d1, i1, _ = gpu.depth_map(cam, W, H, MINT, MAXT, accel=accel, ids=True)
    d2, n2, _ = gpu.depth_map(cam, W, H, MINT, MAXT, accel=accel, normals=True)
    for d in (d0, d1, d2):
        assert np.array_equal(bits(d), bits(want_depth))
    assert np.array_equal(i1, ids) and np.array_equal(bits(n2), bits(normals))
    assert np.any(depth == miss) == bool(np.any(want[1] < 0))


@pytest.mark.parametrize("width,height", [(1, 1), (64, 1), (1, 5), (65, 3)])
def test_depth_map_of_small_and_narrow_images(gpu, geom, width, height):
    scene = geom[0]
    cam = depth_camera("geom", width, height)
    gpu.set_scene(scene)
    rays = R.depth_rays(cam, width, height)
    t, idx, nrm, _ = gpu.scene_hits(rays, MINT, MAXT, normals=True)
    depth, ids, normals, st = gpu.depth_map(cam, width, height, MINT, MAXT, ids=True, normals=True)
    want_depth = np.where(np.isinf(t), F(MAXT) * F(1.6), t).astype(F).reshape(height, width)
    assert np.array_equal(bits(depth), bits(want_depth)) and np.array_equal(ids, idx.reshape(height, width))
    assert np.array_equal(bits(normals), bits(nrm.reshape(height, width, 3)))
    assert st.segments == width * height


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------

def test_errors(gpu, forty):
    L = R.lib()
    scene, rays, _ = forty
    cam = depth_camera("geom", 4, 4)
    t = np.zeros(4, F)
    idx = np.zeros(4, np.int32)
    r4 = np.ascontiguousarray(rays[:4])
    with R.Renderer(0) as fresh:
        assert L.rtw_ctx_scene_hits(fresh._h, r4.ctypes.data, 4, 0.0, MINT, MAXT, R.ACCEL_BVH, t.ctypes.data, idx.ctypes.data, None,
                                    None) == E_NO_SCENE
        d = np.zeros(16, F)
        assert L.rtw_ctx_depth_map(fresh._h, C.byref(cam), 4, 4, 0.0, MINT, MAXT, R.ACCEL_BVH, d.ctypes.data, None, None, None) == E_NO_SCENE
        with pytest.raises(R.RtwError):
            fresh.scene_hits(r4, MINT, MAXT)
    gpu.set_scene(scene, 0.0, 1.0)
    args = (0.0, MINT, MAXT)
    assert L.rtw_ctx_scene_hits(gpu._h, r4.ctypes.data, 0, *args, R.ACCEL_BVH, t.ctypes.data, idx.ctypes.data, None, None) == E_INVALID
    assert L.rtw_ctx_scene_hits(gpu._h, r4.ctypes.data, 4, *args, 2, t.ctypes.data, idx.ctypes.data, None, None) == E_INVALID
    assert L.rtw_ctx_scene_hits(gpu._h, None, 4, *args, R.ACCEL_BVH, t.ctypes.data, idx.ctypes.data, None, None) == E_INVALID
    assert L.rtw_ctx_scene_hits(gpu._h, r4.ctypes.data, 4, *args, R.ACCEL_BVH, None, idx.ctypes.data, None, None) == E_INVALID
    assert L.rtw_ctx_scene_hits(gpu._h, r4.ctypes.data, 4, *args, R.ACCEL_BVH, t.ctypes.data, None, None, None) == E_INVALID
    d = np.zeros(16, F)
    assert L.rtw_ctx_depth_map(gpu._h, C.byref(cam), 0, 4, *args, R.ACCEL_BVH, d.ctypes.data, None, None, None) == E_INVALID
    assert L.rtw_ctx_depth_map(gpu._h, C.byref(cam), 4, 0, *args, R.ACCEL_BVH, d.ctypes.data, None, None, None) == E_INVALID
    assert L.rtw_ctx_depth_map(gpu._h, C.byref(cam), 4, 4, *args, 2, d.ctypes.data, None, None, None) == E_INVALID
    assert L.rtw_ctx_depth_map(gpu._h, None, 4, 4, *args, R.ACCEL_BVH, d.ctypes.data, None, None, None) == E_INVALID
    assert L.rtw_ctx_depth_map(gpu._h, C.byref(cam), 4, 4, *args, R.ACCEL_BVH, None, None, None, None) == E_INVALID
    assert not t.any() and not idx.any() and not d.any()
    assert L.rtw_ctx_scene_hits(gpu._h, r4.ctypes.data, 4, *args, R.ACCEL_BVH, t.ctypes.data, idx.ctypes.data, None, None) == R.RTW_OK
