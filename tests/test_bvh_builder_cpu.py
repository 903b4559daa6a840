"""The sphere-BVH builder (rtw_host.cpp: full-sweep SAH, subtree reinsertion, a depth cap from the LDS budget), on the host alone.

Every scene below is built through rtw_bvh_dump and checked from the outside: the leaves partition the tree spheres, every box
stored for a child holds the time-expanded boxes of the spheres below it, depth + ceil(log2(count)) <= RTW_BVH_STACK at every node,
and no leaf lies deeper than the cap -- which is restated here from the LDS budget, not read back from the builder."""
import ctypes as C
import math

import numpy as np
import pytest

import rtw_amd as R

STACK, LDS_NODES_MAX, LDS_GEOM_MAX = 24, 512, 640
NODE = np.dtype([("lo0", "<f4", 3), ("hi0", "<f4", 3), ("lo1", "<f4", 3), ("hi1", "<f4", 3), ("c0", "<i4"), ("c1", "<i4"), ("pad", "<u4", 2)])
EMPTY = -2 ** 31


def dump(scene, t0=0.0, t1=0.0):
    n = scene.pod.n_spheres
    nodes = np.zeros(max(n, 1), NODE)
    nodes16 = np.zeros((max(n, 1), 16), np.uint16)
    big = np.zeros(16, np.uint32)
    nn, depth, cap, nbig, root = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32()
    rc = R.lib().rtw_bvh_dump(C.byref(scene.pod), t0, t1, nodes.ctypes.data, len(nodes), C.byref(nn), C.byref(root), C.byref(depth), C.byref(cap),
                              big.ctypes.data, 16, C.byref(nbig), nodes16.ctypes.data)
    assert rc == 0
    return dict(nodes=nodes[:nn.value], nodes16=nodes16[:nn.value], root=root.value, depth=depth.value, cap=cap.value, big=big[:nbig.value].tolist())


def expected_cap(n_leaves, n_spheres, abs_max):
    """The budget, restated: f16 nodes + (depth + 3) stack levels of 256 lanes x 2 bytes within a seventh of 160 KiB -- and, where a
    balanced tree leaves room for the scene's 16 bytes per sphere of geometry within a sixth of it (the shim's rule), still with that room."""
    cap = STACK
    balanced = math.ceil(math.log2(n_leaves)) if n_leaves > 1 else 0
    if 2 <= n_leaves <= LDS_NODES_MAX + 1 and n_spheres <= LDS_GEOM_MAX and abs_max < 30000.0:
        node_bytes = ((n_leaves - 1) * 32 + 15) & ~15
        cap = min(cap, max((160 * 1024 // 7 - node_bytes) // 512 - 3, 0))
        with_geom = max((160 * 1024 // 6 - node_bytes - n_spheres * 16) // 512 - 3, 0)
        if with_geom >= balanced:
            cap = min(cap, with_geom)
    return max(cap, balanced)


def sphere_box(pod, t0, t1):
    f = np.float32
    c = np.array(pod.center[:], f)
    v = np.array(pod.velocity[:], f)
    ends = np.stack([c + v * f(t0), c + v * f(t1)])
    r = abs(f(pod.radius))
    return ends.min(0) - r, ends.max(0) + r


def check_tree(scene, t0=0.0, t1=0.0, finite=True):
    d = dump(scene, t0, t1)
    n = scene.pod.n_spheres
    nodes, seen = d["nodes"], np.zeros(n, np.int64)
    for i in d["big"]:
        seen[i] += 1
    n_leaves = n - len(d["big"])
    assert d["depth"] <= d["cap"] <= STACK
    if d["root"] == EMPTY:
        assert n_leaves == 0 and len(nodes) == 0
        assert (seen == 1).all()
        return d
    assert len(nodes) == n_leaves - 1

    def walk(ref, depth, lo, hi):
        """-> (count, box lo, box hi) of the subtree; asserts containment on the way"""
        if ref < 0:
            s = ~ref
            assert 0 <= s < n
            seen[s] += 1
            assert depth <= d["cap"]
            if finite:
                blo, bhi = sphere_box(scene.pod.spheres[s], t0, t1)
                assert (blo >= lo).all() and (bhi <= hi).all(), (s, blo, bhi, lo, hi)
            return 1
        assert 0 <= ref < len(nodes)
        nd = nodes[ref]
        if finite:
            assert (nd["lo0"] >= lo).all() and (nd["hi0"] <= hi).all() and (nd["lo1"] >= lo).all() and (nd["hi1"] <= hi).all()
        cnt = walk(int(nd["c0"]), depth + 1, nd["lo0"], nd["hi0"]) + walk(int(nd["c1"]), depth + 1, nd["lo1"], nd["hi1"])
        assert depth + math.ceil(math.log2(cnt)) <= STACK           # the invariant, at every node
        return cnt

    inf = np.full(3, np.inf, np.float32)
    assert walk(d["root"], 0, -inf, inf) == n_leaves
    assert (seen == 1).all(), np.nonzero(seen != 1)
    if finite:
        boxes = [sphere_box(scene.pod.spheres[s], t0, t1) for s in range(n) if s not in d["big"]]
        abs_max = max(float(np.abs(np.concatenate(b)).max()) for b in boxes)
        assert d["cap"] == expected_cap(n_leaves, n, abs_max), (d["cap"], n_leaves)
    return d


def S(x, y, z, r, vel=None):
    s = R.Sphere.with_albedo((float(x), float(y), float(z)), float(r), (0.5, 0.5, 0.5))
    if vel is not None:
        s.pod.velocity[0], s.pod.velocity[1], s.pod.velocity[2] = vel
    return s


def field(n_small, n_large, seed=3, ground=False, moving=False):
    """n_small spheres of radius 0.2 on a jittered grid in a slab, n_large of 5x the radius among them (the bench scene's shape)"""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(n_small)))
    sp = [S(0, -1000, 0, 1000)] if ground else []
    for i in range(n_small):
        a, b = i % side - side // 2, i // side - side // 2
        vel = (0.0, float(rng.uniform(0, 15)), 0.0) if moving and i % 3 == 0 else None
        sp.append(S(a + 0.9 * rng.random(), 0.2, b + 0.9 * rng.random(), 0.2, vel))
    for k in range(n_large):
        sp.append(S(-4.0 + 4.0 * k, 1.0, 0.0, 1.0))
    return R.Scene(sp)


def geometric(n, ratio=1.2):
    f = np.float32
    return R.Scene([S(float(f(ratio) ** i), 0.0, -5.0, 0.01) for i in range(n)])


SCENES = {
    "n1": lambda: R.Scene([S(0, 0, -1, 0.5)]),
    "n2": lambda: R.Scene([S(0, 0, -1, 0.5), S(1, 0, -1, 0.5)]),
    "n3": lambda: R.Scene([S(0, 0, -1, 0.5), S(1, 0, -1, 0.5), S(2, 0, -1, 0.25)]),
    "all_centres_equal": lambda: R.Scene([S(1, 2, 3, 0.1 + 0.01 * (i % 5)) for i in range(100)]),
    "geometric_400": lambda: geometric(400),
    "collinear": lambda: R.Scene([S(0.37 * i, 1.0, -2.0, 0.1) for i in range(300)]),
    "bench_shape_480_3": lambda: field(480, 3),
    "bench_shape_with_ground": lambda: field(480, 3, ground=True),
    "lds_nodes_max_minus_1": lambda: field(LDS_NODES_MAX, 0),          # 511 inner nodes
    "lds_nodes_max": lambda: field(LDS_NODES_MAX + 1, 0),              # 512
    "lds_nodes_max_plus_1": lambda: field(LDS_NODES_MAX + 2, 0),       # 513: global nodes, cap = the device stack
    "lds_geom_max_minus_1": lambda: field(LDS_GEOM_MAX - 1, 0),
    "lds_geom_max": lambda: field(LDS_GEOM_MAX, 0),
    "lds_geom_max_plus_1": lambda: field(LDS_GEOM_MAX + 1, 0),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_tree_is_a_partition_with_nested_boxes_within_the_cap(name):
    check_tree(SCENES[name]())


def test_bench_scene_keeps_the_depth_its_lds_share_allows():
    """Book-1 final (seed 42): 485 spheres, 484 of them in the tree -> the budget allows depth 12, and the tree stays at or under the 11 of the builder before."""
    d = check_tree(R.Scene.generate(R.SCENE_C2, 42))
    assert len(d["big"]) == 1 and len(d["nodes"]) == 483 and d["cap"] == 12 and d["depth"] <= 11


def test_cap_binds_on_a_skewed_scene_that_could_live_in_lds():
    """Spheres at x = 1.02^i, n = 500 (all within the f16 range): SAH wants a chain far deeper than the 11 levels that 499 f16 nodes leave
    room for, and the tree stops there."""
    d = check_tree(geometric(500, 1.02))
    assert d["cap"] == 11 and d["depth"] == 11


def test_moving_spheres_with_a_shutter():
    check_tree(field(300, 3, moving=True), 0.0, 1.0 / 30.0)
    check_tree(R.Scene.generate(R.SCENE_C5, 42), 0.0, 1.0 / 30.0)


def shim_span(scene, t0, t1):
    """rtw_ctx_set_scene's scene_span, restated: how far a centre reaches over the shutter, +inf for a NaN radius or a non-finite centre or
    velocity.  rtw_ctx_render sends a scene whose span exceeds 1e18 down the list walk, whatever tree was built."""
    span, tmax = 0.0, max(abs(t0), abs(t1))
    for i in range(scene.pod.n_spheres):
        q = scene.pod.spheres[i]
        vals = [float(q.center[k]) for k in range(3)] + [float(q.velocity[k]) for k in range(3)]
        if math.isnan(q.radius) or not all(math.isfinite(v) for v in vals):
            return math.inf
        span = max(span, max(abs(vals[k]) + abs(vals[3 + k]) * tmax for k in range(3)))
    return span


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e30, 3e38])
def test_non_finite_centres_and_radii_terminate(bad):
    """Must come back, with a tree the device stack can hold and every sphere accounted for once -- and the scene must be one the shim
    demotes to the list walk (its span criterion), so that whatever boxes such members produced are never traversed."""
    sc = field(200, 3)
    for i, k in ((5, 0), (17, 1), (40, 2)):
        sc.pod.spheres[i].center[k] = bad
    sc.pod.spheres[60].radius = bad
    sc.pod.spheres[61].velocity[1] = bad
    d = check_tree(sc, 0.0, 0.5, finite=False)
    assert not shim_span(sc, 0.0, 0.5) <= 1e18


def test_infinite_box_around_a_finite_centre_keeps_the_order_strict():
    """A finite centre with a huge velocity and t_begin < 0 < t_end: the two ends are -inf and +inf, their midpoint is not a number, and the
    builder's sorts must still see a strict weak order (such centroids count as 0).  Terminates, partitions, twice the same bytes."""
    sc = field(200, 3)
    for i in (3, 50, 120):
        sc.pod.spheres[i].velocity[0] = 3e38
    a, b = check_tree(sc, -2.0, 2.0, finite=False), dump(sc, -2.0, 2.0)
    assert a["nodes"].tobytes() == b["nodes"].tobytes()


@pytest.mark.parametrize("name", ["bench_shape_480_3", "geometric_400", "all_centres_equal"])
def test_same_input_same_bytes(name):
    a, b = dump(SCENES[name]()), dump(SCENES[name]())
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["nodes16"].tobytes() == b["nodes16"].tobytes()
    assert (a["root"], a["depth"], a["cap"], a["big"]) == (b["root"], b["depth"], b["cap"], b["big"])


def query(scene, rays, use_tree, t0=0.0, t1=0.0, time=0.0):
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    hit, t, visits = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    assert R.lib().rtw_bvh_query_host(C.byref(scene.pod), t0, t1, rays.ctypes.data, n, time, 0.001, 1e5, int(use_tree),
                                      hit.ctypes.data, t.ctypes.data, visits.ctypes.data) == 0
    return hit, t, visits


@pytest.mark.parametrize("name,moving", [("bench_shape_with_ground", False), ("geometric_400", False), ("lds_nodes_max_plus_1", False), ("moving", True)])
def test_host_traversal_returns_the_list_walks_hit(name, moving):
    """The yardstick's traversal (the device's rules: big list first, rho / tau, f16 planes where the tree has them, near child first) over
    the new tree against a list walk with the same sphere test: same sphere, same t, bit for bit, for 4000 rays -- half from outside towards
    a sphere of the scene, half starting on the ground inside the field."""
    scene = field(300, 3, ground=True, moving=True) if moving else SCENES[name]()
    rng = np.random.default_rng(11)
    n = 4000
    o = np.empty((n, 3), np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    o[: n // 2] = rng.uniform(-30, 30, (n // 2, 3))
    # towards a sphere of the scene, off its centre by up to 0.8 radii
    pods = [scene.pod.spheres[int(i)] for i in rng.integers(0, scene.pod.n_spheres, n // 2)]
    aim = np.array([[q.center[0], q.center[1], q.center[2]] for q in pods], np.float32)
    aim += (rng.uniform(-0.8, 0.8, (n // 2, 3)) * np.array([[abs(q.radius)] for q in pods])).astype(np.float32)
    d[: n // 2] = aim - o[: n // 2]
    o[n // 2:] = np.stack([rng.uniform(-12, 12, n - n // 2), np.full(n - n // 2, 1e-3), rng.uniform(-12, 12, n - n // 2)], 1)
    d[n // 2:, 1] = np.abs(d[n // 2:, 1])
    rays = np.concatenate([o, d], 1)
    t1, tm = (1.0 / 30.0, 0.02) if moving else (0.0, 0.0)
    h_tree, t_tree, visits = query(scene, rays, True, 0.0, t1, tm)
    h_list, t_list, _ = query(scene, rays, False, 0.0, t1, tm)
    assert (h_list >= 0).sum() > n // 10
    assert np.array_equal(h_tree, h_list)
    assert np.array_equal(t_tree.view(np.uint32)[h_list >= 0], t_list.view(np.uint32)[h_list >= 0])
    assert visits.sum() > 0
