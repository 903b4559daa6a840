"""Scenes, rays and range cases of the query-kernel edge tests (test_query_edges_cpu.py proves on the CPU that each set does what its test
needs; test_gpu_query_edges.py runs them through rtw_ctx_scene_hits / rtw_ctx_depth_map).  Everything is deterministic from fixed seeds, and
the f32 restatements below (d.d, |o|_1, the discriminant, the two per-ray fall-back predicates) follow the kernel's expression order
(csrc/rtw_query.hip q_ray_ordinary, csrc/rtw_tri.h tri_ray_ordinary), which is the oracle's."""
import functools

import numpy as np

import rtw_amd as R
from tests.test_gpu_scene_hits import (MAXT, MINT, TIME, bits, centre_of, forced_tree, forty_rays, forty_spheres, geom_scene,  # noqa: F401
                                        oracle_hits)

F = np.float32
INF = float("inf")
NAN = float("nan")
UP, DOWN = F(np.inf), F(-np.inf)


def above(x):
    return float(np.nextafter(F(x), UP))


def below(x):
    return float(np.nextafter(F(x), DOWN))


def same_nan(a, b):
    """Elementwise: the same bits, or a NaN in both (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same_nan(got, want, what):
    """(t, idx[, normals]) against (t, idx[, normals]): indices exactly, floats on the bits, a NaN in both counting as equal."""
    for name, g, w in zip(("t", "idx", "normal"), got, want):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w) if name == "idx" else np.flatnonzero(~same_nan(g, w))
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


def hit_share(idx):
    return float(np.mean(np.asarray(idx).reshape(-1) >= 0))


def as_depth(t, maxt, height, width):
    """The depth map that belongs to scene_hits' t: maxt * 1.6 (an f32 product) where the ray misses."""
    t = np.asarray(t, F)
    return np.where(np.isinf(t) & (t > 0), F(maxt) * F(1.6), t).astype(F).reshape(height, width)


# ---- f32 restatements of what the kernel decides per ray ---------------------------------------------------------------------------

def dot3(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def dd_of(rays):
    rays = np.asarray(rays, F).reshape(-1, 6)
    return dot3(rays[:, 3:], rays[:, 3:]).astype(F)


def l1(v):
    v = np.abs(np.asarray(v, F))
    with np.errstate(all="ignore"):
        return ((v[..., 0] + v[..., 1]).astype(F) + v[..., 2]).astype(F)


def scene_span(scene):
    """The largest |coordinate| a top-level sphere's centre reaches (static scenes): rtw_ctx_set_scene's scene_span, as an f32."""
    return F(max(abs(float(scene._spheres[k].center[j])) for k in range(scene.n_spheres) for j in range(3)))


def reach_product(rays, span):
    """fmaxf(nd, 2) * (span + no + 1) of q_ray_ordinary, in f32."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    no, nd = l1(rays[:, :3]), l1(rays[:, 3:])
    with np.errstate(all="ignore"):
        return (np.fmax(nd, F(2.0)) * ((F(span) + no).astype(F) + F(1.0)).astype(F)).astype(F)


def q_ordinary(rays, span):
    """q_ray_ordinary (csrc/rtw_query.hip) per ray."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    no, nd, a = l1(rays[:, :3]), l1(rays[:, 3:]), dd_of(rays)
    with np.errstate(all="ignore"):
        return ((no + nd).astype(F) < F(2.0 ** 60)) & (a >= F(1e-30)) & (a <= F(1e30)) & (reach_product(rays, span) <= F(1e18))


def tri_sum(rays, t_bound):
    """ao + ad * t_bound of tri_ray_ordinary, in f32."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    ao, ad = np.abs(rays[:, :3]).max(axis=1), np.abs(rays[:, 3:]).max(axis=1)
    with np.errstate(all="ignore"):
        return (ao + (ad * F(t_bound)).astype(F)).astype(F)


def tri_ordinary(rays, t_bound):
    """tri_ray_ordinary (csrc/rtw_tri.h) per ray; the shim drops the triangles' tree for the whole call when t_bound is not finite or above 2^40."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    if not (np.isfinite(t_bound) and t_bound <= 2.0 ** 40):
        return np.zeros(len(rays), bool)
    return np.isfinite(rays).all(axis=1) & (tri_sum(rays, t_bound) <= F(2.0 ** 40))


def a_plain(rays):
    """Lanes whose d.d lies in [2^-20, 2^20]: a wave takes sphere_root's plain sequence only when all of its lanes do."""
    a = np.abs(dd_of(rays))
    return (a >= F(2.0 ** -20)) & (a <= F(2.0 ** 20))


def unit_plain(v):
    """Vectors with every component in [2^-40, 2^40]: unit()'s plain sequence (csrc/rtw_device.h)."""
    v = np.abs(np.asarray(v, F))
    return (v.min(axis=-1) >= F(2.0 ** -40)) & (v.max(axis=-1) <= F(2.0 ** 40))


def sphere_disc(ray, centre, radius):
    """(b, c, disc) of sphere.rs:99-105 in f32, the oracle's expression order."""
    ray = np.asarray(ray, F)
    oc = (ray[:3] - np.asarray(centre, F)).astype(F)
    a, b = dot3(ray[3:], ray[3:]), dot3(oc, ray[3:])
    c = F(dot3(oc, oc) - F(F(radius) * F(radius)))
    return F(b), c, F(F(b * b) - F(a * c))


# ---- Part A: depth maps through the sphere tree ----------------------------------------------------------------------------------------

BOOK1_W, BOOK1_H = 65, 33           # 2145 pixels: not a multiple of 256, the last wave is ragged
FORTY_W, FORTY_H = 33, 17


@functools.lru_cache(maxsize=None)
def book1_scene():
    return R.Scene.generate(R.SCENE_C2)


def book1_camera(width=BOOK1_W, height=BOOK1_H):
    return R.camera2_new(width / height, (13.0, 2.0, 3.0), (0.0, 1.0, 0.0), (-13.0, -2.0, -3.0), 60.0, 0.0)


def forty_camera(width=FORTY_W, height=FORTY_H):
    return R.camera2_new(width / height, (0.0, 3.0, 9.0), (0.0, 1.0, 0.0), (0.0, -3.0, -9.0), 40.0, 0.0)


@functools.lru_cache(maxsize=None)
def forty_scene():
    return forty_spheres()


@functools.lru_cache(maxsize=None)
def map_reference(O, which):
    """(scene, camera, width, height, time, the oracle's (t, idx, normal) of the map's rays)."""
    if which == "book1":
        scene, cam, w, h, time = book1_scene(), book1_camera(), BOOK1_W, BOOK1_H, 0.0
    else:
        scene, cam, w, h, time = forty_scene(), forty_camera(), FORTY_W, FORTY_H, TIME
    rays = R.depth_rays(cam, w, h)
    return scene, cam, w, h, time, oracle_hits(O, scene, rays, time, MINT, MAXT)


# ---- Part B: range edges --------------------------------------------------------------------------------------------------------------

def _next_behind(O, scene, ray, time, t_near, maxt):
    t, idx, _ = oracle_hits(O, scene, ray[None, :], time, above(t_near), maxt)
    return float(t[0]), int(idx[0])


def edge_cases(t_near, t_next, maxt):
    """The (mint, maxt) cases about a ray whose first hit is at t_near and whose next root or sphere behind it is at t_next (inf: none)."""
    nothing = float(F(t_near) * F(0.5))
    cases = [(MINT, maxt),
             (MINT, below(t_near)), (MINT, t_near),                      # maxt just below / exactly at the hit
             (t_near, maxt), (above(t_near), maxt),                      # mint exactly at / just above it: the next root or sphere
             (t_near, t_near), (nothing, nothing),                       # mint == maxt at a hit, and where nothing is
             (MINT, INF), (-1.0, maxt), (maxt, MINT), (0.0, maxt)]       # maxt = +inf, mint = -1, mint > maxt, mint = 0
    if np.isfinite(t_next):
        cases += [(above(t_near), below(t_next)), (above(t_near), t_next), (t_next, t_next)]      # the far root out of range too / at maxt
    return cases


@functools.lru_cache(maxsize=None)
def range_reference(O, which):
    """(scene, time, rays [k][6], [(mint, maxt, the oracle's answer for all k rays, the ray the case was made for)], base answer).
    forty: 8 rays from outside the field whose answer is a sphere; book1: a ray that ends on the ground (index 0, outside the tree) and one
    that ends on a small sphere."""
    if which == "forty":
        scene, time, maxt = forty_scene(), TIME, 30.0
        rng = np.random.default_rng(41)
        cand = np.empty((64, 6), F)
        for k in range(len(cand)):
            o = np.array([0.0, 3.0, 9.0]) + rng.uniform(-0.3, 0.3, 3)
            d = centre_of(scene, int(rng.integers(0, 40)), TIME) + rng.normal(0, 0.2, 3) - o
            cand[k, :3], cand[k, 3:] = o, d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        t, idx, _ = oracle_hits(O, scene, cand, time, MINT, maxt)
        behind = [_next_behind(O, scene, cand[k], time, t[k], maxt) if idx[k] >= 0 else (INF, -1) for k in range(len(cand))]
        other = [k for k in range(len(cand)) if idx[k] >= 0 and behind[k][1] >= 0 and behind[k][1] != idx[k]][:4]     # another sphere behind
        own = [k for k in range(len(cand)) if idx[k] >= 0 and behind[k][1] == idx[k] and k not in other][:4]           # the far root behind
        pick = other + own
        assert len(pick) == 8
    else:
        scene, time, maxt = book1_scene(), 0.0, MAXT
        cand = np.array([[13.0, 2.0, 3.0, -9.0, -2.0, -1.5],                                   # down onto the ground
                         [13.0, 2.0, 3.0, *(centre_of(scene, 1) - np.array([13.0, 2.0, 3.0]))]], F)
        cand[1, 3:] *= F(0.125)
        t, idx, _ = oracle_hits(O, scene, cand, time, MINT, maxt)
        behind = [_next_behind(O, scene, cand[k], time, t[k], maxt) for k in range(len(cand))]
        pick = [0, 1]
    rays = np.ascontiguousarray(cand[pick])
    cases = []
    for j, k in enumerate(pick):
        for mint_c, maxt_c in edge_cases(float(t[k]), behind[k][0], maxt):
            cases.append((mint_c, maxt_c, oracle_hits(O, scene, rays, time, mint_c, maxt_c), j))
    base = tuple(a[pick] for a in (t, idx))
    return scene, time, rays, cases, base


# ---- Parts C and D: the scene ----------------------------------------------------------------------------------------------------------

EYE = np.array([0.0, 0.3, 1.5])


@functools.lru_cache(maxsize=None)
def field_scene():
    """geom_scene() (three spheres, two quads, two instances, the triangles with their tree) plus 60 small spheres among its objects: 63
    top-level spheres, so that a forced tree is a real one."""
    g = geom_scene()
    rng = np.random.default_rng(19)
    sp = [R.Sphere(R.RtwSphere.from_buffer_copy(g._spheres[k])) for k in range(g.n_spheres)]
    for _ in range(60):
        c = rng.uniform((-3.0, -1.2, -5.5), (3.0, 2.6, -1.5))
        sp.append(R.Sphere.new(tuple(float(x) for x in c), float(rng.uniform(0.1, 0.3)), (0.5, 0.5, 0.5), R.SCATTER_M))
    scene = R.Scene(sp, triangles=[g.triangles[i] for i in range(g.n_triangles)])
    pool = lambda arr, n: [type(arr[0]).from_buffer_copy(arr[i]) for i in range(n)]
    scene._install_geom(pool(g._quads, g.pod.n_quads), pool(g._instances, g.pod.n_instances), pool(g._inst_spheres, g.pod.n_inst_spheres),
                        pool(g._inst_quads, g.pod.n_inst_quads))
    return scene


def ordinary_rays(n, seed):
    """From about the eye point into the field: half aimed at sphere centres, half at the back wall and the sky about it; |d| in 0.5 .. 2,
    every component away from zero."""
    scene = field_scene()
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), F)
    k = 0
    while k < n:
        o = EYE + rng.uniform(-0.2, 0.2, 3)
        if k % 2 == 0:
            target = centre_of(scene, int(rng.integers(0, scene.n_spheres))) + rng.normal(0, 0.15, 3)
        else:
            target = np.array([rng.uniform(-5.5, 5.5), rng.uniform(-3.5, 5.5), -6.0])
        d = target - o
        rays[k, :3], rays[k, 3:] = o, d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        k += bool(np.all(np.abs(rays[k, 3:]) > 1e-4))                   # (drawn again otherwise)
    return rays


def aimed(n, seed, length, origin=EYE, jitter=0.05):
    """n rays from `origin` at sphere centres of the field, direction length `length`."""
    scene = field_scene()
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), F)
    for k in range(n):
        o = np.asarray(origin, np.float64) + rng.uniform(-0.1, 0.1, 3)
        d = centre_of(scene, int(rng.integers(0, scene.n_spheres))) + rng.normal(0, jitter, 3) - o
        rays[k, :3], rays[k, 3:] = o, d / np.linalg.norm(d) * length
    return rays


def tangent_rays():
    """Rays that start ON one of the three large spheres (c == 0 in f32) and leave it at a right angle but for a tiny component towards it:
    b is tiny, so the discriminant b * b - a * 0 is positive and far below 2^-60 -- outside sphere_root's plain range.  The last one has
    b == 0 too: a discriminant of exactly +0 (b * b is never -0, so a discriminant of -0 cannot be reached through sphere.rs:105)."""
    out = []
    for (cx, cy, cz), r in (((0.0, -0.4, -3.0), 0.5), ((0.5, -0.2, -3.4), 0.6), ((-2.4, 1.6, -4.0), 0.4)):
        for eps in (1e-12, -3e-13, 2e-15, 1e-20):
            out.append([float(F(cx) + F(r)), cy, cz, eps, 0.0, -1.0])
            out.append([float(F(cx) + F(r)), cy, cz, eps, 0.25, -1.0])
    rays = np.array(out, F)
    sph = [((0.0, -0.4, -3.0), 0.5)] * 8 + [((0.5, -0.2, -3.4), 0.6)] * 8 + [((-2.4, 1.6, -4.0), 0.4)] * 8
    keep = [k for k in range(len(rays)) if 0.0 < sphere_disc(rays[k], *sph[k])[2] < F(2.0 ** -60)]
    zero = np.array([[0.5, -0.4, -3.0, 0.0, 0.0, -1.0]], F)
    return np.concatenate([rays[keep], zero]), [sph[k] for k in keep] + [sph[0]]


# (mint, maxt) per range class.  "plain": finite, so the triangles' tree is in use (t_bound = 2^20 makes tri_ray_ordinary's bound max|d| <= 2^20
# for origins about the eye); "far": maxt = +inf for hits at t ~ 1e15 (the shim drops the triangles' tree for the call); "near": hits at t ~ 1e-14.
RANGES = {"plain": (1e-9, 1048576.0), "far": (MINT, INF), "near": (1e-18, 1000.0)}


@functools.lru_cache(maxsize=None)
def edge_kinds():
    """[(name, range class, rays [k][6], what the CPU module checks)].  A check is (predicate name, expected value per ray) or None."""
    s = lambda v: float(np.sqrt(v))
    K = []
    # either side of a_plain: d.d = 2^-21, 2^-19, 2^19, 2^21
    for e in (-21, -19, 19, 21):
        K.append((f"dd=2^{e}", "plain", aimed(12, 100 + e, s(2.0 ** e)), ("a_plain", abs(e) < 20)))
    # either side of q_ray_ordinary's d.d bounds
    for v, inside in ((0.9e-30, False), (1.1e-30, True)):
        K.append((f"dd={v}", "far", aimed(12, 7, s(v)), ("q_ordinary", inside)))
    for v, inside in ((0.9e30, True), (1.1e30, False)):
        K.append((f"dd={v}", "near", aimed(12, 8, s(v), origin=(0.0, 0.3, 60.0)), ("q_ordinary", inside)))
    # |o|_1 either side of 2^60 (|d| tiny, so that |o| + |d| is |o|): aimed back at the scene
    for name, ox in (("below", below(2.0 ** 60)), ("above", 2.0 ** 60)):
        K.append((f"|o|_1 {name} 2^60", "far", np.array([[ox, 0.0, 0.0, -1.0, 0.0, 0.0], [0.0, 0.0, ox, 1e-3, 2e-3, -1.0]], F),
                  ("l1o<2^60", name == "below")))
    # nd * (span + no + 1) either side of 1e18: |d| = 8e14 (nd about 8.3e14) from 1000 / 1500 away
    for name, dist in (("below", 1000.0), ("above", 1500.0)):
        K.append((f"reach {name} 1e18", "near", aimed(12, 9, 8e14, origin=(0.0, 0.3, dist)), ("reach<=1e18", name == "below")))
    # either side of tri_ray_ordinary: max|d_i| = 2^20 / the next float, and an origin 2^40 away
    tri_in = aimed(12, 10, 1.0)
    tri_out = tri_in.copy()
    for k in range(len(tri_in)):
        d = tri_in[k, 3:].astype(np.float64)
        j = int(np.argmax(np.abs(d)))
        d = d / abs(d[j]) * 2.0 ** 20
        tri_in[k, 3:] = tri_out[k, 3:] = d
        tri_in[k, 3 + j] = np.sign(d[j]) * 2.0 ** 20                   # max |d_i| = 2^20 exactly: ao + 2^40 rounds to 2^40
        tri_out[k, 3 + j] = np.sign(d[j]) * above(2.0 ** 20)           # ... and the next float: 2^40 + 2^17
    K.append(("tri inside", "plain", tri_in, ("tri_ordinary", True)))
    K.append(("tri outside", "plain", tri_out, ("tri_ordinary", False)))
    K.append(("tri far origin", "plain", np.array([[0.0, 0.3, above(2.0 ** 40), 0.0, 1e-3, -1.0], [below(-2.0 ** 40), 0.3, -3.0, 1.0, 1e-3, 1e-3]], F),
              ("tri_ordinary", False)))
    # degenerate directions and non-finite rays
    base = aimed(8, 11, 1.0)
    zero = base.copy(); zero[:, 3:] = 0.0; zero[1, 5] = -0.0
    K.append(("zero direction", "plain", zero, ("q_ordinary", False)))
    nan = np.repeat(base[:1], 6, axis=0)
    nan[0, 3] = NAN; nan[1, 1] = NAN; nan[2, [3, 4]] = NAN; nan[3, [0, 5]] = NAN; nan[4, 3:] = NAN; nan[5, :3] = NAN
    K.append(("NaN components", "plain", nan, ("q_ordinary", False)))
    inf = np.repeat(base[:1], 6, axis=0)
    inf[0, 0] = INF; inf[1, 2] = -INF; inf[2, 3] = INF; inf[3, 5] = -INF; inf[4, [1, 4]] = INF; inf[5, 3:] = -INF
    K.append(("inf components", "plain", inf, ("q_ordinary", False)))
    # one direction component denormal -- all but one below 2^-127, where 1 / d overflows -- or a signed zero, the others ordinary: straight at
    # the icosphere, the spheres and the wall, as zero_component_rays do
    for name, values in (("components below 2^-126", (1e-40, -1e-40, 2.0 ** -149, 2.0 ** -128, -(2.0 ** -130), 2.0 ** -127)), ("signed-zero components", (-0.0, 0.0))):
        tiny = []
        for v in values:
            for ox, oy in ((0.0, 1.3), (0.2, -0.3), (-2.4, 1.6), (0.45, 0.9)):
                tiny.append([ox, oy, 1.5, v, 0.01, -1.0])
                tiny.append([ox, oy, 1.5, 0.01, v, -1.25])
        if values[0] == 0.0:
            tiny.append([0.1, 4.0, -3.4, -0.0, -1.0, -0.0])
        K.append((name, "plain", np.array(tiny, F), ("tiny", values[0] != 0.0)))
    K.append(("tangent", "plain", tangent_rays()[0], ("tangent", True)))
    return K


def scatter(base, rays, seed):
    """`rays` put into a copy of `base` at seeded positions (returned, sorted): each among ordinary wave-mates."""
    pos = np.sort(np.random.default_rng(seed).choice(len(base), len(rays), replace=False))
    out = base.copy()
    out[pos] = rays
    return out, pos


@functools.lru_cache(maxsize=None)
def edge_reference(O):
    """Per range class: (mint, maxt, [(name, slice)], all its kinds' rays in a row, a 512-ray ordinary batch with those rays scattered through
    it, their positions, the oracle's answer for the row and for the batch)."""
    scene = field_scene()
    out = {}
    for k, (cls, (mint, maxt)) in enumerate(RANGES.items()):
        kinds = [(name, rays) for name, c, rays, _ in edge_kinds() if c == cls]
        row = np.concatenate([r for _, r in kinds])
        cuts, at = [], 0
        for name, r in kinds:
            cuts.append((name, slice(at, at + len(r))))
            at += len(r)
        batch, pos = scatter(ordinary_rays(512, 300 + k), row, 400 + k)
        out[cls] = (mint, maxt, cuts, row, batch, pos, oracle_hits(O, scene, row, 0.0, mint, maxt), oracle_hits(O, scene, batch, 0.0, mint, maxt))
    return out


# ---- Part D: one spoiler per wave --------------------------------------------------------------------------------------------------------

D_MINT, D_MAXT = RANGES["plain"]
LANES = [(7 * w * w + (0, 31, 32, 63)[w % 4]) % 64 if w >= 4 else (0, 31, 32, 63)[w] for w in range(16)]      # the spoiler's lane, wave by wave


def spoiler_rays():
    """{kind: 16 rays}: what each spoiler switches is said in test_gpu_query_edges.py and proved in test_query_edges_cpu.py."""
    far = np.array([0.0, 0.3, 6e17])
    tang = tangent_rays()[0]
    zero = aimed(16, 21, 1.0)
    zero[:, 3] = 0.0                                                     # d.x == 0: any_zero in q_tri_tree
    scene = field_scene()
    for k in range(8):                                                   # ... and from the x of a sphere's centre at that centre: the hit's normal has
        c = centre_of(scene, (0, 1, 2, 5, 9, 14, 20, 33)[k])            # x == 0 exactly, which sends unit() down its generic path
        o = np.array([c[0], 0.3 + 0.05 * k, 1.5])
        d = c - o
        zero[2 * k, :3], zero[2 * k, 3:] = o, d / np.linalg.norm(d) * (0.6 + 0.1 * k)
        zero[2 * k, 0], zero[2 * k, 3] = scene._spheres[(0, 1, 2, 5, 9, 14, 20, 33)[k]].center[0], 0.0
    nan = aimed(16, 22, 1.0)
    nan[np.arange(16), 3 + np.arange(16) % 3] = NAN
    beyond = np.array([[0.0, 0.3, above(2.0 ** 40) * (1 + k), 1e-3, 2e-3, -1.0] for k in range(16)], F)
    return {"dd outside [2^-20, 2^20]": np.concatenate([aimed(8, 23, 2.0 ** -10.5), aimed(8, 24, 2.0 ** 10.5)]),
            "tangent, disc < 2^-60": tang[np.arange(16) % (len(tang) - 1)],
            "zero direction component": zero,
            "refused by q_ray_ordinary (dd < 1e-30)": aimed(16, 25, 0.9e-15),
            "refused by q_ray_ordinary (far origin)": aimed(16, 26, 1.0, origin=far),
            "refused by tri_ray_ordinary": beyond,
            "NaN": nan}


def spoil(base, rays):
    """A copy of `base` (1024 rays) with rays[w] at lane LANES[w] of wave w."""
    pos = np.array([64 * w + LANES[w] for w in range(16)])
    out = base.copy()
    out[pos] = rays
    return out, pos


@functools.lru_cache(maxsize=None)
def wave_reference(O):
    """(the 1024 ordinary rays, the oracle's answer for them, {kind: (spoiled launch, positions, the oracle's answer for the 16 spoilers)})."""
    scene = field_scene()
    base = ordinary_rays(1024, 31)
    want = oracle_hits(O, scene, base, 0.0, D_MINT, D_MAXT)
    kinds = {}
    for name, rays in spoiler_rays().items():
        launch, pos = spoil(base, rays)
        kinds[name] = (launch, pos, oracle_hits(O, scene, rays, 0.0, D_MINT, D_MAXT))
    return base, want, kinds


MIXED_W, MIXED_H = 34, 15         # 510 pixels: seven whole waves and one of 62 lanes


def mixed_camera(width=MIXED_W, height=MIXED_H):
    """Axis-aligned: d.x = pixel00.x + delta_u.x * (i / width) is exactly zero where i / width = 1 / 2, so in column width / 2 of an EVEN width
    and nowhere else (Rust2's depth_map puts no half pixel into the ray, so an odd width has no such column)."""
    return R.camera2_new(width / height, (0.0, 0.3, 1.5), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), 75.0, 0.0)


@functools.lru_cache(maxsize=None)
def mixed_reference(O):
    scene = geom_scene()
    cam = mixed_camera()
    rays = R.depth_rays(cam, MIXED_W, MIXED_H)
    return scene, cam, rays, oracle_hits(O, scene, rays, 0.0, MINT, MAXT)


# ---- Part C: the shim's whole-call fall-backs ---------------------------------------------------------------------------------------------

FALLBACK_MAXT = 12.0
FALLBACKS = {"time before t_begin": (-0.5, MINT, FALLBACK_MAXT), "time after t_end": (1.5, MINT, FALLBACK_MAXT),
             "NaN mint": (TIME, NAN, FALLBACK_MAXT), "NaN maxt": (TIME, MINT, NAN), "NaN time": (NAN, MINT, FALLBACK_MAXT)}


@functools.lru_cache(maxsize=None)
def fallback_reference(O):
    """(the forty spheres, 256 rays into them, the oracle's answer inside the time range, {case: (time, mint, maxt, the oracle's answer)})."""
    scene = forty_scene()
    rays = forty_rays(scene, n=256, seed=13)
    inside = oracle_hits(O, scene, rays, TIME, MINT, FALLBACK_MAXT)
    return scene, rays, inside, {name: (tm, lo, hi, oracle_hits(O, scene, rays, tm, lo, hi)) for name, (tm, lo, hi) in FALLBACKS.items()}
