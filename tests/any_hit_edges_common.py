"""Inputs and references of the edge tests of the two fused any-hit passes, ambient occlusion and direct lighting, at the arguments their
own tests leave at one value: the seed, the range, the time and the lights' geometry (tests/test_any_hit_edges_cpu.py proves on the CPU, with
the oracle and the host forms, that every input set reaches the edge it is named for; tests/test_gpu_any_hit_edges.py runs them through
rtw_ctx_ambient_occlusion, rtw_ctx_ao_map, rtw_ctx_direct_light and rtw_ctx_direct_light_map).  Everything is deterministic from fixed seeds,
every helper of an existing module is imported from it, and every reference is computed once."""
import functools

import numpy as np

import rtw_amd as R
from tests import ao_common as AO
from tests import direct_light_common as DL
from tests import query_edges_common as QE
from tests.test_gpu_scene_hits import TIME, geom_scene, oracle_hits

F = np.float32
NAN, INF = QE.NAN, QE.INF
SEEDS = (1, 0xDEADBEEF, 0xFFFFFFFF, 0x61C88647)              # with the last one seed + 0x9E3779B9 wraps to 0
POINTS_AT = {16: 257, 128: 33}                               # points per sample count where a case is about an argument: the ONE build, the round loop
UP = np.array([0.0, 1.0, 0.0], F)


def upward(n):
    n = n.copy()
    n[:, 1] = np.abs(n[:, 1])
    return n


# ---- the sets: name -> (scene, (t_begin, t_end), time, points, normals[, lights]) -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ao_set(O, name):
    """The points of AO.points_of: ("field" | "forty") -> (scene, shutter, time, points, normals, radius)."""
    scene, shutter, _, time, _, _ = AO.case(name)
    p, n = AO.points_of(O, name)
    return scene, shutter, time, p, n, AO.RADIUS[name]


@functools.lru_cache(maxsize=None)
def ao_oracle(O, name, n_points, samples, seed=0, time=None, mint=AO.AO_MINT, radius=None):
    """(counts [n_points], ao) of the first n_points of ao_set(name) from the oracle over the rays of ao_rays."""
    scene, _, t, p, n, r = ao_set(O, name)
    time, radius = t if time is None else time, r if radius is None else radius
    rays = R.ao_rays(p[:n_points], n[:n_points], samples, seed)
    occ = oracle_hits(O, scene, rays.reshape(-1, 6), time, mint, radius)[1] >= 0
    counts = occ.reshape(-1, samples).sum(axis=1)
    return counts, AO.ao_of(counts, samples)


def flat_scene():
    """Direct lighting with an edge that is exact by construction: points on the plane y = 0 with the normal +y, a quad light in the plane
    y = 2, a blocker quad in the plane y = 1 under half of it, and one far sphere so that the sphere group is not empty.  Every cast segment
    has d.y == 2.0f exactly and meets the blocker's plane at t == 0.5 exactly."""
    light = R.Quad.new((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0))
    blocker = R.Quad.new((-1.0, 1.0, -1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 2.0))
    return R.Scene([R.Sphere.new((0.0, -50.0, 0.0), 1.0, (0.5, 0.5, 0.5), R.SCATTER_M)], quads=[light, blocker])


def corner_scene():
    """A large quad light and a blocker above a part of it; corner_points() lie close to its origin corner, so an item's weights
    (n.d)|g.d| / (d.d)^2 span many binades."""
    light = R.Quad.new((0.0, 2.0, 0.0), (16.0, 0.0, 0.0), (0.0, 0.0, 16.0))
    blocker = R.Quad.new((3.0, 1.0, -1.0), (20.0, 0.0, 0.0), (0.0, 0.0, 6.0))
    return R.Scene([R.Sphere.new((8.0, 1.0, 12.0), 1.5, (0.5, 0.5, 0.5), R.SCATTER_M)], quads=[light, blocker])


def corner_points():
    rng = np.random.default_rng(23)
    p = np.zeros((8, 3), F)
    p[:, 0], p[:, 2] = rng.uniform(-0.05, 0.3, 8), rng.uniform(-0.05, 0.3, 8)
    p[:, 1] = 2.0 - np.array([0.01, 0.02, 0.03, 0.05, 0.08, 0.12, 0.2, 0.3])
    return p, np.tile(UP, (8, 1))


MOVING_LIGHTS = {"5": [(R.LIGHT_SPHERE, 5)], "1": [(R.LIGHT_SPHERE, 1)], "9": [(R.LIGHT_SPHERE, 9)],
                 "5+20": [(R.LIGHT_SPHERE, 5), (R.LIGHT_SPHERE, 20)], "38+9": [(R.LIGHT_SPHERE, 38), (R.LIGHT_SPHERE, 9)]}
MOVING_POINTS = 257                                          # x 16 samples: about 2000 cast segments a light


@functools.lru_cache(maxsize=None)
def dl_set(O, name):
    """name -> (scene, lights, shutter, time, points, normals): the cases of DL.case; "flat"; "corner"; "moving <key of MOVING_LIGHTS>":
    forty_spheres() lit by spheres that move; "surface": geom_scene() lit by its sphere light alone."""
    if name in DL.CASES:
        scene, lights, shutter, _, time, _, _ = DL.case(name)
        return (scene, lights, shutter, time) + DL.points_of(O, name)
    if name == "surface":
        scene, lights, shutter, _, time, _, _ = DL.case("geom")
        return (scene, lights[1:], shutter, time) + DL.points_of(O, "geom")
    if name == "flat":
        rng = np.random.default_rng(5)
        p = np.zeros((64, 3), F)
        p[:, 0], p[:, 2] = rng.uniform(-1.0, 1.0, 64), rng.uniform(-1.0, 1.0, 64)
        return flat_scene(), [(R.LIGHT_QUAD, 0)], (0.0, 0.0), 0.0, p, np.tile(UP, (64, 1))
    if name == "corner":
        return (corner_scene(), [(R.LIGHT_QUAD, 0)], (0.0, 0.0), 0.0) + corner_points()
    assert name.startswith("moving "), name
    scene, _, shutter, _, time, _, _ = DL.case("forty")
    p, n = DL.points_of(O, "forty")
    return scene, MOVING_LIGHTS[name[7:]], shutter, time, np.ascontiguousarray(p[:MOVING_POINTS]), np.ascontiguousarray(n[:MOVING_POINTS])


def dl_answer(O, scene, lights, p, n, samples, seed, time, lo, hi):
    """(vis, irr, v, cast counts, occluded [n][n_lights][samples]) from the oracle: every cast ray of light_samples traced over [lo, hi]."""
    rays, w = R.light_samples(scene, lights, p, n, samples, seed)
    cast = DL.cast_mask(rays)
    occ = np.zeros(cast.shape, bool)
    if cast.any():
        occ[cast] = oracle_hits(O, scene, rays[cast], time, lo, hi)[1] >= 0
    return DL.outputs(w, cast, occ, samples) + (cast.sum(axis=-1), occ)


@functools.lru_cache(maxsize=None)
def dl_oracle(O, name, n_points, samples, seed=0, time=None, lo=DL.LO, hi=DL.HI):
    """dl_answer of the first n_points of dl_set(name)."""
    scene, lights, _, t, p, n = dl_set(O, name)
    return dl_answer(O, scene, lights, p[:n_points], n[:n_points], samples, seed, t if time is None else time, lo, hi)


MAP_SIZES = ((16, 16, 12), (128, 6, 4))                      # (samples, width, height) of the camera forms' cases over geom_scene()
MAP_RANGE, MAP_RADIUS = (0.25, 0.75), 1.5                    # another range than the default of either second pass


def map_points_by_the_oracle(O, scene, cam, width, height, time, mint, maxt):
    """The points and faced normals a camera form shades, from the oracle's closest hits of the depth rays (the depth pass is held to
    them bit for bit by tests/test_gpu_scene_hits.py): what TA.map_points forms from the device's depth map."""
    rays = R.depth_rays(cam, width, height)
    t, idx, nrm = oracle_hits(O, scene, rays, time, mint, maxt)
    hit = idx >= 0
    o, d = rays[:, :3], rays[:, 3:]
    p = (o + (d * np.where(hit, t, F(0.0))[:, None]).astype(F)).astype(F)
    faced = np.where((DL.dot(d, nrm) > 0.0)[:, None], -nrm, nrm).astype(F)
    faced[~hit] = 0.0
    p[~hit] = 0.0
    return p, faced, hit


# ---- 2. ranges ------------------------------------------------------------------------------------------------------------------------------------
HALF = 0.5
FLAT_RANGES = {"hi at the blocker": (DL.LO, HALF), "hi one ulp before it": (DL.LO, QE.below(HALF)), "lo at the blocker": (HALF, DL.HI),
               "lo one ulp behind it": (QE.above(HALF), DL.HI), "lo > hi": (0.6, 0.4), "lo = 0": (0.0, DL.HI), "lo = -1": (-1.0, DL.HI),
               "hi = 1": (DL.LO, 1.0)}
FLAT_CLOSED = ("hi at the blocker", "lo at the blocker")
FLAT_OPEN = ("hi one ulp before it", "lo one ulp behind it", "lo > hi")
SURFACE_HI = (DL.HI, 1.0, 1.0 + 1e-3)                        # the light's own surface left out, decided root by root, taken in

AO_EDGE_POINTS = 65                                          # the launch of an AO range-edge case: the first points of the set
AO_EDGE_RAYS = 8                                             # chosen rays per set: 16 in all
AO_CLASSES = {"mint = 0": (0.0, None), "mint = radius": (0.5, 0.5), "mint > radius": (1.0, 0.5), "radius = inf": (AO.AO_MINT, INF),
              "radius = 1e30": (AO.AO_MINT, 1e30)}


@functools.lru_cache(maxsize=None)
def ao_edge_reference(O, name):
    """[(point i, sample k, t, [(mint, radius, occluded bit of ray (i, k) in the oracle, the oracle's count of point i)] x 4)]: AO_EDGE_RAYS rays
    of the first AO_EDGE_POINTS points of ao_set(name) at 16 samples whose closest hit t the oracle reports within [AO_MINT, radius] and
    behind which it reports nothing (the CPU module checks that again); the four ranges put t at either end and one ulp outside."""
    scene, _, time, p, n, radius = ao_set(O, name)
    rays = R.ao_rays(p[:AO_EDGE_POINTS], n[:AO_EDGE_POINTS], 16, 0)
    t, idx, _ = oracle_hits(O, scene, rays.reshape(-1, 6), time, AO.AO_MINT, radius)
    out, used = [], set()
    for j in np.flatnonzero(idx >= 0):
        i, k = divmod(int(j), 16)
        if i in used or not AO.AO_MINT < t[j] < radius:
            continue
        if oracle_hits(O, scene, rays[i, k][None, :], time, QE.above(t[j]), 1e30)[1][0] >= 0:
            continue
        tj, cases = float(t[j]), []
        for mint, rad in ((AO.AO_MINT, tj), (AO.AO_MINT, QE.below(tj)), (tj, radius), (QE.above(tj), radius)):
            occ = oracle_hits(O, scene, rays[i], time, mint, rad)[1] >= 0
            cases.append((mint, rad, bool(occ[k]), int(occ.sum())))
        out.append((i, k, tj, cases))
        used.add(i)
        if len(out) == AO_EDGE_RAYS:
            break
    return out


# ---- 3. whole-call fall-backs ------------------------------------------------------------------------------------------------------------------
# (time, lo or mint, hi or radius; None: the pass's ordinary value).  The forty spheres move over the shutter [0, 1].
INSIDE = {"inside the shutter": (TIME, None, None), "time = t_begin": (0.0, None, None), "time = t_end": (1.0, None, None)}
FALLBACKS = {"time before t_begin": (-0.5, None, None), "time after t_end": (1.5, None, None), "NaN time": (NAN, None, None),
             "NaN lo": (TIME, NAN, None), "NaN hi": (TIME, None, NAN)}
FALLBACK_POINTS = 129


# ---- 5. light and point geometry at the edges ---------------------------------------------------------------------------------------------------
EDGE_POINTS = 128
TINY = np.array([2.5, 1.0, 2.5])                            # the tiny quad light's origin; its edges are 1e-4
BULB = (np.array([1.5, 3.0, 0.5]), 0.5)                     # the sphere light
CEILING_Y = 4.0
EDGE_SPHERES = 48


@functools.lru_cache(maxsize=None)
def edge_scene():
    """48 small spheres in the air above a field of points, then the sphere light BULB and a sphere of radius 1e-13 at the origin; quad 0 the
    ceiling light in the plane y = 4 exactly (cross(u, v) = (0, -16, 0)), quad 1 the tiny light, quad 2 an occluder.
    Returns (Scene, the ordinary light list, the list with the sphere of radius 1e-13 in the tiny quad's place)."""
    rng = np.random.default_rng(29)
    sp = []
    for _ in range(EDGE_SPHERES):
        c = rng.uniform((-3.0, 0.8, -3.0), (3.0, 2.6, 3.0))
        sp.append(R.Sphere.new(tuple(float(x) for x in c), float(rng.uniform(0.1, 0.35)), (0.5, 0.5, 0.5), R.SCATTER_M))
    sp.append(R.Sphere.new(tuple(float(x) for x in BULB[0]), BULB[1], (1.0, 1.0, 1.0), R.SCATTER_M))
    sp.append(R.Sphere.new((0.0, 0.0, 0.0), 1e-13, (1.0, 1.0, 1.0), R.SCATTER_M))
    quads = [R.Quad.new((-2.0, CEILING_Y, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0)),
             R.Quad.new(tuple(float(x) for x in TINY), (1e-4, 0.0, 0.0), (0.0, 0.0, 1e-4)),
             R.Quad.new((-3.0, 2.8, -1.0), (2.5, 0.0, 0.5), (0.0, 0.3, 2.0))]
    lights = [(R.LIGHT_QUAD, 0), (R.LIGHT_SPHERE, EDGE_SPHERES), (R.LIGHT_QUAD, 1)]
    return R.Scene(sp, quads=quads), lights, lights[:2] + [(R.LIGHT_SPHERE, EDGE_SPHERES + 1)]


@functools.lru_cache(maxsize=None)
def edge_points():
    rng = np.random.default_rng(37)
    p = rng.uniform((-3.0, -0.5, -3.0), (3.0, 0.5, 3.0), (EDGE_POINTS, 3)).astype(F)
    v = rng.normal(size=(EDGE_POINTS, 3))
    return p, upward((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F))


# one spoiler point in every four, its place among them varying: at 16 samples and three lights a wave holds four items, so a spoiler's item
# under light l sits at place (3 i + l) % 4 of wave (3 i + l) / 4, next to items of its ordinary neighbours
SPOILED = np.arange(0, EDGE_POINTS, 4) + (np.arange(EDGE_POINTS // 4) * 7) % 4
# kind -> (point, normal, which light list, the light the kind is about)
SPOILERS = {
    "a far light": ((300.0, -1900.0, 400.0), (0.0, 1.0, 0.0), 0, None),                  # every light is 2000 away: d.d > 2^20
    "a tiny near light": (tuple(TINY + (5e-5, -3e-4, 5e-5)), (0.0, 1.0, 0.0), 0, 2),     # 3e-4 under the tiny quad: d.d < 2^-20
    "in the plane of the quad light": ((-5.0, CEILING_Y, 0.5), (1.0, 0.0, 0.0), 0, 0),   # d.y == 0: g.d == 0, the weight is a zero
    "inside the sphere light": (tuple(BULB[0] + (0.1, 0.05, -0.1)), (0.0, 1.0, 0.0), 0, 1),
    "so far that dd * dd overflows": ((0.0, -5e9, 0.0), (0.0, 1.0, 0.0), 0, None),      # the weight is num / inf = 0
    "so near that dd * dd underflows": ((0.0, -1e-12, 0.0), (0.0, 1.0, 0.0), 1, 2),      # 1e-12 under the sphere of radius 1e-13: x / 0
}


def spoiled(kind):
    """(lights, points, normals) of the edge launch with SPOILERS[kind] at the points SPOILED."""
    _, plain, under = edge_scene()
    sp, sn, which, _ = SPOILERS[kind]
    p, n = (a.copy() for a in edge_points())
    p[SPOILED], n[SPOILED] = np.array(sp, F), np.array(sn, F)
    return (plain, under)[which], p, n


@functools.lru_cache(maxsize=None)
def edge_oracle(O, which):
    """dl_answer of the unspoiled edge launch under light list `which` at 16 samples."""
    scene, lists = edge_scene()[0], edge_scene()[1:]
    p, n = edge_points()
    return dl_answer(O, scene, lists[which], p, n, 16, 0, 0.0, DL.LO, DL.HI)


def degenerate_scene():
    """edge_scene()'s objects with a fourth quad whose edges are both zero, at the origin corner (1, 0.25, -1): (Scene, lights) -- the
    degenerate quad last in both."""
    scene, lights, _ = edge_scene()
    pool = lambda arr, k: [type(arr[0]).from_buffer_copy(arr[i]) for i in range(k)]
    quads = [R.Quad(q) for q in pool(scene._quads, scene.pod.n_quads)] + [R.Quad.new((1.0, 0.25, -1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]
    return R.Scene([R.Sphere(s) for s in pool(scene._spheres, scene.n_spheres)], quads=quads), lights[:2] + [(R.LIGHT_QUAD, 3)]


def same_or_nan(got, want):
    """Elementwise: the same bits -- the sign of a zero included --, or a NaN in both (its payload and sign may differ between x86 and the
    GPU: IEEE 754 leaves them open)."""
    return QE.same_nan(got, want)


# ---- 7. state between calls ---------------------------------------------------------------------------------------------------------------------
MOVED_TO = (-1.6, 1.9, -3.2)


def geom_with_its_sphere_light_moved():
    """geom_scene() with sphere 2 -- the sphere light of DL.GEOM_LIGHTS -- at another place: the same (kind, index) names another light."""
    g = geom_scene()
    sp = [R.Sphere(R.RtwSphere.from_buffer_copy(g._spheres[k])) for k in range(g.n_spheres)]
    sp[2] = R.Sphere.new(MOVED_TO, 0.4, (0.5, 0.5, 0.5), R.GLASS_M)
    scene = R.Scene(sp, triangles=[g.triangles[i] for i in range(g.n_triangles)])
    pool = lambda arr, k: [type(arr[0]).from_buffer_copy(arr[i]) for i in range(k)]
    scene._install_geom(pool(g._quads, g.pod.n_quads), pool(g._instances, g.pod.n_instances), pool(g._inst_spheres, g.pod.n_inst_spheres),
                        pool(g._inst_quads, g.pod.n_inst_quads))
    return scene


# ---- 6. the sum's association ------------------------------------------------------------------------------------------------------------------
ASSOC_SAMPLES = (1024, 128, 64)


def ascending_sum(w):
    """A plain ascending f32 sum of one item's weights, times 1 / samples."""
    s = F(0.0)
    for x in np.asarray(w, F):
        s = F(s + x)
    return F(s * (F(1.0) / F(len(w))))


def round_major_sum(w):
    """All of round 0 by the halving tree, then round 1 added, ...: the tree inside a round, the rounds outside."""
    w = np.asarray(w, F)
    L = min(len(w), 64)
    total = F(0.0)
    for k in range(0, len(w), L):
        s = w[k:k + L].copy()
        off = L // 2
        while off:
            s[:off] = (s[:off] + s[off:2 * off]).astype(F)
            off //= 2
        total = F(total + s[0])
    return F(total * (F(1.0) / F(len(w))))
