"""The rule, the scenes, the points and the references of the direct-lighting tests (tests/test_direct_light_cpu.py restates the rule and
proves on the CPU, with the oracle, that each point set exercises every outcome; tests/test_gpu_direct_light.py runs them through
rtw_ctx_direct_light and rtw_ctx_direct_light_map).  Everything is deterministic from fixed seeds, every helper of an existing module is
imported from it, and every reference is computed once."""
import functools

import numpy as np

import rtw_amd as R
from tests import ao_common as AO
from tests import lights_common as LC
from tests.test_gpu_scene_hits import FORTY_MAXT, MAXT, MINT, TIME, forty_rays, forty_spheres, geom_rays, geom_scene, oracle_hits

F = np.float32
M32 = 0xFFFFFFFF
STREAM = 0x4C495445
TWO_PI = F(6.2831855)
LO, HI = 1e-3, 1.0 - 1e-3
SAMPLES = 16
N_RAYS = 512                                                 # camera rays per scene; the points are the hits among them


# ---- the rule, restated in Python integers and numpy f32 (one rounding per operation) ------------------------------------------------------
def item_base(seed, i, l):
    return AO.mix32(AO.mix32(AO.mix32(AO.mix32((seed + 0x9E3779B9) & M32) ^ STREAM) ^ i) ^ (l + 1))


def draws(seed, i, l, samples):
    """(xi1 [samples], xi2 [samples]) of item (i, l)."""
    base = item_base(seed, i, l)
    xi = np.array([AO.draws(base, k) for k in range(samples)], F)
    return xi[:, 0], xi[:, 1]


def dot(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def cross(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.array([F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))], F)


def geometry(scene, light):
    """("quad", o, u, v) or ("sphere", c, r) of light (kind, index) of `scene`."""
    kind, index = light
    if kind == R.LIGHT_QUAD:
        q = scene._quads[index]
        return "quad", np.array(list(q.origin), F), np.array(list(q.u), F), np.array(list(q.v), F)
    s = scene._spheres[index]
    return "sphere", np.array(list(s.center), F), F(s.radius)


def rule_item(geom, p, n, xi1, xi2):
    """(d [samples][3], G [samples], cast [samples]) of one item by the rule's text."""
    p, n = np.asarray(p, F), np.asarray(n, F)
    with np.errstate(all="ignore"):
        if geom[0] == "quad":
            _, o, u, v = geom
            y = ((o[None, :] + (u[None, :] * xi1[:, None]).astype(F)).astype(F) + (v[None, :] * xi2[:, None]).astype(F)).astype(F)
            d = (y - p[None, :]).astype(F)
            num = (dot(n[None, :], d) * np.abs(dot(cross(u, v)[None, :], d))).astype(F)
        else:
            _, c, r = geom
            z = (F(1.0) - (F(2.0) * xi1).astype(F)).astype(F)
            s = np.sqrt((F(1.0) - (z * z).astype(F)).astype(F)).astype(F)
            phi = (TWO_PI * xi2).astype(F)
            w = np.stack([(s * R.cos_plain(phi)).astype(F), (s * R.sin_plain(phi)).astype(F), z], 1).astype(F)
            flip = dot(w, (p - c).astype(F)[None, :]) < F(0.0)
            w = np.where(flip[:, None], -w, w).astype(F)
            y = (c[None, :] + (w * r).astype(F)).astype(F)
            d = (y - p[None, :]).astype(F)
            m = (-dot(w, d)).astype(F)
            cl = np.where(m > F(0.0), m, F(0.0)).astype(F)
            num = ((dot(n[None, :], d) * cl).astype(F) * F(TWO_PI * F(r * r))).astype(F)
        dd = dot(d, d)
        G = (num / (dd * dd).astype(F)).astype(F)
        cast = (dot(n[None, :], d) > F(0.0)) & bool(np.any(n != 0.0))
    return d, G, cast


def rule_samples(scene, lights, points, normals, samples, seed, first=0, first_light=0):
    """rtw_light_samples by the rule's text: (rays [n][n_lights][samples][6], weights [n][n_lights][samples]); six zeros and the weight 0 for
    a sample that is not cast.  first / first_light: the index of points[0] / of lights[0] in the list the stream sees."""
    p, n = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    rays = np.zeros((len(p), len(lights), samples, 6), F)
    wts = np.zeros((len(p), len(lights), samples), F)
    geoms = [geometry(scene, l) for l in lights]
    for i in range(len(p)):
        for l, g in enumerate(geoms):
            xi1, xi2 = draws(seed, first + i, first_light + l, samples)
            d, G, cast = rule_item(g, p[i], n[i], xi1, xi2)
            rays[i, l, cast, :3] = p[i]
            rays[i, l, cast, 3:] = d[cast]
            wts[i, l, cast] = G[cast]
    return rays, wts


def rule_reduce(w):
    """rtw_light_reduce of one item's weights by the association's text."""
    w = np.asarray(w, F)
    samples = len(w)
    L = min(samples, 64)
    s = np.zeros(L, F)
    for k in range(0, samples, L):                           # rounds ascending: lane g adds w[g + k]
        s = (s + w[k:k + L]).astype(F)
    off = L // 2
    while off:
        s[:off] = (s[:off] + s[off:2 * off]).astype(F)
        off //= 2
    return F(s[0] * (F(1.0) / F(samples)))


same = AO.same


def cast_mask(rays):
    """A ray of rtw_light_samples is all zeros exactly when its sample is not cast (a cast ray has dot(n, d) > 0: a direction that is not 0)."""
    return np.any(np.asarray(rays)[..., 3:] != 0.0, axis=-1)


def outputs(weights, cast, occluded, samples):
    """(vis, irr, v) of the contract from the host weights, the cast mask and the occlusion answers of the cast rays ([...][samples] each)."""
    free = cast & ~occluded
    v = free.sum(axis=-1)
    vis = (v.astype(F) * (F(1.0) / F(samples))).astype(F)
    irr = R.light_reduce(np.where(free, weights, F(0.0)).astype(F))
    return vis, irr, v


# ---- the scenes: name -> (scene, lights, (t_begin, t_end), camera rays, time, mint, maxt of the camera rays) --------------------------------
CASES = ("golden", "geom", "forty")


def golden_with_occluders():
    """The golden light scene (a box with a small quad light and a small sphere light near its far end) with a field of small spheres between
    the camera and the lights and two quads that shade parts of the walls: (Scene, lights)."""
    ls, g = LC.golden()
    rng = np.random.default_rng(21)
    sp = list(g["spheres"])
    for _ in range(24):
        sp.append({"origin": [float(rng.uniform(-1.6, 1.6)), float(rng.uniform(-1.6, 1.6)), float(rng.uniform(2.6, 4.1))],
                   "radius": float(rng.uniform(0.15, 0.4)), "material": "lambertian", "color": [0.7, 0.7, 0.7], "emitted": [0.0, 0.0, 0.0]})
    quads = list(g["quads"]) + [
        {"origin": [-2.0, -0.6, 4.9], "u": [1.2, 0.0, 0.0], "v": [0.0, 0.0, 1.0], "material": "lambertian", "color": [0.5, 0.5, 0.5], "emitted": [0.0, 0.0, 0.0]},
        {"origin": [0.6, -2.0, 5.2], "u": [0.0, 1.5, 0.0], "v": [0.9, 0.0, 0.6], "material": "lambertian", "color": [0.5, 0.5, 0.5], "emitted": [0.0, 0.0, 0.0]}]
    return LC.LightScene(sp, quads, ls.lights, g["background"]).scene, list(ls.lights)


def golden_rays(n=N_RAYS, seed=3):
    """From the golden camera's place into the box: a cone that covers the far wall and the side walls."""
    rng = np.random.default_rng(seed)
    rays = np.empty((n, 6), F)
    for k in range(n):
        o = rng.uniform(-0.1, 0.1, 3)
        target = np.array([rng.uniform(-2.6, 2.6), rng.uniform(-2.6, 2.6), 6.0])
        d = target - o
        rays[k, :3], rays[k, 3:] = o, d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
    return rays


GEOM_LIGHTS = [(R.LIGHT_QUAD, 1), (R.LIGHT_SPHERE, 2)]        # geom_scene()'s floor quad and its glass sphere, up and to the left
FORTY_LIGHTS = [(R.LIGHT_SPHERE, 38), (R.LIGHT_SPHERE, 20)]  # two spheres of forty_spheres() that stand still (k % 4 != 1): one far from most
                                                             # points, and the one half of the camera rays start in


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "golden":
        scene, lights = golden_with_occluders()
        return scene, lights, (0.0, 0.0), golden_rays(), 0.0, MINT, MAXT
    if name == "geom":
        return geom_scene(), GEOM_LIGHTS, (0.0, 0.0), geom_rays(N_RAYS), 0.0, MINT, MAXT
    assert name == "forty", name
    scene = forty_spheres()
    return scene, FORTY_LIGHTS, (0.0, 1.0), forty_rays(scene, N_RAYS), TIME, MINT, FORTY_MAXT


@functools.lru_cache(maxsize=None)
def points_of(O, name):
    """(points, normals) f32: the oracle's hit points o + d * t of the case's camera rays (index >= 0) with the oracle's normals there, faced
    towards the viewer."""
    scene, _, _, rays, time, mint, maxt = case(name)
    t, idx, nrm = oracle_hits(O, scene, rays, time, mint, maxt)
    hit = idx >= 0
    o, d, n = rays[hit, :3], rays[hit, 3:], nrm[hit]
    p = (o + (d * t[hit, None]).astype(F)).astype(F)
    away = dot(d, n) > F(0.0)
    return np.ascontiguousarray(p), np.ascontiguousarray(np.where(away[:, None], -n, n).astype(F))


@functools.lru_cache(maxsize=None)
def reference(O, name, samples=SAMPLES, seed=0):
    """(vis [n][n_lights], irr, v, cast counts [n][n_lights]) of the case's points from the oracle: every cast ray of light_samples traced
    over [LO, HI]."""
    scene, lights, _, _, time, _, _ = case(name)
    p, n = points_of(O, name)
    rays, w = R.light_samples(scene, lights, p, n, samples, seed)
    cast = cast_mask(rays)
    occ = np.zeros(cast.shape, bool)
    occ[cast] = oracle_hits(O, scene, rays[cast], time, LO, HI)[1] >= 0
    vis, irr, v = outputs(w, cast, occ, samples)
    return vis, irr, v, cast.sum(axis=-1)
