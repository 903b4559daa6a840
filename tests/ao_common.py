"""Points, normals and references of the ambient-occlusion tests (tests/test_ao_cpu.py proves on the CPU, with the oracle, that each point
set exercises every outcome; tests/test_gpu_ao.py runs them through rtw_ctx_ambient_occlusion and rtw_ctx_ao_map).  Everything is
deterministic from fixed seeds, every helper of an existing module is imported from it, and every reference is computed once."""
import ctypes as C
import functools

import numpy as np

import rtw_amd as R
from tests import query_edges_common as QE
from tests.test_gpu_scene_hits import FORTY_MAXT, MAXT, MINT, TIME, forty_rays, forty_spheres, geom_rays, geom_scene, oracle_hits

F = np.float32
M32 = 0xFFFFFFFF
AO_STREAM = 0x414F5241
SAMPLES = 16
AO_MINT = 1e-3
N_RAYS = 512                                                 # camera rays per scene; the points are the hits among them


# ---- the rule, restated in Python integers ----------------------------------------------------------------------------------------------
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def point_base(seed, i):
    return mix32(mix32(mix32((seed + 0x9E3779B9) & M32) ^ AO_STREAM) ^ i)


def draws(base, k):
    """(xi_phi, xi_cos): the first two draws of the stream started at sample k."""
    state = mix32(base ^ k)
    inc = mix32(state ^ 0x85EBCA6B) | 1
    xi_phi = F(state >> 8) * F(1.0 / 16777216.0)
    state = (state * 747796405 + inc) & M32
    xi_cos = F(state >> 8) * F(1.0 / 16777216.0)
    return xi_phi, xi_cos


def skipped(normals):
    return np.all(np.asarray(normals, F).reshape(-1, 3) == 0.0, axis=1)


def rule_rays(points, normals, samples, seed, first=0):
    """rtw_ao_rays by the rule's text: the hash chain above fed to the existing rtw_mixed_dir(1.0, xi_phi, xi_cos, n), origin p; six zeros for
    the rays of a skipped point.  first: the index of points[0]."""
    p, n = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    out = np.zeros((len(p), samples, 6), F)
    skip = skipped(n)
    L = R.lib()
    d = (C.c_float * 3)()
    for i in range(len(p)):
        if skip[i]:
            continue
        base = point_base(seed, first + i)
        nn = (C.c_float * 3)(*[float(x) for x in n[i]])
        out[i, :, :3] = p[i]
        for k in range(samples):
            xi_phi, xi_cos = draws(base, k)
            assert L.rtw_mixed_dir(1.0, float(xi_phi), float(xi_cos), nn, d) == 0
            out[i, k, 3:] = d[0], d[1], d[2]
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def ao_of(counts, samples, skip=None):
    """The contract's right-hand side: (float)(samples - c) * (1.0f / samples), 1.0 for a skipped point."""
    ao = (F(samples) - np.asarray(counts).astype(F)) * (F(1.0) / F(samples))
    if skip is not None:
        ao = np.where(skip, F(1.0), ao)
    return ao.astype(F)


def random_points(n, seed):
    """n points in a box about the test scenes' objects with random unit normals."""
    rng = np.random.default_rng(seed)
    p = rng.uniform((-3.0, -1.5, -6.0), (3.0, 3.0, 0.0), (n, 3)).astype(F)
    v = rng.normal(size=(n, 3))
    return p, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


# ---- the point sets: name -> (scene, (t_begin, t_end), camera rays, time, mint, maxt of the camera rays, AO radius) -----------------------------
# The radii are chosen in tests/test_ao_cpu.py's terms: at them the oracle finds 20 % .. 80 % of the AO rays of "geom" and "field" occluded,
# at least 50 points partly occluded and at least 20 not at all.  (The normals face the viewer, so most of a hemisphere looks back at empty
# space: "geom" needs a radius that reaches the walls.  "forty" starts half of its camera rays inside a sphere: few of its points see nothing.)
RADIUS = {"geom": 5.0, "field": 2.0, "forty": 1.0}
CASES = ("geom", "field", "forty")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "geom":
        return geom_scene(), (0.0, 0.0), geom_rays(N_RAYS), 0.0, MINT, MAXT
    if name == "field":
        return QE.field_scene(), (0.0, 0.0), QE.ordinary_rays(N_RAYS, 3), 0.0, MINT, 1e30
    assert name == "forty", name
    scene = forty_spheres()
    return scene, (0.0, 1.0), forty_rays(scene, N_RAYS), TIME, MINT, FORTY_MAXT


def unit_f32(v):
    """v / sqrt(v.v) in f32, one rounding per operation."""
    v = np.asarray(v, F)
    l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(F) + v[:, 2] * v[:, 2]
    return (v / np.sqrt(l2.astype(F)).astype(F)[:, None]).astype(F)


@functools.lru_cache(maxsize=None)
def points_of(O, name):
    """(points, normals) f32: the oracle's hit points o + d * t of the case's camera rays (index >= 0), the normals unit(-d)."""
    scene, _, rays, time, mint, maxt = case(name)
    t, idx, _ = oracle_hits(O, scene, rays, time, mint, maxt)
    hit = idx >= 0
    o, d = rays[hit, :3], rays[hit, 3:]
    p = (o + (d * t[hit, None]).astype(F)).astype(F)
    return np.ascontiguousarray(p), np.ascontiguousarray(unit_f32(-d))


@functools.lru_cache(maxsize=None)
def reference(O, name, samples=SAMPLES, seed=0):
    """(counts [n], ao [n]) of the case's points from the oracle: ray [i][k] of ao_rays traced over [AO_MINT, RADIUS]."""
    scene, _, _, time, _, _ = case(name)
    p, n = points_of(O, name)
    rays = R.ao_rays(p, n, samples, seed)
    occ = oracle_hits(O, scene, rays.reshape(-1, 6), time, AO_MINT, RADIUS[name])[1] >= 0
    counts = occ.reshape(len(p), samples).sum(axis=1)
    return counts, ao_of(counts, samples)
