"""Scenes, rays and point pairs of the any-hit tests (tests/test_occluded_cpu.py proves on the CPU, with the oracle and the existing host
forms, that each set exercises both outcomes; tests/test_gpu_occluded.py runs them through rtw_ctx_scene_occluded).  Everything is
deterministic from fixed seeds, every helper of an existing module is imported from it, and every reference is computed once."""
import functools

import numpy as np

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import mesh_top_common as MT
from tests import query_edges_common as QE
from tests import refit_common as RC
from tests.test_gpu_scene_hits import FORTY_MAXT, MAXT, MINT, TIME, forty_rays, forty_spheres, geom_rays, geom_scene, oracle_hits

F = np.float32
N = 1024
FIELD_MAXT = 1e30
SHORT_MAXT = 4.0


def occluded_of(idx):
    """The contract's right-hand side: an index >= 0."""
    return np.asarray(idx).reshape(-1) >= 0


def share(occ):
    return float(np.mean(np.asarray(occ, bool)))


def assert_same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want, bool).reshape(-1)
    assert got.dtype == np.bool_ and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


# ---- whole scenes: name -> (scene, (t_begin, t_end), rays, time, mint, maxt) -----------------------------------------------------------------
def _pool(arr, n):
    return [type(arr[0]).from_buffer_copy(arr[i]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def sub_scene(group):
    """geom_scene() with one group's own records alone: "spheres", "quads", "instances" or "triangles"."""
    g = geom_scene()
    if group == "spheres":
        return R.Scene(_pool(g._spheres, g.n_spheres))
    if group == "triangles":
        return R.Scene((), triangles=[g.triangles[i] for i in range(g.n_triangles)])
    scene = R.Scene(())
    if group == "quads":
        scene._install_geom(_pool(g._quads, g.pod.n_quads), [], [], [])
    else:
        scene._install_geom([], _pool(g._instances, g.pod.n_instances), _pool(g._inst_spheres, g.pod.n_inst_spheres),
                            _pool(g._inst_quads, g.pod.n_inst_quads))
    return scene


GROUPS = ("spheres", "quads", "instances", "triangles")


@functools.lru_cache(maxsize=None)
def scene_case(name):
    if name == "geom":
        return geom_scene(), (0.0, 0.0), geom_rays(N), 0.0, MINT, MAXT
    if name == "geom+medium":
        return geom_scene(medium=True), (0.0, 0.0), geom_rays(N), 0.0, MINT, MAXT
    if name in ("forty", "forty+duplicate"):
        scene = forty_spheres(duplicate=name != "forty")
        return scene, (0.0, 1.0), forty_rays(scene, N), TIME, MINT, FORTY_MAXT
    if name == "field":
        return QE.field_scene(), (0.0, 0.0), QE.ordinary_rays(N, 3), 0.0, MINT, FIELD_MAXT
    if name == "field, short range":
        return QE.field_scene(), (0.0, 0.0), QE.ordinary_rays(N, 3), 0.0, MINT, SHORT_MAXT
    assert name in GROUPS, name
    return sub_scene(name), (0.0, 0.0), geom_rays(N), 0.0, MINT, MAXT


FULL_SCENES = ("geom", "geom+medium", "forty", "forty+duplicate", "field")
SCENES = FULL_SCENES + ("field, short range",) + GROUPS


@functools.lru_cache(maxsize=None)
def scene_reference(O, name):
    """The oracle's occluded bit of every ray of a case.  (The oracle traces a constant-density instance, which the queries skip: the scene with
    the fog answers what the scene without it answers.)"""
    if name == "geom+medium":
        return scene_reference(O, "geom")
    scene, _, rays, time, mint, maxt = scene_case(name)
    return occluded_of(oracle_hits(O, scene, rays, time, mint, maxt)[1])


# ---- point pairs: from about the eye to points behind the field's objects ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def segment_pairs(n=512, seed=43):
    """(p [n][3], q [n][3]) f32: p about the eye of field_scene(), q behind its objects -- half beyond a sphere's centre as seen from p, half
    just in front of the back wall and in the sky about it."""
    scene = QE.field_scene()
    rng = np.random.default_rng(seed)
    p, q = np.empty((n, 3), F), np.empty((n, 3), F)
    for k in range(n):
        o = QE.EYE + rng.uniform(-0.2, 0.2, 3)
        if k % 2 == 0:
            c = QE.centre_of(scene, int(rng.integers(0, scene.n_spheres))) + rng.normal(0, 0.25, 3)
            far = o + (c - o) * rng.uniform(1.3, 1.8)
        else:
            far = np.array([rng.uniform(-5.5, 5.5), rng.uniform(-3.5, 5.5), -5.9])
        p[k], q[k] = o, far
    return p, q


def segment_rays(p, q):
    """The rays of segments_occluded by hand: (p, q - p), one f32 subtraction per component."""
    p, q = np.asarray(p, F).reshape(-1, 3), np.asarray(q, F).reshape(-1, 3)
    return np.concatenate([p, (q - p).astype(F)], 1)


SEG_LO, SEG_HI = 1e-3, 1.0 - 1e-3


# ---- triangles alone --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_triangles(name):
    v, f, _, _ = RC.mesh(name)
    return tuple(RC.triangles_of(v, f)), v, f


def mesh_rays(v, f, n=N, seed=7):
    """Rays about a mesh (vertices v, faces f): aimed at points of its triangles from outside its box, deliberate misses, exactly-zero direction
    components through it, rays tri_ray_ordinary refuses (an origin beyond 2^40: they walk the list), NaN rays and a zero direction."""
    rng = np.random.default_rng(seed)
    v = np.asarray(v, np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) + 1.0
    rays = np.empty((n, 6), np.float64)
    for k in range(n):
        tri = v[np.asarray(f[int(rng.integers(0, len(f)))])]
        w = rng.dirichlet((1.0, 1.0, 1.0))
        target = w @ tri
        kind = k % 8
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if kind < 4:                                           # aimed from outside
            o = centre + size * u
            d = (target - o) * rng.uniform(0.2, 2.0)
        elif kind < 6:                                         # away from the mesh
            o = centre + size * u
            d = u * rng.uniform(0.5, 2.0) + rng.normal(scale=0.1, size=3)
        elif kind == 6:                                        # one or two exactly-zero direction components, through a point of the mesh
            axis = int(rng.integers(0, 3))
            d = np.zeros(3)
            d[axis] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
            o = target - d * size
            if rng.integers(0, 2):
                o[(axis + 1) % 3] += rng.normal(scale=0.3)
        else:                                                  # refused by tri_ray_ordinary: 2^41 away, aimed back at the mesh
            o = target + u * 2.0 ** 41
            d = -u
        rays[k, :3], rays[k, 3:] = o, d
    rays = rays.astype(F)
    rays[-4] = [centre[0], centre[1], centre[2] + size, np.nan, 0.0, -1.0]
    rays[-3] = [np.nan, centre[1], centre[2] + size, 0.0, 0.0, -1.0]
    rays[-2, 3:] = np.nan
    rays[-1, 3:] = 0.0
    return rays


# ---- placements ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def placement_case(name):
    """(mesh pods, placements, rays): "standard", "grid8", "grid32", "coincident32", "far" (a position of 1e5), "refused" (rays
    mesh_top_ray_ordinary refuses among the grid's: origins beyond 2^38, NaN rays, zero directions)."""
    T = MI.standard_mesh()
    if name == "standard":
        pl = MI.standard_placements()
    elif name in ("grid8", "refused"):
        pl = MT.grid(8)
    elif name == "grid32":
        pl = MT.grid(32)
    elif name == "coincident32":
        pl = [([0.5, 0.2, 4.0], [1.0, 0.0, 0.0, 0.0])] * 32
    else:
        assert name == "far", name
        pl = [([1e5, 0.5, -1e5], [0.6, 0.2, -1.4, 0.9]), ([1e5 + 2.5, 0.0, -1e5], [1.0, 0.0, 0.0, 0.0])]
    rays = MI.standard_rays(pl, n=N)
    if name == "refused":
        rng = np.random.default_rng(3)
        for k in range(0, N, 4):                               # every fourth ray: the same line from 2^39 further back, a NaN, or no direction
            d = rays[k, 3:].astype(np.float64)
            if not np.isfinite(d).all() or not d.any():
                continue
            kind = (k // 4) % 3
            if kind == 0:
                rays[k, :3] = (rays[k, :3].astype(np.float64) - d / np.abs(d).max() * 2.0 ** 39).astype(F)
            elif kind == 1:
                rays[k, int(rng.integers(0, 6))] = np.nan
            else:
                rays[k, 3:] = 0.0
    return tuple(T.pods()), pl, rays


PLACEMENTS = ("standard", "grid8", "grid32", "coincident32", "far", "refused")


@functools.lru_cache(maxsize=None)
def placement_reference(name):
    """The host list walk's occluded bit (rtw_mesh_instance_hits: existing code)."""
    pods, pl, rays = placement_case(name)
    return occluded_of(R.mesh_instance_hits(list(pods), pl, rays, MI.MINT, MI.MAXT, normals=False)[1])
