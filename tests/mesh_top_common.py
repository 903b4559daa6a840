"""Inputs of the top-level tree's tests (tests/test_mesh_top_cpu.py, tests/test_gpu_mesh_top.py): grids of placements, the rays aimed at them,
and the float64 image of the mesh under a placement -- where the geometry stands for a ray."""
import numpy as np

import rtw_amd as R
from tests import mesh_inst_common as M
from tests import quat_common as QC

F = np.float32
NEVER = 4294967295                                   # OPT_MESH_LIST_MAX: never the top-level tree
SIZES = (1, 2, 5, 64, 1024)


def grid(g, seed=5, offset=(0.0, 0.0, 0.0), general=True):
    """g x g placements, spacing 3.0, centred at z = 6 (+ offset), y jittered in +-0.8, a general un-normalised quaternion each (seeded)."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(g):
        for i in range(g):
            pos = np.array([3.0 * (i - (g - 1) / 2), rng.uniform(-0.8, 0.8), 6.0 + 3.0 * (j - (g - 1) / 2)]) + np.asarray(offset, np.float64)
            q = rng.normal(size=4) * rng.uniform(0.3, 3.0)
            out.append((pos.astype(F).tolist(), q.astype(F).tolist() if general else [1.0, 0.0, 0.0, 0.0]))
    return out


_CACHE = {}


def grid_case(g):
    """(mesh, placements, rays, the host list form's answer) of the g x g grid with 4096 rays, computed once."""
    if g not in _CACHE:
        T, pl = M.standard_mesh(), grid(g)
        rays = M.standard_rays(placements=pl)
        _CACHE[g] = (T, pl, rays, R.mesh_instance_hits(T.pods(), pl, rays, M.MINT, M.MAXT))
    return _CACHE[g]


def ordinary(rays):
    """Rays that pass tri_ray_ordinary in a placement's frame: finite (the standard rays are all within reach)."""
    return np.isfinite(rays).all(axis=1)


def vertices(T):
    """Every vertex of the mesh, [3 K][3] float64."""
    o, u, v = T.origin.astype(np.float64), T.u.astype(np.float64), T.v.astype(np.float64)
    return np.concatenate([o, o + u, o + v])


def rotate64(q, v):
    """(q (0, v) conj(q)).get_vec() in float64 for q [4], v [N][3]: exact products of the f32 components, no normalisation."""
    w, r = float(q[0]), np.asarray(q[1:], np.float64)
    return v * (w * w - r @ r) + 2.0 * np.outer(v @ r, r) + 2.0 * w * np.cross(r, v)


def placed64(placement, v, conj=True):
    """Where the mesh's points v stand in the world for a ray: conj(qn).rotate(v) + position, qn the f32 quaternion the device reads.
    conj=False: the q.rotate(v) + position of the hit record -- the wrong way for a box."""
    pos, quat = placement
    qn = QC.normalised(QC.f32(quat)).astype(np.float64)
    if conj:
        qn = qn * np.array([1.0, -1.0, -1.0, -1.0])
    return rotate64(qn, v) + np.asarray(QC.f32(pos), np.float64)
