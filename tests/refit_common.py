"""What the refit tests share (tests/test_refit_cpu.py, tests/test_gpu_refit.py): the meshes, the deformations of their vertices, a numpy
float64 restatement of a triangle's inflated box with np.nextafter as the outward rounding, and the nodes a refit must write.

The restatement follows rtw_refit.h's tri_box operation by operation -- float64 +, *, /, sqrt are IEEE in numpy as in C++ --, so the
comparison is on the bits: there is no tolerance in these tests."""
import numpy as np

import rtw_amd as R

F = np.float32
D = np.float64


# ---- meshes: name -> (vertices [k][3] f32, faces [n][3]), and the tree the builder gives them (nodes, depth) ---------------------------------
def row(k):
    """k separate triangles along x."""
    v = []
    for i in range(k):
        v += [(2.0 * i, 0.0, 0.0), (2.0 * i + 1.0, 0.0, 0.0), (2.0 * i, 1.0, 0.5)]
    return np.array(v, F), np.arange(3 * k).reshape(k, 3)


def coincident(k=33):
    """The same triangle k times: no split separates anything, the builder falls back to the median."""
    return np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.25)], F), np.tile(np.arange(3), (k, 1))


def uneven(k=40):
    """Triangle j at x = 1.6^j, of size 0.1 x: SAH peels the far ones off one by one, the leaves lie at very uneven depths."""
    v = []
    for j in range(k):
        x = 1.6 ** j
        v += [(x, 0.0, 0.0), (1.1 * x, 0.0, 0.0), (x, 0.1 * x, 0.0)]
    return np.array(v, F), np.arange(3 * k).reshape(k, 3)


MESHES = {
    "row1": (lambda: row(1), 1, 1, 0),
    "row4": (lambda: row(4), 4, 1, 0),
    "row5": (lambda: row(5), 5, 3, 1),
    "icosphere1": (lambda: R.mesh_icosphere(1), 80, 55, 5),
    "icosphere2": (lambda: R.mesh_icosphere(2), 320, 209, 8),
    "terrain12": (lambda: R.mesh_terrain(12), 288, 175, 7),
    "coincident33": (coincident, 33, 17, 4),
    "uneven40": (uneven, 40, 27, 13),
}


def mesh(name):
    """(vertices, faces, nodes, depth) of a mesh of the table."""
    make, n, nodes, depth = MESHES[name]
    v, f = make()
    assert len(f) == n
    return v, f, nodes, depth


# ---- deformations of a vertex array: name -> (function of (vertices, faces), list_walk of the deformed mesh) -----------------------------------
A = np.array([[3.0, 0.5, 0.0], [0.0, 1.0, 0.25], [0.0, 0.0, 0.5]], D)


def sine_wave(v, f):
    w = v.astype(D) @ A.T + np.array([5.0, -2.0, 1.0])
    w[:, 1] += 0.3 * np.sin(4.0 * w[:, 0])
    return w.astype(F)


def degenerate(v, f):
    w = v.copy()
    w[f[7][2]] = w[f[7][1]]
    return w


def far_vertex(v, f):
    w = v.copy()
    w[0, 0] = F(2.0 ** 41)
    return w


def flat(v, f):
    w = v.copy()
    w[:, 2] = (w[:, 2].astype(D) * 1e-3).astype(F)
    return w


DEFORMATIONS = {"sine_wave": (sine_wave, 0), "degenerate": (degenerate, 1), "far_vertex": (far_vertex, 1), "flat": (flat, 1)}


# ---- the inflated box, restated ----------------------------------------------------------------------------------------------------------------
def tri_boxes(ouv):
    """(lo [n][3], hi [n][3]) float64 of every triangle of ouv [n][9] f32: rtw_refit.h's tri_box for triangles it accepts."""
    a = np.asarray(ouv, F).reshape(-1, 9)
    o, u, v = a[:, 0:3].astype(D), a[:, 3:6].astype(D), a[:, 6:9].astype(D)
    p, q = o + u, o + v
    lo, hi = np.minimum(o, np.minimum(p, q)), np.maximum(o, np.maximum(p, q))
    amax = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1)
    lu = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
    lv = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    nl = np.sqrt(nx * nx + ny * ny + nz * nz)
    e = np.maximum(lu, lv)
    assert (nl > 0.0).all() and (amax <= 2.0 ** 40).all(), "the restatement covers triangles the tree accepts"
    kappa = e * e / nl
    assert (kappa <= 256.0).all()
    r = 2.0 ** -24 * (256.0 * amax + 4096.0 * kappa * (1.0 + kappa) * e) + 2.0 ** -100
    return lo - r[:, None], hi + r[:, None]


def down(x):
    """The largest f32 <= x."""
    f = np.asarray(x, D).astype(F)
    return np.where(f.astype(D) > x, np.nextafter(f, F(-np.inf)), f).astype(F)


def up(x):
    """The smallest f32 >= x."""
    f = np.asarray(x, D).astype(F)
    return np.where(f.astype(D) < x, np.nextafter(f, F(np.inf)), f).astype(F)


def expected_nodes(dump, order, ouv):
    """The nodes a refit to `ouv` must leave: `dump`'s skip and leaf words, and for every node the outward rounding of the float64 union of
    the inflated boxes of the triangles of its subtree -- the leaf slots of the leaves in [node, skip), `order` naming their triangles."""
    lo, hi = tri_boxes(ouv)
    out = dump.copy()
    n = len(dump)
    first = np.where(dump["leaf"] != 0, dump["leaf"] >> 3, 0).astype(np.int64)
    count = (dump["leaf"] & 7).astype(np.int64)
    for i in range(n):
        leaves = [j for j in range(i, int(dump["skip"][i])) if dump["leaf"][j]]
        slots = np.concatenate([np.arange(first[j], first[j] + count[j]) for j in leaves])
        t = np.asarray(order)[slots]
        out["lo"][i] = down(lo[t].min(axis=0))
        out["hi"][i] = up(hi[t].max(axis=0))
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def triangles_of(v, f):
    """The mesh as set_triangles takes it, two materials in turn (a refit must leave them alone)."""
    tris = list(R.Triangle.from_mesh(v, f, mat=R.SCATTER_M, color=(0.3, 0.7, 0.4)))
    for k in range(1, len(tris), 3):
        tris[k] = R.Triangle.new(tris[k].pod.origin, tris[k].pod.u, tris[k].pod.v, R.METALLIC_M, (0.9, 0.8, 0.7))
    return tris
