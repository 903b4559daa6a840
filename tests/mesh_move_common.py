"""What the tests of moving placements share (tests/test_mesh_move_cpu.py, tests/test_gpu_mesh_move.py): the placement lists, the motions in
float32, and a numpy float64 restatement of a placement's world box and of the nodes a refit of the top-level tree must write.

The restatement is DESIGN.md 4.11's rule ("Boxes", "The bound"): the eight corners of the mesh tree's root box turned by C(v) = conj(qn) (0, v) qn
in float64 -- v (w^2 - r.r) + 2 r (r.v) + 2 w (r x v) with r = -(x, y, z) --, plus the position, padded by 512 u (|position|_inf + rho) + 2^-40 of
the box's largest coordinate + 2^-100, rounded outward with np.nextafter; a node's box is the union over the placements of its subtree, read from
the skip links.  float64 +, * and sqrt are IEEE in numpy as in C++, so every comparison is on the bits: there is no tolerance in these tests."""
import numpy as np

import rtw_amd as R
from tests import mesh_inst_common as MI
from tests import mesh_top_common as MT
from tests import quat_common as QC
from tests.refit_common import down, up

F = np.float32
D = np.float64
REACH = 2.0 ** 38


# ---- placement lists -------------------------------------------------------------------------------------------------------------------------
def one_triangle():
    return MI.TriSet([{"origin": [0.0, 0.0, 0.0], "u": [1.0, 0.0, 0.0], "v": [0.0, 1.0, 0.0], "material": "lambertian", "color": [0.5, 0.5, 0.5],
                       "emitted": [0.0, 0.0, 0.0]}])


def outlier_chain(n=20):
    """Identity placements of a one-triangle mesh at x = 4^k: 2 n - 7 nodes, leaves at very uneven depths."""
    return one_triangle(), [([4.0 ** k, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]) for k in range(n)]


def coincident(n=32):
    """n coincident placements of the standard mesh: no split separates anything, the builder falls back to the median."""
    return MI.standard_mesh(), [([0.5, 0.2, 4.0], [1.0, 0.0, 0.0, 0.0])] * n


def grid_n(n):
    """The first n placements of the 32 x 32 grid of tests/mesh_top_common.py (general, un-normalised quaternions)."""
    return MT.grid(32)[:n]


def cases():
    """name -> (mesh, placements): the sizes 1, 2, 5, 64 and 1024, the chain of outliers and the coincident placements."""
    out = {f"grid{n}": (MI.standard_mesh(), grid_n(n)) for n in MT.SIZES}
    out["outliers20"] = outlier_chain()
    out["coincident32"] = coincident()
    return out


def as_array(placements):
    """[n][7] float32 = position, (w, x, y, z)."""
    return np.array([list(p) + list(q) for p, q in placements], F).reshape(-1, 7)


def as_list(poses):
    return [(p[:3].tolist(), p[3:].tolist()) for p in np.asarray(poses, F).reshape(-1, 7)]


# ---- the motions, in float32: name -> function of the [n][7] array -------------------------------------------------------------------------------
PITCH = 3.0                                                     # the grid's spacing (mesh_top_common.grid)


def hamilton(a, b):
    """Quaternion::hamilton in f32, a and b [n][4] = w, x, y, z."""
    aw, ax, ay, az = (a[:, k] for k in range(4))
    bw, bx, by, bz = (b[:, k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1).astype(F)


def turn_and_shift(poses, seed=23):
    """Every placement turned by a random quaternion and shifted by a third of the grid pitch in a random direction."""
    rng = np.random.default_rng(seed)
    out = np.array(poses, F).reshape(-1, 7)
    d = rng.normal(size=(len(out), 3))
    out[:, :3] = (out[:, :3] + (PITCH / 3.0) * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    out[:, 3:] = hamilton(rng.normal(size=(len(out), 4)).astype(F), out[:, 3:])
    return out


def permute(poses, seed=29):
    """The poses permuted at random among the placements: what a refit handles worst."""
    out = np.array(poses, F).reshape(-1, 7)
    return out[np.random.default_rng(seed).permutation(len(out))].copy()


def identity(poses):
    return np.array(poses, F).reshape(-1, 7)


def shrink_to_a_point(poses):
    """Every placement at the first one's position, its quaternion kept."""
    out = np.array(poses, F).reshape(-1, 7)
    out[:, :3] = out[0, :3]
    return out


MOTIONS = {"turn_and_shift": turn_and_shift, "permute": permute, "identity": identity, "shrink_to_a_point": shrink_to_a_point}


# ---- invalid poses ---------------------------------------------------------------------------------------------------------------------------
def spoil(poses, where):
    """The list with an invalid pose at each index of `where`: a NaN position, an inf quaternion component and a zero quaternion in turn."""
    out = np.array(poses, F).reshape(-1, 7)
    for j, k in enumerate(where):
        if j % 3 == 0:
            out[k, 1] = np.nan
        elif j % 3 == 1:
            out[k, 5] = np.inf
        else:
            out[k, 3:] = 0.0
    return out


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def rows_of(poses):
    """The rows a placement list gives: [n][8] f32 = quat_normalised(q) (q * (1.0 / q.len()), one rounding per operation), position, 0."""
    p = np.asarray(poses, F).reshape(-1, 7)
    q = p[:, 3:]
    with np.errstate(all="ignore"):
        ln = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(F) + q[:, 2] * q[:, 2]).astype(F) + q[:, 3] * q[:, 3]).astype(F)
        s = (F(1.0) / ln).astype(F)
    out = np.zeros((len(p), 8), F)
    out[:, :4] = (q * s[:, None]).astype(F)
    out[:, 4:7] = p[:, :3]
    return out


def placement_boxes(root, rows):
    """(lo [n][3], hi [n][3] float64, beyond [n] bool) of the placements `rows` ([n][8]) of a mesh whose tree's root is `root` (a TOP_NODE)."""
    rows = np.asarray(rows, F).reshape(-1, 8).astype(D)
    w, r, pos = rows[:, 0], -rows[:, 1:4], rows[:, 4:7]
    blo, bhi = np.asarray(root["lo"], D), np.asarray(root["hi"], D)
    lo, hi = np.full((len(rows), 3), np.inf), np.full((len(rows), 3), -np.inf)
    rho = np.zeros(len(rows))
    rr = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
    for c in range(8):
        v = np.array([bhi[k] if c >> k & 1 else blo[k] for k in range(3)], D)
        rho = np.maximum(rho, np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
        rv = r[:, 0] * v[0] + r[:, 1] * v[1] + r[:, 2] * v[2]
        cx = np.stack([r[:, 1] * v[2] - r[:, 2] * v[1], r[:, 2] * v[0] - r[:, 0] * v[2], r[:, 0] * v[1] - r[:, 1] * v[0]], 1)
        p = v[None, :] * (w * w - rr)[:, None] + 2.0 * r * rv[:, None] + (2.0 * w)[:, None] * cx + pos
        lo, hi = np.minimum(lo, p), np.maximum(hi, p)
    pmax = np.abs(pos).max(axis=1)
    pad = 2.0 ** -24 * 512.0 * (pmax + rho)
    amax = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1)
    slack = pad + 2.0 ** -40 * amax + 2.0 ** -100
    return lo - slack[:, None], hi + slack[:, None], ~(np.isfinite(rho) & (pmax <= REACH) & (rho <= REACH))


def expected_nodes(dump, order, root, rows):
    """The nodes a refit to `rows` must leave: `dump`'s skip and leaf words, and for every node the outward rounding of the float64 union of
    the world boxes of the placements of its subtree -- the leaf slots of the leaves in [node, skip), `order` naming their placements."""
    lo, hi, _ = placement_boxes(root, rows)
    out = dump.copy()
    first = np.where(dump["leaf"] != 0, dump["leaf"] >> 3, 0).astype(np.int64)
    count = (dump["leaf"] & 7).astype(np.int64)
    slots_of = [np.arange(first[j], first[j] + count[j]) for j in range(len(dump))]
    for i in range(len(dump)):
        leaves = [j for j in range(i, int(dump["skip"][i])) if dump["leaf"][j]]
        k = np.asarray(order)[np.concatenate([slots_of[j] for j in leaves])]
        out["lo"][i] = down(lo[k].min(axis=0))
        out["hi"][i] = up(hi[k].max(axis=0))
    return out


def heights(nodes):
    """The height of every node from the skip links: a leaf 0, an inner node 1 + its higher child (children: i + 1 and nodes[i + 1].skip)."""
    h = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes) - 1, -1, -1):
        if not nodes["leaf"][i]:
            h[i] = 1 + max(h[i + 1], h[int(nodes["skip"][i + 1])])
    return h


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sine_ouv(T):
    """The mesh T (a TriSet) under refit_common's sine wave: (ouv [k][9] f32, the moved mesh as a TriSet)."""
    from tests import refit_common as RC
    o, u, v = T.origin, T.u, T.v
    a, b, c = RC.sine_wave(o, None), RC.sine_wave((o + u).astype(F), None), RC.sine_wave((o + v).astype(F), None)
    ouv = np.ascontiguousarray(np.concatenate([a, (b - a).astype(F), (c - a).astype(F)], 1), F)
    tris = [dict(t, origin=ouv[k, 0:3].tolist(), u=ouv[k, 3:6].tolist(), v=ouv[k, 6:9].tolist()) for k, t in enumerate(T.tris)]
    return ouv, MI.TriSet(tris)


def scaled_mesh(T, s):
    """The mesh T scaled by s about the origin: (ouv, TriSet)."""
    ouv = np.ascontiguousarray(np.concatenate([T.origin * F(s), T.u * F(s), T.v * F(s)], 1), F)
    tris = [dict(t, origin=ouv[k, 0:3].tolist(), u=ouv[k, 3:6].tolist(), v=ouv[k, 6:9].tolist()) for k, t in enumerate(T.tris)]
    return ouv, MI.TriSet(tris)
