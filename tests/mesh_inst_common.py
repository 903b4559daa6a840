"""Restatement of mesh placements -- Rust2's `Instance` of triangles (Rust2/src/objects/instance.rs:215-255 around triangle.rs) -- in numpy
f32, one rounding per written operation: the reference of tests/test_mesh_instances_cpu.py and tests/test_gpu_mesh_instances.py.

    Triangle::new / get_hit                                     TriSet (derived fields as rtw_triangle_new forms them), TriSet.pick
    Instance::get_hit around the triangle group                 placement_hits
    the scene's closest hit over the four groups                MeshScene.closest (spheres, quads, quaternion instances: quat_common's)
    a RUST2 path on the oracle's random stream                  quat_common.trace over a MeshScene; render() here, for every sampler

The triangle group's rule -- closest in list order, a later triangle only when strictly closer: `best < 0 || bt > t` -- is evaluated without a
loop over the list: the winner is the FIRST triangle that attains the least t among those the test accepts, except that an accepted first
candidate whose t is NaN stays (nothing is `>` or `<` a NaN, so it is never replaced and a later NaN never replaces).  -0 and +0 compare
equal, so argmin keeps the first of them as the rule does."""
import numpy as np

import rtw_amd as R
from tests import lights_common as LC
from tests import quat_common as QC
from tests.quat_common import F, cross3, dot3, f32, normalised, rotate_n

MINT, MAXT = 1e-4, 1e4
N_RAYS = 4096


def same_nan(a, b):
    """Elementwise: the same bits, or a NaN in both (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_hits_equal(got, want, what):
    """(t, placement, triangle, normals) against the same: indices exactly, floats on the bits (NaN in both counts as equal)."""
    for name, g, w in zip(("t", "placement", "triangle", "normal"), got, want):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(~same_nan(g, w)) if name in ("t", "normal") else np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])


# ---- triangles ----------------------------------------------------------------------------------------------------------------------------
class TriSet:
    """K triangles {"origin", "u", "v"[, "material", "color", "emitted"]} with Triangle::new's derived fields (triangle.rs:35-49): n = u x v,
    normal = n / |n|, d = normal . origin, w = n / (n . n)."""

    def __init__(self, tris):
        self.tris = list(tris)
        self.k = len(self.tris)
        self.origin = f32([t["origin"] for t in self.tris]).reshape(-1, 3)
        self.u = f32([t["u"] for t in self.tris]).reshape(-1, 3)
        self.v = f32([t["v"] for t in self.tris]).reshape(-1, 3)
        n = cross3(self.u, self.v)
        nn = dot3(n, n)
        with np.errstate(all="ignore"):
            self.normal = (n / np.sqrt(nn)[:, None]).astype(F)
            self.w = (n / nn[:, None]).astype(F)
        self.d = dot3(self.normal, self.origin)

    def pods(self):
        return [R.Triangle.new(t["origin"], t["u"], t["v"], QC._mat(t) if "material" in t else None, t.get("color", (1.0, 1.0, 1.0)),
                               t.get("emitted")) for t in self.tris]

    def pick(self, o, d, mint, maxt):
        """get_hit (triangle.rs:95-124) of every triangle for rays o, d [N][3] and the group rule: (found [N], t [N], index [N] or -1)."""
        with np.errstate(all="ignore"):
            oo, dd = o[:, None, :], d[:, None, :]
            den = dot3(self.normal[None], dd)
            t = ((self.d[None] - dot3(self.normal[None], oo)) / den).astype(F)
            point = (oo + dd * t[..., None]).astype(F)
            planar = (point - self.origin[None]).astype(F)
            alfa = dot3(self.w[None], cross3(planar, np.broadcast_to(self.v[None], planar.shape)))
            beta = dot3(self.w[None], cross3(np.broadcast_to(self.u[None], planar.shape), planar))
            ok = ~(np.abs(den) <= F(1e-8)) & ~((t < F(mint)) | (t > F(maxt))) & ~((alfa < 0) | (beta < 0) | ((alfa + beta).astype(F) > 1))
        found = ok.any(axis=1)
        rows = np.arange(len(o))
        first = np.argmax(ok, axis=1)
        first_nan = found & np.isnan(t[rows, first])
        least = np.argmin(np.where(ok & ~np.isnan(t), t, F(np.inf)), axis=1)
        idx = np.where(first_nan, first, least)
        return found, np.where(found, t[rows, idx], F(0.0)).astype(F), np.where(found, idx, -1)


def placement_hits(T, placements, o, d, mint=MINT, maxt=MAXT):
    """The placement group: placements [(position, quat)] in list order, each by Instance::get_hit -- o' = q.rotate(o - position), d' =
    q.rotate(d), the triangle group there, t untouched --, a later placement only when strictly closer.  Dict of found, t, placement,
    triangle (-1), point = q.rotate(p') + position, normal = q.rotate(n') (0 on a miss), local = d' of the winner."""
    o, d = f32(o).reshape(-1, 3), f32(d).reshape(-1, 3)
    n = len(o)
    found, bt = np.zeros(n, bool), np.zeros(n, F)
    pl, tri = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    point, normal, local = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
    with np.errstate(all="ignore"):
        for k, (pos, quat) in enumerate(placements):
            qn, pos = normalised(f32(quat)), f32(pos)
            lo, ld = rotate_n(qn, (o - pos[None]).astype(F)), rotate_n(qn, d)
            f, t, j = T.pick(lo, ld, mint, maxt)
            take = f & (~found | (bt > t))
            if take.any():
                lp = (lo[take] + ld[take] * t[take, None]).astype(F)
                point[take] = (rotate_n(qn, lp) + pos[None]).astype(F)
                normal[take] = rotate_n(qn, T.normal[j[take]])
                local[take] = ld[take]
            found |= take
            bt = np.where(take, t, bt).astype(F)
            pl, tri = np.where(take, k, pl), np.where(take, j, tri)
    return {"found": found, "t": bt, "placement": pl, "triangle": tri, "point": point, "normal": normal, "local": local}


def as_outputs(h):
    """placement_hits' answer in the shape of rtw_mesh_instance_hits' outputs: (t, +inf on a miss; placement; triangle; normals)."""
    return (np.where(h["found"], h["t"], F(np.inf)).astype(F), h["placement"].astype(np.int32), h["triangle"].astype(np.int32), h["normal"])


# ---- the standard inputs ---------------------------------------------------------------------------------------------------------------------
MATERIALS = ("lambertian", "mirror", "glass")


def standard_mesh():
    """mesh_icosphere(1): 80 triangles, Lambertian, Mirror and MirrorGlass in turn, each with a colour of its own."""
    vtx, faces = R.mesh_icosphere(1)
    tris = []
    for k, (a, b, c) in enumerate(faces):
        col = [0.55 + 0.1 * (k % 4), 0.5 + 0.05 * (k % 7), 0.9 - 0.1 * (k % 5)]
        tris.append({"origin": vtx[a].tolist(), "u": (vtx[b] - vtx[a]).astype(F).tolist(), "v": (vtx[c] - vtx[a]).astype(F).tolist(),
                     "material": MATERIALS[k % 3], "color": col, "emitted": [0.0, 0.0, 0.0]})
    return TriSet(tris)


def standard_placements():
    """The identity; a pure translation; a turn of pi/4 about y plus a translation; an un-normalised general quaternion; and two coincident
    placements that overlap the third: the later of the pair never wins (a tie), the earlier replaces the third where it is strictly closer."""
    third = [0.4, 0.3, 3.2]
    pair = [1.1, 0.5, 2.9]
    return [([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]),
            ([3.0, 0.0, 0.5], [1.0, 0.0, 0.0, 0.0]),
            (third, QC.from_axis(np.pi / 4, (0.0, 1.0, 0.0)).tolist()),
            ([-3.0, 0.5, 1.0], [0.6, 0.2, -1.4, 0.9]),
            (pair, [1.0, 0.0, 0.0, 0.0]),
            (pair, [1.0, 0.0, 0.0, 0.0])]


def standard_rays(placements=None, n=N_RAYS, seed=17):
    """4096 rays [n][6]: aimed at the placements from outside, deliberate misses, origins inside a mesh, exactly-zero direction components
    (axis-parallel rays through the placements), and at the end a NaN ray and a zero direction.  Directions are not normalised."""
    placements = standard_placements() if placements is None else placements
    rng = np.random.default_rng(seed)
    centres = np.array([p[0] for p in placements], np.float64)
    rays = np.empty((n, 6), np.float64)
    for k in range(n):
        c = centres[k % len(centres)]
        kind = (k // len(centres)) % 8
        if kind in (0, 1, 2):                                  # aimed from outside
            o = c + 8.0 * QC.unit3(rng.normal(size=3).astype(F)).astype(np.float64)
            d = (c + rng.normal(scale=0.45, size=3) - o) * rng.uniform(0.2, 2.0)
        elif kind in (3, 4, 5):                                # a deliberate miss: away from every placement
            o = c + np.array([0.0, 6.0, 0.0]) + rng.normal(scale=0.5, size=3)
            d = np.array([rng.normal(), abs(rng.normal()) + 0.2, rng.normal()])
        elif kind == 6:                                        # from inside the mesh
            o = c + rng.uniform(-0.3, 0.3, 3)
            d = rng.normal(size=3) * rng.uniform(0.5, 1.5)
        else:                                                  # one or two exactly-zero direction components
            axis = int(rng.integers(0, 3))
            d = np.zeros(3)
            d[axis] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
            if rng.integers(0, 2):
                d[(axis + 1) % 3] = rng.normal(scale=0.05)
            o = c - 6.0 * d / np.linalg.norm(d) + rng.uniform(-0.7, 0.7, 3)
        rays[k, :3], rays[k, 3:] = o, d
    rays = rays.astype(F)
    rays[-2] = [0.0, 0.0, -5.0, np.nan, 0.0, 1.0]
    rays[-1] = [0.0, 0.0, -5.0, 0.0, 0.0, 0.0]
    return rays


def assert_input_quality(h, n_placements=6, later=5):
    """The conditions the issue puts on the standard rays, from the restatement's answer."""
    hit = float(h["found"].mean())
    assert 0.25 <= hit <= 0.75, f"{hit:.2%} of the rays hit: both outcomes must hold at least a quarter"
    wins = np.bincount(h["placement"][h["found"]], minlength=n_placements)
    assert wins[later] == 0, wins
    assert all(wins[k] >= 20 for k in range(n_placements) if k != later), wins


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------------
class MeshScene(QC.QuatScene):
    """quat_common.QuatScene plus the mesh `tris` (a TriSet) placed at `placements`: the fourth group.  world_dir: Hit.r of a placed hit is
    the WORLD direction -- not what Rust2 does; the test that shows the rule decides pixels renders both."""

    def __init__(self, tris, placements, spheres=(), quads=(), instances=(), background=(0.0, 0.0, 0.0), mint=MINT, maxt=MAXT, world_dir=False):
        super().__init__(spheres, quads, instances, (), background, mint=mint, maxt=maxt)
        self.T, self.placements, self.world_dir = tris, list(placements), world_dir

    def install(self, gpu, t0=0.0, t1=0.0, placements=True):
        gpu.set_scene(self.scene, t0, t1)
        if self.instances:
            gpu.set_instance_rotations(self.quats)
        gpu.set_triangles(self.T.pods())
        if placements:
            gpu.set_mesh_instances(self.placements)

    def closest(self, o, d, tm=0.0):
        h = super().closest(o, d, tm)
        o, d = f32(o).reshape(-1, 3), f32(d).reshape(-1, 3)
        m = placement_hits(self.T, self.placements, o, d, self.mint, self.maxt)
        with np.errstate(all="ignore"):
            win = m["found"] & (~h["found"] | (h["t"] > m["t"]))                  # the group replaces the result so far only when strictly closer
        base = len(self.spheres) + len(self.quads) + len(self.instances)
        h["found"] = h["found"] | win
        h["t"] = np.where(win, m["t"], h["t"]).astype(F)
        h["idx"] = np.where(win, base + m["placement"], h["idx"])
        h["point"][win] = m["point"][win]
        h["normal"][win] = m["normal"][win]
        h["member"] = np.where(win, m["triangle"], h["member"])
        if not self.world_dir:
            h["din"][win] = m["local"][win]
        return h

    def surface(self, idx, member):
        base = len(self.spheres) + len(self.quads) + len(self.instances)
        if idx < base:
            return super().surface(idx, member)
        t = self.T.tris[member]
        return QC._mat(t), LC.v((f32(t["color"]) * F(1.0)).astype(F)), LC.v(t["emitted"])


_FRAMES = {}


def render(ms, cam, params, key):
    """The restated frame at gamma 1 under any sampler (lights_common.pixel_samples, quat_common.trace, lights_common.resolve): ([h][w][3] f32,
    segments), kept under `key` and computed once."""
    k = (key, params.width, params.height, params.samples, params.depth, params.sampler, params.seed, ms.world_dir)
    if k not in _FRAMES:
        assert params.gamma == 1.0 and params.integrator == R.INTEGRATOR_RUST2 and params.flags & ~R.FLAG_GLOBAL_NODES == 0
        img = np.empty((params.height, params.width, 3), F)
        seg = 0
        for j in range(params.height):
            for i in range(params.width):
                cols = []
                for o, d, tm, rng in LC.pixel_samples(cam, params, i, j):
                    r = QC.trace(ms, o, d, params, rng, time=tm)
                    cols.append(r["ftb"])
                    seg += r["queries"]
                img[j, i] = LC.resolve(params, cols)
        _FRAMES[k] = (img, seg)
    return _FRAMES[k]
