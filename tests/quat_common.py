"""Restatement of Rust2's quaternion-rotated instances (Rust2/src/quaternions.rs, rotation.rs, objects/instance.rs:215-255) in numpy f32, one
rounding per written operation -- the reference of tests/test_quat_instances_cpu.py and tests/test_gpu_quat_instances.py.

    Quaternion::rotate, hamilton, new_from_axis, From<&EulerAngles>          rotate / hamilton / from_axis / from_euler
    Instance::get_hit over quad and sphere members                             QuatScene.closest (the instance group)
    the scene's closest hit over spheres / quads / instances                   QuatScene.closest, the library's tie order (rtw.h)
    a RUST2 / LIGHT_CAST / LIGHT_BIASED path on the oracle's RNG stream         trace / render, built like tests/lights_common.trace

Everything is evaluated on float32 arrays (every numpy operation on them rounds once to f32), so one code path serves a single ray and
thousands.  The closest hit is NOT the oracle's (which knows no quaternions): it is restated here.  The random stream, the camera samples,
on_hit, material_pdf, the light term and the resolve are lights_common's / mixed_common's pure helpers."""
import ctypes as C
import ctypes.util
import json
import os

import numpy as np

import rtw_amd as R
from tests import lights_common as LC
from tests import mixed_common as MC

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rust2_rotation_scene.json")
CAST, BIASED, RUST2 = R.INTEGRATOR_LIGHT_CAST, R.INTEGRATOR_LIGHT_BIASED, R.INTEGRATOR_RUST2

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = C.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [C.c_float]


def sinf(x):
    return F(_libm.sinf(float(F(x))))


def cosf(x):
    return F(_libm.cosf(float(F(x))))


def f32(x):
    return np.asarray(x, dtype=F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


# ---- the quaternion -----------------------------------------------------------------------------------------------------------------
def hamilton(a, b):
    """Quaternion::hamilton (quaternions.rs:141-149) on [..., 4] = w, x, y, z."""
    a, b = f32(a), f32(b)
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    with np.errstate(all="ignore"):
        return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                         aw * bx + ax * bw + ay * bz - az * by,
                         aw * by - ax * bz + ay * bw + az * bx,
                         aw * bz + ax * by - ay * bx + az * bw], axis=-1).astype(F)


def qlen(q):
    q = f32(q)
    with np.errstate(all="ignore"):
        return np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3]).astype(F)


def normalised(q):
    """`self * (1.0 / self.len())` (quaternions.rs:181)."""
    q = f32(q)
    with np.errstate(all="ignore"):
        s = (F(1.0) / qlen(q)).astype(F)
        return (q * s[..., None]).astype(F)


def rotate_n(qn, v):
    """The rest of Quaternion::rotate for a normalised qn: (qn (0, v) conj(qn)).get_vec(), every term kept."""
    qn, v = f32(qn), f32(v)
    shape = np.broadcast_shapes(qn.shape[:-1], v.shape[:-1])
    qn = np.broadcast_to(qn, shape + (4,))
    v = np.broadcast_to(v, shape + (3,))
    p = np.concatenate([np.zeros(shape + (1,), F), v], axis=-1)
    cq = (qn * f32([1.0, -1.0, -1.0, -1.0])).astype(F)          # conjugate: exact negations
    return hamilton(hamilton(qn, p), cq)[..., 1:].copy()


def rotate(q, v):
    """Quaternion::rotate (quaternions.rs:180-186)."""
    return rotate_n(normalised(q), v)


def from_axis(angle, axis):
    """Quaternion::new_from_axis (quaternions.rs:114-123), sin / cos through the platform's sinf / cosf."""
    a = f32(axis)
    with np.errstate(all="ignore"):
        u = (a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])).astype(F)
        half = F(F(angle) * F(0.5))
        s = sinf(half)
        return f32([cosf(half), s * u[0], s * u[1], s * u[2]])


def from_euler(e):
    """From<&EulerAngles> for Quaternion (quaternions.rs:68-85)."""
    cx, cy, cz = cosf(e[0]), cosf(e[1]), cosf(e[2])
    sx, sy, sz = sinf(e[0]), sinf(e[1]), sinf(e[2])
    return f32([cx * cy * cz + sx * sy * sz, sx * cy * cz - cx * sy * sz, cx * sy * cz - sx * cy * sz, cx * cy * sz - sx * sy * cz])


# ---- primitives ---------------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


class QuadSet:
    """K quads with the derived fields of Quad::new as the library forms them (n = u x v, normal = n / |n|, d = normal . origin, w = n / n.n)."""

    def __init__(self, quads):
        self.k = len(quads)
        self.origin = f32([q["origin"] for q in quads]).reshape(-1, 3)
        self.u = f32([q["u"] for q in quads]).reshape(-1, 3)
        self.v = f32([q["v"] for q in quads]).reshape(-1, 3)
        if self.k:
            n = cross3(self.u, self.v)
            nn = dot3(n, n)
            with np.errstate(all="ignore"):
                self.normal = (n / np.sqrt(nn)[:, None]).astype(F)
                self.w = (n / nn[:, None]).astype(F)
            self.d = dot3(self.normal, self.origin)

    def pick(self, o, d, mint, maxt, found, cur_t):
        """Quads in list order against rays o, d [N][3] (quad.rs:37-63 as the device's quad_pick): a quad replaces the current hit when it is
        a Some(hit) and (nothing found yet or cur_t > t).  Returns (found, t, index [N], -1 where no quad replaced what came in)."""
        n = len(o)
        idx = np.full(n, -1, np.int64)
        if not self.k:
            return found, cur_t, idx
        with np.errstate(all="ignore"):
            oo, dd = o[:, None, :], d[:, None, :]
            den = dot3(self.normal[None], dd)
            t = (self.d[None] - dot3(self.normal[None], oo)) / den
            point = oo + dd * t[..., None]
            planar = point - self.origin[None]
            alfa = dot3(self.w[None], cross3(planar, np.broadcast_to(self.v[None], planar.shape)))
            beta = dot3(self.w[None], cross3(np.broadcast_to(self.u[None], planar.shape), planar))
            ok = ~(np.abs(den) <= F(1e-8)) & ~((t < mint) | (t > maxt)) & ~((alfa < 0) | (alfa > 1) | (beta < 0) | (beta > 1))
            found, cur_t = found.copy(), cur_t.copy()
            for k in range(self.k):
                take = ok[:, k] & (~found | (cur_t > t[:, k]))
                found |= take
                cur_t = np.where(take, t[:, k], cur_t)
                idx = np.where(take, k, idx)
        return found, cur_t, idx


class SphereSet:
    def __init__(self, spheres):
        self.k = len(spheres)
        self.c = f32([s["origin"] for s in spheres]).reshape(-1, 3)
        self.vel = f32([s.get("velocity", (0.0, 0.0, 0.0)) for s in spheres]).reshape(-1, 3)
        r = f32([s["radius"] for s in spheres]).reshape(-1)
        self.r2 = (r * r).astype(F)

    def centre(self, k, tm):
        return (self.c[k] + self.vel[k] * F(tm)).astype(F)

    def pick(self, o, d, tm, mint, maxt):
        """Spheres in list order (sphere.rs:99-147 as the device's closest_brute / instance_pick): (found, t, index [N])."""
        n = len(o)
        found, cur_t, idx = np.zeros(n, bool), np.zeros(n, F), np.full(n, -1, np.int64)
        with np.errstate(all="ignore"):
            a = dot3(d, d)
            for k in range(self.k):
                oc = o - self.centre(k, tm)[None]
                b = dot3(oc, d)
                c = dot3(oc, oc) - self.r2[k]
                disc = b * b - a * c
                sq = np.sqrt(disc)
                x = (-b - sq) / a
                x = np.where(x < mint, (-b + sq) / a, x)
                take = ~(disc < 0) & ~((x < mint) | (x > maxt)) & (~found | (cur_t > x))
                found |= take
                cur_t = np.where(take, x, cur_t).astype(F)
                idx = np.where(take, k, idx)
        return found, cur_t, idx


def unit3(a):
    with np.errstate(all="ignore"):
        return (a / np.sqrt(dot3(a, a))[..., None]).astype(F)


def _mat(d):
    return LC.MATS[d["material"]] if isinstance(d["material"], str) else tuple(d["material"])


class QuatScene:
    """Top-level spheres and quads and quaternion instances {"quads", "spheres", "translation", "quat"} (dicts as lights_common.LightScene's),
    the R.Scene of them, the rotations for Renderer.set_instance_rotations, and the restated closest hit."""

    def __init__(self, spheres=(), quads=(), instances=(), lights=(), background=(0.0, 0.0, 0.0), weight=100.0, mint=1e-4, maxt=1e4):
        self.spheres, self.quads, self.instances = list(spheres), list(quads), list(instances)
        self.lights, self.weight = list(lights), float(weight)
        self.background = LC.v(background)
        self.mint, self.maxt = F(mint), F(maxt)
        self.S, self.Q = SphereSet(self.spheres), QuadSet(self.quads)
        self.I = [(SphereSet(i.get("spheres", ())), QuadSet(i.get("quads", ())), f32(i["translation"]), normalised(f32(i["quat"]))) for i in self.instances]
        self.quats = f32([i["quat"] for i in self.instances]).reshape(-1, 4)
        self.moving = any(np.any(f32(s.get("velocity", (0, 0, 0))) != 0) for s in self.spheres)

        def rs(s):
            x = R.Sphere.with_albedo(s["origin"], s["radius"], s["color"], _mat(s), velocity=[float(c) for c in s.get("velocity", (0.0, 0.0, 0.0))])
            for k in range(3):
                x.pod.emitted[k] = float(s["emitted"][k])
            return x

        def rq(q):
            return R.Quad.new(q["origin"], q["u"], q["v"], _mat(q), q["color"], q["emitted"])

        inst = []
        for i in self.instances:
            x = R.Instance([rs(s) for s in i.get("spheres", ())], [rq(q) for q in i.get("quads", ())])
            x.translation = [float(c) for c in i["translation"]]
            inst.append(x)
        self.scene = R.Scene([rs(s) for s in self.spheres], background=background, quads=[rq(q) for q in self.quads], instances=inst)
        self.mids = [LC.mid_sphere(self.spheres[i]["origin"], self.spheres[i]["radius"]) if k == R.LIGHT_SPHERE else
                     LC.mid_quad(self.quads[i]["origin"], self.quads[i]["u"], self.quads[i]["v"]) for k, i in self.lights]
        self.light_obj = [i if k == R.LIGHT_SPHERE else len(self.spheres) + i for k, i in self.lights]

    def install(self, gpu, t0=0.0, t1=0.0, rotations=True):
        gpu.set_scene(self.scene, t0, t1)
        if rotations:
            gpu.set_instance_rotations(self.quats)
        if self.lights:
            gpu.set_lights(self.lights, self.weight)

    def closest(self, o, d, tm=0.0):
        """The closest hit of rays o, d [N][3] at ray.time tm: dict of found [N], t, idx (top-level: spheres, quads, instances; -1), point,
        normal [N][3], member [N] (an instance's member: >= 0 sphere, < 0 quad ~member), din [N][3] = Hit.r.direction: the ray's direction,
        or for a member of an instance the direction in the instance's frame (the member's get_hit stores the ray it was given, and
        Instance::get_hit turns back p and n only) -- what on_hit and material_pdf read as the incoming direction."""
        o, d = f32(o).reshape(-1, 3), f32(d).reshape(-1, 3)
        n = len(o)
        mint, maxt = self.mint, self.maxt
        with np.errstate(all="ignore"):
            found, t, si = self.S.pick(o, d, tm, mint, maxt)
            idx = si.copy()
            point = (o + d * t[:, None]).astype(F)
            normal = np.zeros((n, 3), F)
            for k in range(self.S.k):
                m = si == k
                if m.any():
                    normal[m] = unit3(point[m] - self.S.centre(k, tm)[None])
            # quads: the closest in list order, then against the spheres (strictly closer)
            qf, qt, qi = self.Q.pick(o, d, mint, maxt, np.zeros(n, bool), np.zeros(n, F))
            win = qf & (~found | (t > qt))
            found = found | win
            t = np.where(win, qt, t).astype(F)
            idx = np.where(win, len(self.spheres) + qi, idx)
            if win.any():
                point[win] = (o[win] + d[win] * qt[win, None]).astype(F)
                normal[win] = self.Q.normal[qi[win]]
            # instances: Instance::get_hit, the closest of them, then against what came before (strictly closer)
            ifound, it, ii = np.zeros(n, bool), np.zeros(n, F), np.full(n, -1, np.int64)
            imember = np.zeros(n, np.int64)
            ipoint, inormal, idir = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
            for k, (ss, qq, tr, qn) in enumerate(self.I):
                loc = rotate_n(qn, np.stack([(o - tr[None]).astype(F), d], axis=1))        # r.origin -= position; r = r.rotated(q)
                lo, ld = np.ascontiguousarray(loc[:, 0]), np.ascontiguousarray(loc[:, 1])
                mf, mt, ms = ss.pick(lo, ld, tm, mint, maxt)
                mf2, mt2, mq = qq.pick(lo, ld, mint, maxt, mf, mt)
                member = np.where(mq >= 0, ~mq, ms)
                lp = (lo + ld * mt2[:, None]).astype(F)
                ln = np.zeros((n, 3), F)
                isq = mf2 & (mq >= 0)
                if isq.any():
                    ln[isq] = qq.normal[mq[isq]]
                for s in range(ss.k):
                    m = mf2 & (mq < 0) & (ms == s)
                    if m.any():
                        ln[m] = unit3(lp[m] - ss.centre(s, tm)[None])
                take = mf2 & (~ifound | (it > mt2))
                if take.any():
                    ipoint[take] = (rotate_n(qn, lp[take]) + tr[None]).astype(F)          # p = q.rotate(p) + position
                    inormal[take] = rotate_n(qn, ln[take])                                  # n = q.rotate(n): the same q
                    idir[take] = ld[take]                                                   # Hit.r stays the LOCAL ray (get_hit does not turn it back)
                ifound |= take
                it = np.where(take, mt2, it).astype(F)
                ii = np.where(take, k, ii)
                imember = np.where(take, member, imember)
            win = ifound & (~found | (t > it))
            found = found | win
            t = np.where(win, it, t).astype(F)
            idx = np.where(win, len(self.spheres) + len(self.quads) + ii, idx)
            point[win] = ipoint[win]
            normal[win] = inormal[win]
            member = np.where(win, imember, 0)
            din = d.copy()
            din[win] = idir[win]
        idx = np.where(found, idx, -1)
        normal[~found] = 0
        return {"found": found, "t": t, "idx": idx, "point": point, "normal": normal, "member": member, "din": din}

    def surface(self, idx, member):
        """(material, multiplied, emitted) of the top-level object idx (an instance's member `member`)."""
        ns, nq = len(self.spheres), len(self.quads)
        if idx < ns:
            d = self.spheres[idx]
        elif idx < ns + nq:
            d = self.quads[idx - ns]
        else:
            inst = self.instances[idx - ns - nq]
            d = inst["spheres"][member] if member >= 0 else inst["quads"][~member]
        return _mat(d), LC.v(d["color"]), LC.v(d["emitted"])

    def params(self, width, height, integrator, depth, samples=4, seed=1, flags=0, accel=None):
        p = R.RtwParams()
        p.width, p.height, p.samples, p.depth = width, height, samples, depth
        p.gamma, p.mint, p.maxt = 1.0, float(self.mint), float(self.maxt)
        p.integrator, p.sampler, p.flags = integrator, R.SAMPLER_CENTRES, flags
        p.accel = R.ACCEL_BRUTE if accel is None else accel
        p.seed = seed
        p.row_block, p.part_index, p.part_count = 8, 0, 1
        return p


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------
def golden():
    return json.load(open(GOLDEN))


def box_instance(g, material=None, quat=None):
    quads = [dict(q, material=material or g["material"], color=g["color"], emitted=g["emitted"]) for q in g["box_quads"]]
    return {"quads": quads, "spheres": [], "translation": g["translation"], "quat": g["quaternion_wxyz"] if quat is None else quat}


def fixture_scene(g=None, spheres=(), quads=(), lights=(), material=None, extra_instances=()):
    g = g or golden()
    return QuatScene(spheres, quads, [box_instance(g, material)] + list(extra_instances), lights, g["background"], mint=g["mint"], maxt=g["maxt"])


def camera(g, width, height):
    c = g["camera"]
    return R.camera2_new(width / height * c["aspect"], c["origin"], c["vup"], c["direction"], c["vfov"], c["lens_radius"])


def depth_rays(cam, width, height):
    """Viewport::depth_map's rays (rtw.h rtw_depth_rays): unit(left_top + delta_x * (i / width) + delta_y * (j / height)), row-major."""
    o, p00, du, dv = (f32(list(x)) for x in (cam.origin, cam.pixel00, cam.delta_u, cam.delta_v))
    i, j = np.meshgrid(np.arange(width), np.arange(height))
    fx = (i.reshape(-1).astype(F) / F(width)).astype(F)
    fy = (j.reshape(-1).astype(F) / F(height)).astype(F)
    d = ((p00[None] + du[None] * fx[:, None]).astype(F) + dv[None] * fy[:, None]).astype(F)
    return np.broadcast_to(o, d.shape).copy(), unit3(d)


# ---- the path -------------------------------------------------------------------------------------------------------------------------------
def trace(qs, o, d, params, rng, time=0.0):
    """One camera ray under RUST2 / LIGHT_BIASED / LIGHT_CAST, front to back as the device computes it (lights_common.trace's "ftb"; RUST2 is
    LIGHT_BIASED with no lights): {"ftb", "queries", "hits", "blocked", "reached", "blocked_inst", "side_differs"} -- shadow queries
    whose closest hit was another object / was the light / was an instance, and accepted lights for which material_pdf's side test
    (h.r.direction . n >= 0) differs between the instance-local direction Rust2's Hit carries and the path's world direction."""
    integ = params.integrator
    mixed = bool(params.flags & R.FLAG_MIXED_MATERIAL)
    walks = integ != CAST
    lights = range(len(qs.lights)) if integ in (CAST, BIASED) else range(0)
    depth = params.depth if walks else 1
    on_hit = MC.on_hit if mixed else LC.on_hit
    material_pdf = MC.material_pdf if mixed else LC.material_pdf
    L, thr = np.zeros(3, F), np.ones(3, F)
    queries = hits = blocked = reached = blocked_inst = side_differs = 0
    first_inst = len(qs.spheres) + len(qs.quads)
    o, d = LC.v(o), LC.v(d)
    end_bg = True
    with np.errstate(all="ignore"):
        for _ in range(depth):
            h = qs.closest(o, d, time)
            queries += 1
            if not h["found"][0]:
                break
            hits += 1
            p, n, din = h["point"][0].copy(), h["normal"][0].copy(), h["din"][0].copy()
            mat, m, e = qs.surface(int(h["idx"][0]), int(h["member"][0]))
            scat, scat_time = None, None
            if walks:
                scat = on_hit(mat, n, din, rng)
                if mixed:
                    scat, scat_time = scat                       # (direction, 0.0 for a MixedMaterial's Ray::new or None)
            S, count = np.zeros(3, F), F(1.0) if walks else F(0.0)
            for li in lights:
                to = (qs.mids[li] - p).astype(F)
                rd = (to / np.sqrt(LC.dot(to, to))).astype(F)
                sh = qs.closest(p, rd, 0.0)
                if not sh["found"][0] or int(sh["idx"][0]) != qs.light_obj[li]:
                    blocked += int(sh["found"][0])
                    blocked_inst += int(sh["found"][0] and int(sh["idx"][0]) >= first_inst)
                    continue
                reached += 1
                side_differs += int(bool(LC.dot(din, n) >= F(0.0)) != bool(LC.dot(d, n) >= F(0.0)))
                _, _, el = qs.surface(int(sh["idx"][0]), 0)
                pdf = material_pdf(mat, p, n, din, time, p, rd, 0.0)
                s, dc = LC.light_term(integ == BIASED, pdf, el, sh["t"][0], rd, qs.weight)
                if s is None:
                    continue
                S = (S + s).astype(F)
                count = F(count + dc)
            if not walks:
                c = ((S * m).astype(F) / count).astype(F) if count != F(0.0) else np.zeros(3, F)
                return {"ftb": (c + e).astype(F), "queries": queries, "hits": hits, "blocked": blocked, "reached": reached, "blocked_inst": blocked_inst,
                        "side_differs": side_differs}
            L = (L + (thr * (((S * m).astype(F) / count).astype(F) + e).astype(F)).astype(F)).astype(F)
            thr = (thr * (m / count).astype(F)).astype(F)
            o, d = p, scat
            if scat_time is not None:
                time = scat_time
        if end_bg:
            L = (L + (qs.background * thr).astype(F)).astype(F)
    return {"ftb": L, "queries": queries, "hits": hits, "blocked": blocked, "reached": reached, "blocked_inst": blocked_inst,
            "side_differs": side_differs}


_FRAMES = {}


def render(qs, cam, params, key=None):
    """The restated frame at gamma 1 under RTW_SAMPLER_CENTRES: ([h][w][3] f32, segments, {"blocked", "reached"}).  `key`: the frame is kept
    under it and computed once (the tests that share a scene share its reference)."""
    k = None if key is None else (key, params.width, params.height, params.samples, params.depth, params.integrator, params.flags, params.seed)
    if k is not None and k in _FRAMES:
        return _FRAMES[k]
    assert params.sampler == R.SAMPLER_CENTRES and params.gamma == 1.0
    img = np.empty((params.height, params.width, 3), F)
    seg, info = 0, {"blocked": 0, "reached": 0, "blocked_inst": 0, "side_differs": 0}
    n_l = len(qs.lights) if params.integrator in (CAST, BIASED) else 0
    for j in range(params.height):
        for i in range(params.width):
            cols = []
            for o, d, tm, rng in LC.pixel_samples(cam, params, i, j):
                r = trace(qs, o, d, params, rng, time=tm)
                cols.append(r["ftb"])
                seg += r["queries"] + n_l * r["hits"]
                for kk in info:
                    info[kk] += r[kk]
            img[j, i] = LC.resolve(params, cols)
    out = (img, seg, info)
    if k is not None:
        _FRAMES[k] = out
    return out
