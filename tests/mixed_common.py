"""Restatement of Rust2's MixedMaterial (Rust2/src/objects/material.rs:235-297, onb.rs:30-44) in numpy f32 on top of tests/lights_common.py
(imported as it is) -- the reference of tests/test_mixed_cpu.py and tests/test_gpu_mixed.py.

on_hit and material_pdf gain the mixed branch, one f32 rounding per operation; pow_plain / sin_plain / cos_plain are restated operation for
operation from csrc/rtw_mixed.h (fmaf emulated exactly: the product and the sum in f64, the sum rounded to odd before the final rounding to
f32).  The frozen oracle supplies only closest hits (depth-1 RTW_INTEGRATOR_RUST2 traces, the new flag bit cleared) and the random stream.
The hop-by-hop check against the oracle's full RUST2 trace stays on for every path until it meets a mixed surface.
"""
import json
import os

import numpy as np

import rtw_amd as R
from tests import lights_common as LC
from tests import oracle_binding as O

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rust2_mixed_scene.json")
PI = F(3.14159265358979323846)
FRAC_1_2PI = F(F(F(1.0) / F(2.0)) / PI)
v, dot, unit, veq = LC.v, LC.dot, LC.unit, LC.veq


# ---- exact f32 fmaf over arrays -----------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fmaf(a, b, c) for f32 arrays: a * b is exact in f64; the f64 sum is rounded to odd (TwoSum gives the discarded part), so the final
    rounding to f32 is the rounding of the exact a * b + c."""
    with np.errstate(all="ignore"):
        a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
        toward = np.where(err > 0, np.inf, -np.inf)
        nudge = (err != 0) & np.isfinite(s) & ((bits & 1) == 0)
        s = np.where(nudge, np.nextafter(s, toward), s)
        return s.astype(F)


def _bits(x):
    return np.asarray(x, F).view(np.uint32).astype(np.int64)


def _from_bits(b):
    return np.asarray(b, np.int64).astype(np.uint32).view(F)


def pow_plain(x, y):
    """csrc/rtw_mixed.h pow_plain, operation for operation."""
    with np.errstate(all="ignore"):
        x, y = np.broadcast_arrays(np.asarray(x, F), np.asarray(y, F))
        tiny = x < F(2.0 ** -126)
        xs = np.where(tiny, x * F(2.0 ** 24), x).astype(F)
        b = _bits(xs)
        e = (((b >> 23) & 0xFF) - 127).astype(F) - np.where(tiny, F(24.0), F(0.0))
        man = b & 0x7FFFFF
        upper = man >= 0x3504F3
        m = _from_bits(man | np.where(upper, 0x3F000000, 0x3F800000))
        e = np.where(upper, e + F(1.0), e).astype(F)
        f = (m - F(1.0)).astype(F)
        dh = (m + F(1.0)).astype(F)
        dl = (m - (dh - F(1.0)).astype(F)).astype(F)
        s_hi = (f / dh).astype(F)
        rem = fma(-s_hi, dh, f)
        rem = fma(-s_hi, dl, rem)
        s_lo = (rem / dh).astype(F)
        z = (s_hi * s_hi).astype(F)
        Q = np.full(z.shape, F(0.23330962657928467), F)
        for k in (0.28550803661346436, 0.4000012278556824, 0.6666666865348816):
            Q = fma(Q, z, F(k))
        t_hi = (s_hi + s_hi).astype(F)
        c = fma((s_hi * z).astype(F), Q, (s_lo + s_lo).astype(F))
        HI, LO = F(1.4426950216293335), F(1.925963033500011e-08)
        p_hi = (t_hi * HI).astype(F)
        p_lo = fma(t_hi, HI, -p_hi)
        p_lo = fma(t_hi, LO, p_lo)
        p_lo = fma(c, HI, p_lo)
        a_hi = (e + p_hi).astype(F)
        a_lo = ((p_hi - (a_hi - e).astype(F)).astype(F) + p_lo).astype(F)
        q_hi = (y * a_hi).astype(F)
        q_lo = fma(y, a_lo, fma(y, a_hi, -q_hi))
        n = np.rint(np.fmin(np.fmax(q_hi, F(-252.0)), F(254.0))).astype(F)
        r = np.fmin(np.fmax(((q_hi - n).astype(F) + q_lo).astype(F), F(-1.0)), F(1.0)).astype(F)
        E = np.full(r.shape, F(1.529732435301412e-05), F)
        for k in (0.00015461444854736328, 0.0013333501992747188, 0.009618056938052177, 0.05550410971045494, 0.24022650718688965,
                  0.6931471824645996):
            E = fma(E, r, F(k))
        val = fma(r, E, F(1.0))
        ni = n.astype(np.int64)
        n1 = ni >> 1
        n2 = ni - n1
        res = ((val * _from_bits((n1 + 127) << 23)).astype(F) * _from_bits((n2 + 127) << 23)).astype(F)
        res = np.where(x == F(0.0), F(0.0), res)
        res = np.where(x == F(np.inf), F(np.inf), res)
        res = np.where((x != x) | (x < F(0.0)), F(np.nan), res)
        return np.where(y == F(0.0), F(1.0), res).astype(F)


def sincos_plain(phi):
    """csrc/rtw_mixed.h sincos_plain, operation for operation: (sin, cos)."""
    with np.errstate(all="ignore"):
        phi = np.asarray(phi, F)
        k = np.rint((phi * F(0.6366197466850281)).astype(F)).astype(F)
        r = fma(-k, F(1.5707963705062866), phi)
        r = fma(-k, F(-4.371138828673793e-08), r)
        r = fma(-k, F(-1.7151245100058819e-15), r)
        s = (r * r).astype(F)
        S = np.full(s.shape, F(2.7243811473454116e-06), F)
        for c in (-0.00019840039021801203, 0.008333331905305386, -0.1666666716337204):
            S = fma(S, s, F(c))
        sr = fma((r * s).astype(F), S, r)
        Cq = np.full(s.shape, F(-2.7295945415062306e-07), F)
        for c in (2.4800561732263304e-05, -0.00138888880610466, 0.0416666679084301):
            Cq = fma(Cq, s, F(c))
        h = (F(0.5) * s).astype(F)
        w = (F(1.0) - h).astype(F)
        cr = (w + fma((s * s).astype(F), Cq, ((F(1.0) - w).astype(F) - h).astype(F))).astype(F)
        swap = (k == F(1.0)) | (k == F(3.0))
        a, b = np.where(swap, cr, sr), np.where(swap, sr, cr)
        sn = np.where((k == F(2.0)) | (k == F(3.0)), -a, a).astype(F)
        cs = np.where((k == F(1.0)) | (k == F(2.0)), -b, b).astype(F)
        return sn, cs


def sin_plain(phi):
    return sincos_plain(phi)[0]


def cos_plain(phi):
    return sincos_plain(phi)[1]


# ---- the material -------------------------------------------------------------------------------------------------------------------
def cross(a, b):
    return np.array([F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))], F)


def mixed_dir(exp, xi_phi, xi_cos, n):
    """MixedMaterial::new(exp).on_hit(h)'s direction for the two draws: ONB::new_from_w(h.n).from_local(gen_random_dir())."""
    with np.errstate(all="ignore"):
        exp, xi_phi, xi_cos, n = F(exp), F(xi_phi), F(xi_cos), v(n)
        gen_exp = F(F(1.0) / F(exp + F(1.0)))
        w = unit(n)
        a = v([0.0, 1.0, 0.0]) if abs(w[0]) > F(0.9) else v([1.0, 0.0, 0.0])
        vv = unit(cross(w, a))
        u = unit(cross(w, vv))
        phi = F(F(xi_phi * F(2.0)) * PI)
        ct = F(pow_plain(F(F(1.0) - xi_cos), gen_exp))
        st = F(np.sqrt(F(F(1.0) - F(ct * ct))))
        sp, cp = sincos_plain(phi)
        x, y = F(F(cp) * st), F(F(sp) * st)
        return (((u * x).astype(F) + (vv * y).astype(F)).astype(F) + (w * ct).astype(F)).astype(F)


def mixed_pdf(exp, p, n, din, ro, rd):
    """MixedMaterial::material_pdf (material.rs:280-296)."""
    with np.errstate(all="ignore"):
        exp = F(exp)
        if not veq(v(ro), v(p)):
            return F(0.0)
        c0 = dot(unit(v(rd)), unit(v(n)))
        cos = c0 if dot(v(din), v(n)) < F(0.0) else F(-c0)
        if cos < F(0.0):
            return F(0.0)
        return F(F(F(pow_plain(cos, exp)) * F(exp + F(1.0))) * FRAC_1_2PI)


def is_mixed(mat):
    return F(mat[1]) < F(0.0)


KEEP_TIME = False       # tests only: True restates a MixedMaterial WITHOUT the reference's quirk (the scattered ray would keep h.r.time)


def on_hit(mat, n, din, rng):
    """(direction, ray.time of the scattered ray or None = the incoming ray's)."""
    if is_mixed(mat):
        xi_phi = rng.next()
        xi_cos = rng.next()
        return mixed_dir(mat[2], xi_phi, xi_cos, n), (None if KEEP_TIME else 0.0)        # Ray::new: time 0
    return LC.on_hit(mat, n, din, rng), None


def material_pdf(mat, p, n, din, tm, ro, rd, rtm):
    if is_mixed(mat):
        return mixed_pdf(mat[2], p, n, din, ro, rd)
    return LC.material_pdf(mat, p, n, din, tm, ro, rd, rtm)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def material_of(d):
    """A fixture's material entry: a name of lights_common.MATS, "mixed" (with "exp"), or a triple."""
    m = d["material"]
    if m == "mixed":
        return R.mixed(d["exp"])
    return LC.MATS[m] if isinstance(m, str) else tuple(m)


class MixedScene(LC.LightScene):
    """lights_common.LightScene with "mixed" materials resolved and, optionally, box instances whose six quads share one material and
    colour (the oracle reports which instance was hit, not which member).  boxes: dicts {a, b, material[, exp], color, rotation,
    translation}."""

    def __init__(self, spheres, quads, lights, background=(0.0, 0.0, 0.0), weight=100.0, boxes=()):
        spheres = [dict(s, material=material_of(s)) for s in spheres]
        quads = [dict(q, material=material_of(q)) for q in quads]
        super().__init__(spheres, quads, lights, background, weight=weight)
        self.boxes = [dict(b, material=material_of(b)) for b in boxes]
        if self.boxes:
            inst = []
            for b in self.boxes:
                it = R.Instance.new_box(b["a"], b["b"], b["color"], b["material"])
                it.rotate(b.get("rotation", (0.0, 0.0, 0.0)))
                it.translate(b.get("translation", (0.0, 0.0, 0.0)))
                inst.append(it)
            self.scene._set_geom([self.scene._quads[k] for k in range(len(self.quads))], inst)

    def _box(self, obj):
        k = obj - len(self.spheres) - len(self.quads)
        return self.boxes[k] if k >= 0 else None

    def mat(self, obj):
        b = self._box(obj)
        return b["material"] if b is not None else super().mat(obj)

    def color(self, obj, normal):
        b = self._box(obj)
        return (v(b["color"]), np.zeros(3, F)) if b is not None else super().color(obj, normal)

    def has_mixed(self):
        return any(is_mixed(d["material"]) for d in self.spheres + self.quads + self.boxes)


def golden(weight=None):
    g = json.load(open(GOLDEN))
    kinds = {"sphere": R.LIGHT_SPHERE, "quad": R.LIGHT_QUAD}
    ms = MixedScene(g["spheres"], g["quads"], [(kinds[l["kind"]], l["index"]) for l in g["lights"]], g["background"],
                    weight=g["biased_weight"] if weight is None else weight)
    return ms, g


def oracle_params(params, **kw):
    """A copy of params for the frozen oracle: RTW_INTEGRATOR_RUST2, the new flag bit cleared."""
    p = R.RtwParams.from_buffer_copy(params)
    p.integrator = R.INTEGRATOR_RUST2
    p.flags &= ~R.FLAG_MIXED_MATERIAL
    for k, x in kw.items():
        setattr(p, k, x)
    return p


def trace(ms, o, d, params, pixel, check=True, time=0.0, rng=None):
    """lights_common.trace with the mixed branch and RTW_INTEGRATOR_RUST2 (LIGHT_BIASED's path without lights).  Returns {"ftb", "rec",
    "queries", "hits", "shadow" (shadow queries), "bound", "mixed_hits", "times" (ray.time of every path query)}.  check: hop by hop against
    the oracle's full RUST2 trace for as long as the path has met no mixed surface (`rng` None only).  Also "inst_hits" (path hits on an
    instance), "shadow_inst" (shadow queries whose closest hit is an instance), "reached" / "blocked" (per light: shadow queries whose closest
    hit is the light's own object / another object)."""
    assert rng is None or not check
    mixed_on = bool(params.flags & R.FLAG_MIXED_MATERIAL)
    time = float(F(time))
    cast = params.integrator == R.INTEGRATOR_LIGHT_CAST
    lights = [] if params.integrator == R.INTEGRATOR_RUST2 else list(range(len(ms.lights)))
    depth = 1 if cast else params.depth
    p1 = oracle_params(params, depth=1)
    full = None
    if check and not cast:
        full, _ = O.trace_ray(o, d, time, ms.scene, oracle_params(params), pixel, 0, cap=max(4, depth + 2))
    rng = LC.Rng(params.seed, pixel) if rng is None else rng
    levels, queries, hits, shadow, mixed_hits, times = [], 0, 0, 0, 0, []
    n_top = len(ms.spheres) + len(ms.quads)                  # object codes from here on are instances
    inst_hits, shadow_inst, reached, blocked = 0, 0, [0] * len(ms.lights), [0] * len(ms.lights)
    end_bg = True
    o, d = v(o), v(d)
    for k in range(depth):
        h = LC.closest(ms, o, d, p1, pixel, time)
        queries += 1
        times.append(time)
        if full is not None and mixed_hits == 0:
            assert k < len(full), (k, len(full))
            fb = full[k]
            assert bool(fb.hit) == (h is not None), ("hop", k)
            if h is not None:
                assert fb.sphere == h[0] and F(fb.t).tobytes() == h[1].tobytes(), ("hop", k, fb.sphere, h[0], fb.t, h[1])
                assert v(list(fb.point)).tobytes() == h[2].tobytes() and v(list(fb.normal)).tobytes() == h[3].tobytes(), ("hop", k)
        if h is None:
            break
        hits += 1
        obj, t, p, n = h
        inst_hits += int(obj >= n_top)
        mat = ms.mat(obj)
        if not mixed_on and is_mixed(mat):
            mat = (mat[0], 0.0, mat[2])                      # without the flag opacity < 0 is Mirror / Lambertian by metallicness
        m, e = ms.color(obj, n)
        scat, t_next = (None, None) if cast else on_hit(mat, n, d, rng)
        if is_mixed(mat):
            mixed_hits += 1
        terms, count = [], F(0.0) if cast else F(1.0)
        for li in lights:
            with np.errstate(divide="ignore", invalid="ignore"):
                to = (ms.mids[li] - p).astype(F)
                rd = (to / np.sqrt(dot(to, to))).astype(F)
            sh = LC.closest(ms, p, rd, p1, pixel)
            shadow += 1
            shadow_inst += int(sh is not None and sh[0] >= n_top)
            if sh is None or sh[0] != ms.light_obj[li]:
                blocked[li] += int(sh is not None)
                continue
            reached[li] += 1
            _, el = ms.color(sh[0], sh[3])
            pdf = material_pdf(mat, p, n, d, time, p, rd, 0.0)
            s, dc = LC.light_term(not cast, pdf, el, sh[1], rd, ms.weight)
            if s is None:
                continue
            terms.append(s)
            count = F(count + dc)
        levels.append((m, e, terms, count))
        if cast:
            end_bg = False
            break
        o, d = p, scat
        if t_next is not None:
            time = t_next
    if full is not None and mixed_hits == 0:
        assert len(full) == queries, (len(full), queries)
    bg = ms.background
    n_l = len(lights)
    out = {"queries": queries, "hits": hits, "shadow": shadow, "mixed_hits": mixed_hits, "times": times, "bound": 0.0,
           "inst_hits": inst_hits, "shadow_inst": shadow_inst, "reached": reached, "blocked": blocked}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if cast:
            if not levels:
                out["ftb"], out["rec"] = bg.copy(), bg.copy()
                return out
            m, e, terms, count = levels[0]
            S = np.zeros(3, F)
            for s in terms:
                S = (S + s).astype(F)
            c = ((S * m).astype(F) / count).astype(F) if count != F(0.0) else np.zeros(3, F)
            out["ftb"] = (c + e).astype(F)
            out["rec"] = out["ftb"].copy()
            return out
        L, thr = np.zeros(3, F), np.ones(3, F)
        for m, e, terms, count in levels:
            S = np.zeros(3, F)
            for s in terms:
                S = (S + s).astype(F)
            L = (L + (thr * (((S * m).astype(F) / count).astype(F) + e).astype(F)).astype(F)).astype(F)
            thr = (thr * (m / count).astype(F)).astype(F)
        if end_bg:
            L = (L + (bg * thr).astype(F)).astype(F)
        c = bg.copy()
        for m, e, terms, count in reversed(levels):
            for s in terms:
                c = (c + s).astype(F)
            c = (((c * m).astype(F) / count).astype(F) + e).astype(F)
    D = max(1, len(levels))
    out["bound"] = ((n_l + 3) * D + (n_l + 4 + 2 * D)) * LC.U * 1.001       # lights_common.trace's rounding bound
    out["ftb"], out["rec"] = L, c
    return out


def render(ms, cam, params, check=False):
    """The restatement's frame (gamma 1, any sampler: lights_common.pixel_samples and lights_common.resolve, as lights_common.render):
    ([h][w][3] f32, segments = path + shadow queries, {"mixed_hits", "nonzero_time_queries", "time_reset", "max_rel" (front to back against
    the recursion, relative to its bound), "path_queries", "path_hits", "inst_hits", "shadow_inst", "reached" / "blocked" per light})."""
    assert params.sampler in LC.SAMPLERS and params.gamma == 1.0
    img = np.empty((params.height, params.width, 3), F)
    n_l = len(ms.lights)
    seg, info = 0, {"mixed_hits": 0, "nonzero_time_queries": 0, "time_reset": 0, "max_rel": 0.0, "path_queries": 0, "path_hits": 0,
                    "inst_hits": 0, "shadow_inst": 0, "reached": np.zeros(n_l, np.int64), "blocked": np.zeros(n_l, np.int64)}
    for j in range(params.height):
        for i in range(params.width):
            pixel = j * params.width + i
            cols = []
            for o, d, tm, rng in LC.pixel_samples(cam, params, i, j):
                r = trace(ms, o, d, params, pixel, check=check and rng is None, time=tm, rng=rng)
                cols.append(r["ftb"])
                seg += r["queries"] + r["shadow"]
                info["mixed_hits"] += r["mixed_hits"]
                info["nonzero_time_queries"] += sum(1 for t in r["times"] if t != 0.0)
                info["time_reset"] += int(bool(r["times"]) and r["times"][0] != 0.0 and any(t == 0.0 for t in r["times"][1:]))
                info["path_queries"] += r["queries"]
                info["path_hits"] += r["hits"]
                info["inst_hits"] += r["inst_hits"]
                info["shadow_inst"] += r["shadow_inst"]
                info["reached"] += np.asarray(r["reached"], np.int64)
                info["blocked"] += np.asarray(r["blocked"], np.int64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ok = np.isfinite(r["rec"]) & (r["rec"] != 0) & np.isfinite(r["ftb"])
                    if r["bound"] > 0 and ok.any():
                        rel = np.abs(r["ftb"][ok].astype(np.float64) - r["rec"][ok]) / np.abs(r["rec"][ok].astype(np.float64))
                        info["max_rel"] = max(info["max_rel"], float(rel.max() / r["bound"]))
            img[j, i] = LC.resolve(params, cols)
    return img, seg, info
