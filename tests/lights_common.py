"""Restatement of Rust2's light-biased integrators (Rust2/src/viewport/ray_color.rs:55-164, objects/material.rs material_pdf) in numpy f32,
on top of what the CPU oracle exposes -- the reference of tests/test_lights_cpu.py and tests/test_gpu_lights.py.

The oracle knows RTW_INTEGRATOR_RUST2 only.  Every closest hit used here, path or shadow, is the oracle's (a depth-1 rtw_oracle_trace_ray of
the ray: object, t, point, normal); Rust2's on_hit is restated over the oracle's exposed random stream and checked hop by hop against the
oracle's full RUST2 trace of the same camera ray, so the restated scatter is pinned to the oracle before anything new is judged by it.
Everything else -- light mid-points, material_pdf, the light loop, the combination -- is evaluated here, one f32 rounding per operation.

Association of the combination (DESIGN.md "Light-biased integrators"):
    recursion (the reference):  c = next; for every accepted light: c = c + s_i;  ret = (c (.) m) / count + e
    front to back (the device):  S = 0; S = S + s_i;  L = L + thr (.) ((S (.) m) / count + e);  thr = thr (.) (m / count)
"""
import ctypes as C
import json
import os

import numpy as np

import rtw_amd as R
from tests import oracle_binding as O

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rust2_light_scene.json")
MATS = {"lambertian": (0.0, 0.0, 1.0), "mirror": (1.0, 0.0, 1.0), "glass": (1.0, 1.0, 1.5)}
FRAC_1_PI = F(0.318309886183790671538)
U = 2.0 ** -24


def v(x):
    return np.asarray(x, dtype=F).reshape(3).copy()


def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def unit(a):
    return (a / np.sqrt(dot(a, a))).astype(F)


def veq(a, b):
    with np.errstate(invalid="ignore"):
        d = (a - b).astype(F)
        return bool(abs(d[0]) < F(1e-7) and abs(d[1]) < F(1e-7) and abs(d[2]) < F(1e-7))


def reflect(a, n):
    return (a - ((n * F(2.0)).astype(F) * dot(a, n)).astype(F)).astype(F)


def refract(uv, n, ratio):
    ct = dot(-uv, n)
    if ct > F(1.0):
        ct = F(1.0)
    perp = ((uv + (n * ct).astype(F)).astype(F) * ratio).astype(F)
    par = (n * F(-np.sqrt(F(abs(F(F(1.0) - dot(perp, perp))))))).astype(F)
    return (perp + par).astype(F)


def reflectance(cosine, ratio):
    r0 = F(F(F(1.0) - ratio) / F(F(1.0) + ratio))
    r0 = F(r0 * r0)
    x = F(F(1.0) - cosine)
    x2 = F(x * x)
    return F(r0 + F(F(F(1.0) - r0) * F(x * F(x2 * x2))))


def glass_parts(mat, n, din):
    front = not (dot(din, n) > F(0.0))
    nn = n if front else (-n).astype(F)
    ratio = F(F(1.0) / F(mat[2])) if front else F(mat[2])
    ud = unit(din)
    ct = dot(-ud, nn)
    if ct > F(1.0):
        ct = F(1.0)
    with np.errstate(invalid="ignore"):
        st = F(np.sqrt(F(F(1.0) - F(ct * ct))))
    return nn, ratio, ud, ct, bool(F(ratio * st) > F(1.0))


def material_pdf(mat, p, n, din, tm, ro, rd, rtm):
    """material_pdf(h, r): Lambertian material.rs:45-62, Mirror :93-99, MirrorGlass :199-232, selected as RTW_INTEGRATOR_RUST2 does."""
    mat = [F(x) for x in mat]
    if mat[1] > F(0.0):
        if not veq(ro, p):
            return F(0.0)
        nn, ratio, ud, ct, cannot = glass_parts(mat, n, din)
        refl = reflect(ud, nn)
        if cannot and veq(refl, rd):
            return F(1.0)
        rfl = reflectance(ct, ratio)
        if veq(refl, rd):
            return rfl
        if veq(refract(ud, nn, ratio), rd):
            return F(F(1.0) - rfl)
        return F(0.0)
    if mat[0] == F(1.0):
        return F(1.0) if (veq(ro, p) and veq(rd, reflect(din, n)) and F(rtm) == F(tm)) else F(0.0)
    if not veq(ro, p):
        return F(0.0)
    cos = dot(unit(rd), unit(n))
    c = F(-cos) if dot(din, n) >= F(0.0) else cos
    if c < F(0.0):
        c = F(0.0)
    if c > F(1.0):
        c = F(1.0)
    return F(c * FRAC_1_PI)


def light_term(biased, pdf, e, t, rd, w):
    """The term one accepted light adds (None: light_biased_ray_color skips it) and what it adds to count."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if biased:
            mx = e[0] if e[0] >= e[1] else e[1]
            mx = mx if mx >= e[2] else e[2]
            if pdf <= F(F(1.0) / F(F(255.0) * mx)):
                return None, F(0.0)
            d2 = F(F(t * t) * dot(rd, rd))
            return (((e * pdf).astype(F) / d2).astype(F) * F(w)).astype(F), F(w)
        d2 = F(F(t * t) * dot(rd, rd))
        return ((e * pdf).astype(F) / d2).astype(F), F(1.0)


def mid_sphere(c, r):
    c, r = v(c), F(r)
    a, b = (c - r).astype(F), (c + r).astype(F)
    return ((np.minimum(a, b) + np.maximum(a, b)).astype(F) * F(0.5)).astype(F)


def mid_quad(o, u, w):
    o, u, w = v(o), v(u), v(w)
    corners = [((o + u).astype(F) + w).astype(F), (o + w).astype(F), (o + u).astype(F), o]
    mn, mx = np.min(corners, axis=0).astype(F), np.max(corners, axis=0).astype(F)
    out = np.empty(3, F)
    for k in range(3):
        lo, hi = mn[k], mx[k]
        if F(hi - lo) < F(0.005):
            c = F(F(0.5) * F(hi + lo))
            hi, lo = F(c + F(F(0.005) * F(0.5))), F(c - F(F(0.005) * F(0.5)))
        out[k] = F(F(lo + hi) * F(0.5))
    return out


class LightScene:
    """A scene of top-level spheres and quads with what the restatement needs of it (materials, colours, emission) kept on the side."""

    def __init__(self, spheres, quads, lights, background=(0.0, 0.0, 0.0), textures=(), emission_images=None, weight=100.0):
        """spheres: dicts {origin, radius, material, color, emitted[, tex]}; quads: dicts {origin, u, v, material, color, emitted};
        lights: [(kind, index)]."""
        self.spheres, self.quads, self.lights, self.weight = list(spheres), list(quads), list(lights), float(weight)
        self.background = v(background)
        self.textures = [np.ascontiguousarray(t, dtype=F) for t in textures]
        self.emission_images = dict(emission_images or {})
        sp = []
        for s in self.spheres:
            mat = MATS[s["material"]] if isinstance(s["material"], str) else tuple(s["material"])
            if s.get("tex", -1) >= 0:
                x = R.Sphere.new_with_texture(s["origin"], s["radius"], (1.0, 1.0, 1.0), mat, s["tex"])
            else:
                x = R.Sphere.with_albedo(s["origin"], s["radius"], s["color"], mat)
            for k in range(3):
                x.pod.emitted[k] = float(s["emitted"][k])
                x.pod.velocity[k] = float(s.get("velocity", (0.0, 0.0, 0.0))[k])
            sp.append(x)
        qd = [R.Quad.new(q["origin"], q["u"], q["v"], MATS[q["material"]] if isinstance(q["material"], str) else tuple(q["material"]),
                         q["color"], q["emitted"]) for q in self.quads]
        self.scene = R.Scene(sp, textures=self.textures, background=background, quads=qd, emission_images=self.emission_images)
        self.mids = [mid_sphere(self.spheres[i]["origin"], self.spheres[i]["radius"]) if k == R.LIGHT_SPHERE else
                     mid_quad(self.quads[i]["origin"], self.quads[i]["u"], self.quads[i]["v"]) for k, i in self.lights]
        self.light_obj = [i if k == R.LIGHT_SPHERE else len(self.spheres) + i for k, i in self.lights]

    def mat(self, obj):
        d = self.spheres[obj] if obj < len(self.spheres) else self.quads[obj - len(self.spheres)]
        return MATS[d["material"]] if isinstance(d["material"], str) else tuple(d["material"])

    def color(self, obj, normal):
        """ColorResult{multiplied, emmited} of top-level object `obj` for a hit with outward normal `normal`."""
        if obj >= len(self.spheres):
            q = self.quads[obj - len(self.spheres)]
            return v(q["color"]), v(q["emitted"])
        s = self.spheres[obj]
        if s.get("tex", -1) < 0:
            return v(s["color"]), v(s["emitted"])
        # Rust2's ImageTexture::color_at through the device's UV sequences (the oracle's restatement of them)
        nn = np.ascontiguousarray(normal, F).reshape(1, 3)
        out = np.empty((1, 4), F)
        O.lib().rtw_oracle_sphere_uv(nn.ctypes.data_as(C.POINTER(C.c_float)), 1, 1, out.ctypes.data_as(C.POINTER(C.c_float)))
        uu, vv = float(out[0, 2]), float(out[0, 3])
        img = self.textures[s["tex"]]
        h, w = img.shape[0], img.shape[1]
        m = img.reshape(-1, 3)[O.lib().rtw_oracle_rust2_texel_index(uu, vv, w, h, 0)].copy()
        e = v(s["emitted"])
        if s["tex"] in self.emission_images:
            ei = self.textures[self.emission_images[s["tex"]]]
            e = ei.reshape(-1, 3)[O.lib().rtw_oracle_rust2_texel_index(uu, vv, ei.shape[1], ei.shape[0], 1)].copy()
        return m.astype(F), e.astype(F)

    def params(self, width, height, integrator, depth, seed=1, sampler=None, samples=1, mint=0.001, maxt=1000.0, gamma=1.0, accel=None):
        p = R.RtwParams()
        p.width, p.height, p.samples, p.depth = width, height, samples, depth
        p.gamma, p.mint, p.maxt = gamma, mint, maxt
        p.integrator = integrator
        p.sampler = R.SAMPLER_NO_RAND if sampler is None else sampler
        p.accel = R.ACCEL_BRUTE if accel is None else accel
        p.seed = seed
        p.row_block, p.part_index, p.part_count = 8, 0, 1
        return p


def golden(weight=None):
    g = json.load(open(GOLDEN))
    kinds = {"sphere": R.LIGHT_SPHERE, "quad": R.LIGHT_QUAD}
    ls = LightScene(g["spheres"], g["quads"], [(kinds[l["kind"]], l["index"]) for l in g["lights"]], g["background"],
                    weight=g["biased_weight"] if weight is None else weight)
    return ls, g


def mirror_glass_scene():
    ls, g = golden()
    sp = g["spheres"] + [
        {"origin": [0.9, -1.2, 3.6], "radius": 0.6, "material": "glass", "color": [1.0, 1.0, 1.0], "emitted": [0.0, 0.0, 0.0]},
        {"origin": [-1.0, -1.4, 3.0], "radius": 0.5, "material": "mirror", "color": [0.9, 0.9, 0.9], "emitted": [0.0, 0.0, 0.0]}]
    return LightScene(sp, g["quads"], ls.lights, g["background"], weight=g["biased_weight"]), g


def camera(g, width, height):
    c = g["camera"]
    return R.camera2_new(width / height, c["origin"], c["vup"], c["direction"], c["vfov"], c["lens_radius"])


def camera_no_rand(g, width, height):
    """Rust/'s Viewport::new_from_res camera (per-pixel deltas, what RTW_SAMPLER_NO_RAND reads) at the golden camera's place."""
    c = g["camera"]
    return R.Viewport.new_from_res(width, height, 1, 1, 1.0, vfov=c["vfov"], origin=c["origin"], direction=c["direction"], vup=c["vup"]).camera()


def camera_ray(cam, i, j):
    """RTW_SAMPLER_NO_RAND's ray of pixel (i, j): origin, (pixel00 + delta_u * i) + delta_v * j."""
    o, p00, du, dv = v(list(cam.origin)), v(list(cam.pixel00)), v(list(cam.delta_u)), v(list(cam.delta_v))
    d = ((p00 + (du * F(i)).astype(F)).astype(F) + (dv * F(j)).astype(F)).astype(F)
    return o, d


class Rng:
    def __init__(self, seed, pixel, sample=0):
        self.state = (C.c_uint32 * 2)()
        O.lib().rtw_oracle_rng_seed(seed, pixel, sample, self.state)

    def next(self):
        return F(O.lib().rtw_oracle_rng_next(self.state))


def random_unit_vec(rng):
    while True:
        p = np.array([F(F(rng.next() * F(2.0)) + F(-1.0)) for _ in range(3)], F)
        if dot(p, p) <= F(1.0):
            return unit(p)


def on_hit(mat, n, din, rng):
    """Rust2's Material::on_hit direction (material.rs:27-35, 77-83, 132-162) over the oracle's stream."""
    mat = [F(x) for x in mat]
    if mat[1] > F(0.0):
        nn, ratio, ud, ct, cannot = glass_parts(mat, n, din)
        rfl = reflectance(ct, ratio)
        do_reflect = cannot
        if not do_reflect:
            do_reflect = bool(rfl > rng.next())
        return reflect(ud, nn) if do_reflect else refract(ud, nn, ratio)
    if mat[0] == F(1.0):
        return reflect(din, n)
    return unit((n + random_unit_vec(rng)).astype(F))


def closest(ls, o, d, p1, pixel, time=0.0):
    """The oracle's closest hit of the ray at ray.time `time` (a depth-1 RUST2 trace): None, or (object, t, point, normal)."""
    b, _ = O.trace_ray(o, d, time, ls.scene, p1, pixel, 0, cap=4)
    assert len(b) == 1
    if not b[0].hit:
        return None
    return b[0].sphere, F(b[0].t), v(list(b[0].point)), v(list(b[0].normal))


def trace(ls, o, d, params, pixel, check=True, time=0.0, rng=None):
    """One camera ray under params.integrator (LIGHT_CAST / LIGHT_BIASED): {"ftb": front-to-back colour (what the device computes), "rec": the
    reference's recursion, "queries": path queries, "hits": path hits, "bound": the rounding bound between the two forms}.  check: assert hop
    by hop that the restated scatter reproduces the oracle's full RUST2 trace of the same ray.  `time`: the path's ray.time (the shadow rays
    run at time 0 whatever it is); `rng`: the pixel's stream after the sampler's camera draws (default: a fresh one, RTW_SAMPLER_NO_RAND) --
    the full trace starts on a fresh stream, so check needs rng None.  "blocked": shadow queries whose closest hit was another object, per
    light."""
    assert rng is None or not check
    time = float(F(time))
    biased = params.integrator == R.INTEGRATOR_LIGHT_BIASED
    depth = params.depth if biased else 1
    p1 = R.RtwParams.from_buffer_copy(params)
    p1.integrator, p1.depth = R.INTEGRATOR_RUST2, 1
    full = None
    if check and biased:
        pf = R.RtwParams.from_buffer_copy(params)
        pf.integrator = R.INTEGRATOR_RUST2
        full, _ = O.trace_ray(o, d, time, ls.scene, pf, pixel, 0, cap=max(4, depth + 2))
    rng = Rng(params.seed, pixel) if rng is None else rng
    levels, queries, hits = [], 0, 0
    blocked = [0] * len(ls.lights)
    end_bg = True                                   # the path ends on the background (miss or depth)
    o, d = v(o), v(d)
    for k in range(depth):
        h = closest(ls, o, d, p1, pixel, time)
        queries += 1
        if full is not None:
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
        mat = ls.mat(obj)
        m, e = ls.color(obj, n)
        scat = on_hit(mat, n, d, rng) if biased else None
        terms, count = [], F(1.0) if biased else F(0.0)
        for li in range(len(ls.lights)):
            with np.errstate(divide="ignore", invalid="ignore"):
                to = (ls.mids[li] - p).astype(F)
                rd = (to / np.sqrt(dot(to, to))).astype(F)
            sh = closest(ls, p, rd, p1, pixel)
            if sh is None or sh[0] != ls.light_obj[li]:
                blocked[li] += int(sh is not None)
                continue
            _, el = ls.color(sh[0], sh[3])
            pdf = material_pdf(mat, p, n, d, time, p, rd, 0.0)
            s, dc = light_term(biased, pdf, el, sh[1], rd, ls.weight)
            if s is None:
                continue
            terms.append(s)
            count = F(count + dc)
        levels.append((m, e, terms, count))
        if not biased:
            end_bg = False
            break
        o, d = p, scat
    if full is not None:
        assert len(full) == queries, (len(full), queries)
    bg = ls.background
    n_l = len(ls.lights)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if not biased:
            if not levels:
                return {"ftb": bg.copy(), "rec": bg.copy(), "queries": queries, "hits": hits, "bound": 0.0, "blocked": blocked}
            m, e, terms, count = levels[0]
            S = np.zeros(3, F)
            for s in terms:
                S = (S + s).astype(F)
            c = ((S * m).astype(F) / count).astype(F) if count != F(0.0) else np.zeros(3, F)
            out = (c + e).astype(F)
            return {"ftb": out, "rec": out.copy(), "queries": queries, "hits": hits, "bound": 0.0, "blocked": blocked}
        # front to back
        L, thr = np.zeros(3, F), np.ones(3, F)
        for m, e, terms, count in levels:
            S = np.zeros(3, F)
            for s in terms:
                S = (S + s).astype(F)
            L = (L + (thr * (((S * m).astype(F) / count).astype(F) + e).astype(F)).astype(F)).astype(F)
            thr = (thr * (m / count).astype(F)).astype(F)
        if end_bg:
            L = (L + (bg * thr).astype(F)).astype(F)
        # the reference's recursion
        c = bg.copy()
        for m, e, terms, count in reversed(levels):
            for s in terms:
                c = (c + s).astype(F)
            c = (((c * m).astype(F) / count).astype(F) + e).astype(F)
    # Rounding bound between the two forms (every term is >= 0, so relative errors only add up): a term reaches the result through at most
    # (n_l + 3) roundings per level in the recursion (n_l additions, the product, the quotient, + e: (n_l + 3) D over D levels), and front to
    # back a term of level k through n_l + 5 of its own (the sum S, the product, the quotient, + e, the product with thr, its addition to L),
    # 2 k in thr (m / count and the product, per earlier level) and D - k later additions to L (the background's included):
    # n_l + 5 + D + k <= n_l + 4 + 2 D.  count is the same number in both forms.  Each rounding is at most 2^-24 relative, so the forms differ
    # by at most ((n_l + 3) D + n_l + 4 + 2 D) 2^-24 of the value (1.001: the second-order terms).
    D = max(1, len(levels))
    bound = ((n_l + 3) * D + (n_l + 4 + 2 * D)) * U * 1.001
    return {"ftb": L, "rec": c, "queries": queries, "hits": hits, "bound": bound, "blocked": blocked}


SUM_CHUNK = 4            # RTW_SUM_CHUNK (rtw.h)
SAMPLERS = (R.SAMPLER_NO_RAND, R.SAMPLER_ROW, R.SAMPLER_STRATIFIED, R.SAMPLER_CENTRES)


def sampler_count(sampler, samples):
    """(rays per pixel, s_root) of a sampler (oracle/rtw_oracle.c sampler_count): STRATIFIED rounds sqrt(samples) up, CENTRES down."""
    if sampler == R.SAMPLER_STRATIFIED:
        root = int(np.ceil(np.sqrt(F(samples))))
        return root * root, root
    if sampler == R.SAMPLER_CENTRES:
        root = int(np.floor(np.sqrt(F(samples))))
        return root * root, root
    return (1 if sampler == R.SAMPLER_NO_RAND else samples), 0


def pixel_samples(cam, params, i, j):
    """The camera rays of pixel (i, j), in sample order, as oracle/rtw_oracle.c render_pixel draws them: (origin, direction, ray.time, the
    sample's stream (seed, pixel, s) after the camera draws -- None under RTW_SAMPLER_NO_RAND, whose path starts on the fresh stream).  Every
    sampler but NO_RAND draws a lens-disk point first (random_in_unit_disk: (2 xi - 1, 2 xi - 1), accept len2 <= 1); lens_radius must be 0, so
    the point moves nothing.  ROW (render_row, viewport.rs:286-297): two pixel offsets and the ray's time; STRATIFIED (viewport.rs:452-470):
    cell x = s / root, y = s % root, an offset in each, time 0; CENTRES (Rust2 viewport.rs:92-104): the cell centres over Rust2's camera
    (pixel00 = left_top, delta_u / delta_v the FULL viewport, divided by width / height at use), time 0."""
    if params.sampler == R.SAMPLER_NO_RAND:
        o, d = camera_ray(cam, i, j)
        yield o, d, 0.0, None
        return
    assert cam.lens_radius == 0.0
    n, root = sampler_count(params.sampler, params.samples)
    pixel = j * params.width + i
    o, p00, du, dv = v(list(cam.origin)), v(list(cam.pixel00)), v(list(cam.delta_u)), v(list(cam.delta_v))
    for s in range(n):
        rng = Rng(params.seed, pixel, s)
        while True:
            x, y = F(F(rng.next() * F(2.0)) - F(1.0)), F(F(rng.next() * F(2.0)) - F(1.0))
            if F(F(x * x) + F(y * y)) <= F(1.0):
                break
        tm = F(0.0)
        if params.sampler == R.SAMPLER_ROW:
            jx, jy = F(F(i) + rng.next()), F(F(j) + rng.next())
            tm = F(F(cam.time0) + F(F(cam.shutter) * rng.next()))
        elif params.sampler == R.SAMPLER_STRATIFIED:
            jx = F(F(i) + F(F(F(s // root) + rng.next()) / F(root)))
            jy = F(F(j) + F(F(F(s % root) + rng.next()) / F(root)))
        else:
            jx = F(F(F(i) + F(F(F(s // root) + F(0.5)) / F(root))) / F(params.width))
            jy = F(F(F(j) + F(F(F(s % root) + F(0.5)) / F(root))) / F(params.height))
        d = ((p00 + (du * jx).astype(F)).astype(F) + (dv * jy).astype(F)).astype(F)
        yield o.copy(), d, tm, rng


def resolve(params, cols):
    """The driver's pixel: the samples added from +0 left to right and divided by their number (viewport.rs:299-301) -- or, with
    RTW_FLAG_CHUNK_SUMS, the samples of each chunk of RTW_SUM_CHUNK added left to right into a partial sum (starting from the chunk's first
    sample, not from 0) and the partial sums added from +0 in chunk order (rtw.h)."""
    acc = np.zeros(3, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if params.flags & R.FLAG_CHUNK_SUMS:
            for k in range(0, len(cols), SUM_CHUNK):
                part = np.asarray(cols[k], F).copy()
                for c in cols[k + 1:k + SUM_CHUNK]:
                    part = (part + c).astype(F)
                acc = (acc + part).astype(F)
        else:
            for c in cols:
                acc = (acc + c).astype(F)
        return (acc / F(len(cols))).astype(F)


def render(ls, cam, params, check=False):
    """The restatement's frame at gamma 1 under any sampler (pixel_samples: the oracle's camera draws, stream (seed, pixel, s) per sample;
    resolve: the driver's sum): ([h][w][3] f32, segments = path queries + n_lights * path hits, shadow queries blocked by another object per
    light).  check (RTW_SAMPLER_NO_RAND only): the hop-by-hop check of trace."""
    assert params.sampler in SAMPLERS and params.gamma == 1.0
    img = np.empty((params.height, params.width, 3), F)
    seg, blocked = 0, np.zeros(len(ls.lights), np.int64)
    for j in range(params.height):
        for i in range(params.width):
            pixel = j * params.width + i
            cols = []
            for o, d, tm, rng in pixel_samples(cam, params, i, j):
                r = trace(ls, o, d, params, pixel, check=check and rng is None, time=tm, rng=rng)
                cols.append(r["ftb"])
                seg += r["queries"] + len(ls.lights) * r["hits"]
                blocked += np.asarray(r["blocked"], np.int64)
            img[j, i] = resolve(params, cols)
    return img, seg, blocked


def sphere_field(g, n=60, seed=9):
    """The golden scene's sphere list with a field of n small spheres (Lambertian, mirror, glass in turn) on the floor of the box added: more
    than the 48 spheres up to which a BVH request walks the list.  The scene of the list-walk == tree test and of scripts/measure_lights.py."""
    rng = np.random.default_rng(seed)
    sp = list(g["spheres"])
    for k in range(n):
        sp.append({"origin": [float(rng.uniform(-1.8, 1.8)), float(rng.uniform(-1.9, -0.5)), float(rng.uniform(1.5, 4.8))],
                   "radius": float(rng.uniform(0.05, 0.18)), "material": ["lambertian", "mirror", "glass"][k % 3],
                   "color": [float(x) for x in rng.uniform(0.3, 1.0, 3)], "emitted": [0.0, 0.0, 0.0]})
    return sp
