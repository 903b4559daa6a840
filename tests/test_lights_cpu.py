"""Rust2's light-biased integrators, the parts that need no GPU: the host entry points (rtw_light_mid, rtw_material_pdf, rtw_light_term:
the definitions the kernels compile) against the numpy restatement of tests/lights_common.py bit for bit, known answers worked by hand from
the Rust source, the restatement's own self-checks against the frozen oracle, and the argument checks of the light interface."""
import ctypes as C

import numpy as np

import rtw_amd as R
from tests import lights_common as LC

F = np.float32


def bits(x):
    return np.asarray(x, F).tobytes()


def test_constants_and_abi():
    assert (R.INTEGRATOR_LIGHT_CAST, R.INTEGRATOR_LIGHT_BIASED) == (5, 6)
    assert R.lib().rtw_abi_version() == 4
    assert C.sizeof(R.RtwLight) == 8


def test_light_mid_matches_the_restatement():
    rng = np.random.default_rng(5)
    spheres, quads = [], []
    for _ in range(200):
        spheres.append({"origin": rng.uniform(-5, 5, 3).astype(F), "radius": F(rng.uniform(-1, 2)), "material": "lambertian",
                        "color": (1, 1, 1), "emitted": (1, 1, 1)})
        u, w = rng.uniform(-3, 3, 3).astype(F), rng.uniform(-3, 3, 3).astype(F)
        k = rng.integers(0, 4)
        if k < 3:                       # axis-aligned quads have a thin axis (the 0.005 rule)
            u[k] = 0.0
            w[k] = 0.0
        quads.append({"origin": rng.uniform(-5, 5, 3).astype(F), "u": u, "v": w, "material": "lambertian", "color": (1, 1, 1), "emitted": (1, 1, 1)})
    ls = LC.LightScene(spheres, quads, [])
    for i, s in enumerate(spheres):
        assert bits(R.light_mid(ls.scene, (R.LIGHT_SPHERE, i))) == bits(LC.mid_sphere(s["origin"], s["radius"]))
    for i, q in enumerate(quads):
        assert bits(R.light_mid(ls.scene, (R.LIGHT_QUAD, i))) == bits(LC.mid_quad(q["origin"], q["u"], q["v"]))


def test_light_mid_known_answers():
    ls, g = LC.golden()
    # the 0.2 x 0.2 light quad at z = 4.5: centre (0, 0), the thin z axis widened about 4.5
    assert np.allclose(R.light_mid(ls.scene, (R.LIGHT_QUAD, 1)), (0.0, 0.0, 4.5), atol=1e-6)
    assert np.allclose(R.light_mid(ls.scene, (R.LIGHT_SPHERE, 0)), (-0.4, 0.0, 4.5), atol=1e-6)


def random_hit(rng, kind):
    n = LC.unit(rng.normal(size=3).astype(F))
    din = rng.normal(size=3).astype(F) * F(rng.uniform(0.2, 3.0))
    if rng.random() < 0.5:                       # both face orientations
        din = -din
    p = rng.uniform(-4, 4, 3).astype(F)
    mat = {0: (0.0, 0.0, 1.0), 1: (1.0, 0.0, 1.0), 2: (1.0, 1.0, float(F(rng.uniform(1.1, 2.0))))}[kind]
    return mat, p, n, din.astype(F)


def test_material_pdf_matches_the_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    n_one = 0
    for it in range(3000):
        kind = it % 3
        mat, p, n, din = random_hit(rng, kind)
        rd = LC.unit(rng.normal(size=3).astype(F))
        ro, tm, rtm = p, 0.0, 0.0
        r = rng.random()
        if kind == 1 and r < 0.3:
            rd = LC.reflect(din, n)                                   # the mirror direction itself (un-normalised)
        elif kind == 2 and r < 0.3:
            nn, ratio, ud, ct, cannot = LC.glass_parts([F(x) for x in mat], n, din)
            rd = LC.reflect(ud, nn) if r < 0.15 else LC.refract(ud, nn, ratio)
        elif r > 0.9:
            ro = (p + F(1e-3)).astype(F)                              # another origin: 0
        elif r > 0.85:
            rtm = 0.25                                                # another time: only Mirror's derived PartialEq looks at it
        a = R.material_pdf(mat, p, n, din, tm, ro, rd, rtm)
        b = LC.material_pdf(mat, p, n, din, tm, ro, rd, rtm)
        assert bits(a) == bits(b), (it, kind, a, b)
        n_one += int(a > 0)
    assert n_one > 1000


def test_material_pdf_known_answers():
    p, n = (1.0, 2.0, 3.0), (0.0, 0.0, 1.0)
    # Lambertian at normal incidence: cos = 1 -> FRAC_1_PI; from the back side the cosine is negated
    assert R.material_pdf((0, 0, 1), p, n, (0, 0, -1), 0.0, p, (0, 0, 1), 0.0) == LC.FRAC_1_PI
    assert R.material_pdf((0, 0, 1), p, n, (0, 0, 1), 0.0, p, (0, 0, 1), 0.0) == 0.0
    assert R.material_pdf((0, 0, 1), p, n, (0, 0, 1), 0.0, p, (0, 0, -1), 0.0) == LC.FRAC_1_PI
    assert R.material_pdf((0, 0, 1), p, n, (0, 0, -1), 0.0, (1.0, 2.0, 3.1), (0, 0, 1), 0.0) == 0.0      # r.origin != h.p
    # Mirror: d = (1, 0, -1) reflects about z to (1, 0, 1) -- un-normalised; within 1e-7 is 1, just outside is 0; the time is compared exactly
    assert R.material_pdf((1, 0, 1), p, n, (1, 0, -1), 0.0, p, (1, 0, 1), 0.0) == 1.0
    assert R.material_pdf((1, 0, 1), p, n, (1, 0, -1), 0.0, p, (1.0, 5e-8, 1.0), 0.0) == 1.0
    assert R.material_pdf((1, 0, 1), p, n, (1, 0, -1), 0.0, p, (1.0, 2e-7, 1.0), 0.0) == 0.0
    assert R.material_pdf((1, 0, 1), p, n, (1, 0, -1), 0.5, p, (1, 0, 1), 0.0) == 0.0
    s = float(np.sqrt(F(0.5)))
    assert R.material_pdf((1, 0, 1), p, n, (1, 0, -1), 0.0, p, (s, 0, s), 0.0) == 0.0                      # the unit direction is not the mirror's ray
    # MirrorGlass at normal incidence, ir 1.5: reflect (0,0,1) has Schlick r0 = ((1 - 1/1.5) / (1 + 1/1.5))^2, refract (0,0,-1) the rest
    r0 = LC.reflectance(F(1.0), F(F(1.0) / F(1.5)))
    assert abs(float(r0) - 0.04) < 1e-6
    assert R.material_pdf((1, 1, 1.5), p, n, (0, 0, -2), 0.0, p, (0, 0, 1), 0.0) == r0
    assert R.material_pdf((1, 1, 1.5), p, n, (0, 0, -2), 0.0, p, (0, 0, -1), 0.0) == F(F(1.0) - r0)
    assert R.material_pdf((1, 1, 1.5), p, n, (0, 0, -2), 0.0, p, (0, 1, 0), 0.0) == 0.0
    # total internal reflection from inside (d . n > 0, ratio 1.5, sin > 1 / 1.5): the mirror direction has pdf 1
    din = LC.v((0.9, 0.0, 0.4358899))
    ud = LC.unit(din)
    assert R.material_pdf((1, 1, 1.5), p, n, din, 0.0, p, LC.reflect(ud, -LC.v(n)), 0.0) == 1.0


def test_light_term_matches_the_restatement_and_the_threshold_is_inclusive():
    rng = np.random.default_rng(3)
    for it in range(2000):
        biased = it % 2 == 0
        integ = R.INTEGRATOR_LIGHT_BIASED if biased else R.INTEGRATOR_LIGHT_CAST
        e = rng.uniform(0, 5, 3).astype(F)
        pdf, t, w = F(rng.uniform(0, 0.32)), F(rng.uniform(0.1, 6)), F(rng.choice([0.0, 1.0, 100.0]))
        if it % 7 == 0:
            pdf = F(0.0)
        rd = LC.unit(rng.normal(size=3).astype(F))
        S0, c0 = rng.uniform(0, 2, 3).astype(F), F(1.0 + it % 3)
        added, S, c = R.light_term(integ, pdf, e, t, rd, w, S0, c0)
        s, dc = LC.light_term(biased, pdf, e, t, rd, w)
        assert added == (s is not None)
        if s is None:
            assert bits(S) == bits(S0) and c == c0
        else:
            assert bits(S) == bits((S0 + s).astype(F)) and bits(c) == bits(F(c0 + dc)), it
    # exactly at pdf == 1 / (255 max e): skipped (`<=`); one ulp above: taken
    e = LC.v((0.5, 2.0, 1.0))
    thr = F(F(1.0) / F(F(255.0) * F(2.0)))
    z = np.zeros(3, F)
    assert R.light_term(R.INTEGRATOR_LIGHT_BIASED, thr, e, 1.0, (0, 0, 1), 100.0, z, 1.0)[0] is False
    added, S, c = R.light_term(R.INTEGRATOR_LIGHT_BIASED, np.nextafter(thr, F(1.0)), e, 1.0, (0, 0, 1), 100.0, z, 1.0)
    assert added and c == 101.0
    # light_biased_ray_cast has no such test and counts a light whose pdf is 0
    added, S, c = R.light_term(R.INTEGRATOR_LIGHT_CAST, 0.0, e, 1.0, (0, 0, 1), 100.0, z, 0.0)
    assert added and c == 1.0 and not S.any()
    # a light that emits nothing: 1 / 0 = inf is the threshold, always skipped
    assert R.light_term(R.INTEGRATOR_LIGHT_BIASED, 0.3, (0, 0, 0), 1.0, (0, 0, 1), 100.0, z, 1.0)[0] is False


def check_frame(ls, g, w, h, depth, seeds):
    """Self-checks of the restatement on a w x h frame: hop by hop against the oracle's full trace (inside trace), and front to back against the
    recursion within the rounding bound.  Returns the largest observed |rec - ftb| / max as a multiple of 2^-24."""
    cam = LC.camera_no_rand(g, w, h)
    worst, lit = 0.0, 0
    for seed in seeds:
        p = ls.params(w, h, R.INTEGRATOR_LIGHT_BIASED, depth, seed=seed)
        for j in range(h):
            for i in range(w):
                o, d = LC.camera_ray(cam, i, j)
                r = LC.trace(ls, o, d, p, j * w + i, check=True)
                a, b = r["ftb"].astype(np.float64), r["rec"].astype(np.float64)
                assert np.isfinite(a).all() and np.isfinite(b).all()
                m = np.maximum(a, b)
                assert (np.abs(a - b) <= r["bound"] * m).all(), (seed, i, j, a, b, r["bound"])
                if m.max() > 0:
                    worst = max(worst, float((np.abs(a - b) / np.where(m > 0, m, 1)).max()) / LC.U)
                lit += int(a.max() > 0)
    assert lit > 0
    return worst


def test_restatement_self_check_golden_scene():
    ls, g = LC.golden()
    worst = check_frame(ls, g, 16, 12, 9, (1, 2))
    print(f"golden scene: max |recursion - front to back| = {worst:.2f} x 2^-24 of the value")


def test_restatement_self_check_mirror_and_glass():
    ls, g = LC.mirror_glass_scene()
    worst = check_frame(ls, g, 16, 12, 9, (3,))
    print(f"mirror + glass: max |recursion - front to back| = {worst:.2f} x 2^-24 of the value")


def test_weight_zero_and_no_lights_are_the_rust2_path():
    """The identities the GPU tests tie to the oracle: with biased_weight 0 every term is e * pdf / d2 * 0 -- no inf * 0 on the golden scene --
    and count stays 1, so the restatement's colour is the oracle's RUST2 colour of the same ray bit for bit; likewise without lights."""
    from tests import oracle_binding as O
    _, g = LC.golden()
    w, h = 16, 12
    cam = LC.camera_no_rand(g, w, h)
    for ls in (LC.golden(weight=0.0)[0], LC.LightScene(g["spheres"], g["quads"], [], g["background"])):
        p = ls.params(w, h, R.INTEGRATOR_LIGHT_BIASED, 9, seed=4)
        pr = R.RtwParams.from_buffer_copy(p)
        pr.integrator = R.INTEGRATOR_RUST2
        for j in range(h):
            for i in range(w):
                o, d = LC.camera_ray(cam, i, j)
                r = LC.trace(ls, o, d, p, j * w + i)
                _, rgb = O.trace_ray(o, d, 0.0, ls.scene, pr, j * w + i, 0, cap=16)
                assert np.isfinite(r["ftb"]).all()
                assert np.array_equal(r["ftb"], rgb), (i, j, r["ftb"], rgb)


def test_light_list_argument_checks_without_a_device():
    """rtw_lights_validate runs the argument checks rtw_ctx_set_lights applies to a light list (one shared function in the library) and needs
    no context.  rtw_ctx_set_lights itself needs a device for its context: its own calls, the NULL / n mismatch included, are in
    tests/test_gpu_lights.py::test_set_lights_raw_argument_checks; here a NULL context is all that can be passed to it."""
    L = R.lib()
    ls, _ = LC.golden()
    sc = C.byref(ls.scene.pod)
    one = (R.RtwLight * 1)(R.RtwLight(R.LIGHT_QUAD, 0))
    assert L.rtw_lights_validate(sc, None, 0) == 0                         # the legal clear
    assert L.rtw_lights_validate(sc, one, 1) == 0
    assert L.rtw_lights_validate(sc, None, 1) == -1                        # NULL with n = 1
    assert L.rtw_lights_validate(sc, one, 0) == -1                         # a list with n = 0
    assert L.rtw_lights_validate(None, one, 1) == -1
    assert L.rtw_lights_validate(sc, (R.RtwLight * 1)(R.RtwLight(2, 0)), 1) == -1                  # kind out of range
    assert L.rtw_lights_validate(sc, (R.RtwLight * 1)(R.RtwLight(R.LIGHT_SPHERE, 1)), 1) == -1     # index beyond the scene
    assert L.rtw_lights_validate(sc, (R.RtwLight * 1)(R.RtwLight(R.LIGHT_QUAD, 6)), 1) == -1
    assert L.rtw_lights_validate(sc, (R.RtwLight * 2)(R.RtwLight(R.LIGHT_QUAD, 5), R.RtwLight(R.LIGHT_SPHERE, 0)), 2) == 0
    assert L.rtw_lights_validate(sc, (R.RtwLight * 16)(), 16) == 0 and L.rtw_lights_validate(sc, (R.RtwLight * 17)(), 17) == -1
    assert L.rtw_ctx_set_lights(None, one, 1, 100.0) == -1 and L.rtw_mgpu_set_lights(None, one, 1, 100.0) == -1    # no context
    out = (C.c_float * 3)()
    assert L.rtw_light_mid(sc, (R.RtwLight * 1)(R.RtwLight(2, 0)), out) == -1
    assert L.rtw_light_mid(sc, (R.RtwLight * 1)(R.RtwLight(R.LIGHT_QUAD, 6)), out) == -1
    assert L.rtw_light_mid(sc, (R.RtwLight * 1)(R.RtwLight(R.LIGHT_QUAD, 5)), out) == 0
    assert L.rtw_light_mid(None, one, out) == -1 and L.rtw_light_mid(sc, None, out) == -1
    z = (C.c_float * 3)()
    cnt = C.c_float(1.0)
    assert L.rtw_light_term(R.INTEGRATOR_RUST2, 0.1, z, 1.0, z, 1.0, z, C.byref(cnt)) == -1
