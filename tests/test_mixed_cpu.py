"""Rust2's MixedMaterial without a GPU: the host entry points (rtw_mixed_dir, rtw_mixed_pdf, rtw_pow_plain / rtw_sin_plain / rtw_cos_plain --
the definitions the kernels compile, csrc/rtw_mixed.h) against the numpy restatement of tests/mixed_common.py bit for bit; the error of the
three elementary functions against f64 over the arguments a render can produce (the figures of DESIGN.md 4.7); the distribution on_hit
draws from and the integral of material_pdf, both from the reference's stated pdf cos^exp (exp + 1) / 2 pi; the validation returns; the
reference's recursion against the device's front-to-back form on the golden scene."""
import numpy as np
import pytest

import rtw_amd as R
from tests import lights_common as LC
from tests import mixed_common as MC

F = np.float32
E_INVALID, E_UNSUPPORTED = -1, -5                       # rtw.h
UP = np.nextafter(F(1.0), F(2.0))
# maximum error in ulp against f64
POW_GEN = {0.5: 0.90, 0.25: 0.89, 1.0 / 11.0: 0.89}     # bases 1 - xi, all 2^24 stream values, at gen_exp = 1 / (exp + 1), exp = 1, 3, 10
POW_EXP = {1.0: 0.0, 3.0: 0.92, 10.0: 1.05}             # cosines in [0, 1]
SIN_ULP, COS_ULP = 1.44, 1.43                           # phi = (xi * 2) * PI, all 2^24 stream values


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def ulps(got, ref):
    """|got - ref| in units of the f32 ulp of ref's binade (ref in f64)."""
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(ref), 1e-300)))
    u = np.maximum(2.0 ** (e - 23.0), 2.0 ** -149)
    return np.abs(got.astype(np.float64) - ref) / u


def test_python_surface():
    assert R.FLAG_MIXED_MATERIAL == 32 and R.mixed(3) == (0.0, -1.0, 3.0)
    vp = R.Viewport.new_from_res(8, 6, 1, 3, 1.0)
    assert vp.params().flags == 0
    vp.flags = R.FLAG_MIXED_MATERIAL
    assert vp.params(R.INTEGRATOR_RUST2).flags == R.FLAG_MIXED_MATERIAL
    ms, g = MC.golden()
    assert g["quads"][0]["material"] == "mixed" and g["quads"][0]["exp"] == 3.0 and g["quads"][2]["exp"] == 1.0
    assert ms.scene._quads[0].opacity < 0 and ms.scene._quads[0].ir == 3.0 and ms.has_mixed()


# ---- host functions == the restatement, bit for bit -------------------------------------------------------------------------------------
# The argument sets of the tests below, as functions: tests/test_gpu_device_math.py runs the device compile of the same functions on them.
POW_SPECIAL_X = np.array([0.0, -0.0, 1.0, UP, 1.0000005, np.inf, np.nan, 1e-40, 1.4e-45, 2.0, 3.0e38, 0.99999994, 0.5, 0.70710677, 0.7071068], F)
POW_SPECIAL_Y = (0.0, 0.5, 1.0, 3.0, 10.0, 1.0 / 11.0, 1e-30, 127.0, 3.0e38)


def elementary_arguments():
    """(x, y) for pow_plain and phi for sin_plain / cos_plain: random, near 1, through the subnormals; the quadrant ends and tiny angles."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(300000), 1.0 - rng.random(100000) * 1e-5, 2.0 ** rng.uniform(-149, 4, 100000)]).astype(F)
    y = np.concatenate([rng.random(250000) * 12.0, 1.0 / (1.0 + rng.integers(0, 40, 250000))]).astype(F)
    phi = np.concatenate([rng.random(400000) * 2 * np.pi, np.arange(5) * (np.pi / 2), [2 * np.pi, np.nan, 1e-30, 1.4e-45]]).astype(F)
    return x, y, phi


def test_elementary_functions_equal_the_restatement():
    x, y, phi = elementary_arguments()
    assert same_bits(R.pow_plain(x, y), MC.pow_plain(x, y))
    sx = POW_SPECIAL_X
    for yy in POW_SPECIAL_Y:
        got = R.pow_plain(sx, F(yy))
        assert same_bits(got, MC.pow_plain(sx, F(yy))), yy
        if yy == 0.0:
            assert (got == 1.0).all()                         # pow(x, 0) = 1, a NaN x included
        else:
            assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 1.0 and got[5] == np.inf and np.isnan(got[6]), (yy, got)
            assert got[3] >= 1.0 and (yy > 127.0 or np.isfinite(got[:5]).all())       # ((1 + 2^-23)^3e38 is inf, as libm's)
    assert same_bits(R.sin_plain(phi), MC.sin_plain(phi)) and same_bits(R.cos_plain(phi), MC.cos_plain(phi))
    assert np.isnan(R.sin_plain([np.nan])[0]) and np.isnan(R.cos_plain([np.nan])[0])
    assert R.sin_plain([0.0])[0] == 0.0 and R.cos_plain([0.0])[0] == 1.0


def test_mixed_dir_and_pdf_equal_the_restatement():
    rng = np.random.default_rng(6)
    cases = []
    for _ in range(400):
        cases.append((float(rng.choice([0.0, 1.0, 3.0, 10.0, 2.5, 40.0])), F(rng.random()), F(rng.random()), rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3)))
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    s = np.sqrt(1.0 - 0.81)
    edge = [(0.9, s, 0.0), (np.nextafter(F(0.9), F(1)), s, 0.0), (np.nextafter(F(0.9), F(0)), s, 0.0), (-0.9, 0.0, s), (np.nan, 0.0, 1.0), (0.0, 0.0, 0.0)]
    for n in axes + edge:
        for exp in (0.0, 1.0, 3.0):
            for a, b in ((0.25, 0.5), (0.0, 0.0), (1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24), (0.5, 0.0)):
                cases.append((exp, F(a), F(b), np.array(n)))
    for exp, a, b, n in cases:
        got, ref = R.mixed_dir(exp, a, b, n), MC.mixed_dir(exp, a, b, n)
        assert got.tobytes() == ref.tobytes(), (exp, a, b, n, got, ref)
    # xi_cos = 0: cos_theta = 1, the direction is unit(n) (+ 0 terms); exp = 0: cos_theta = 1 - xi_cos
    assert np.allclose(R.mixed_dir(3.0, 0.3, 0.0, (0, 0, 2)), (0, 0, 1), atol=1e-7)
    assert R.mixed_dir(0.0, 0.3, 0.25, (0, 0, 1))[2] == F(0.75)
    # material_pdf: random, then cos of 0, 1 and just above 1, a NaN normal, a back-face hit, another origin
    pdf_cases = []
    for _ in range(400):
        n, din, rd, p = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        pdf_cases.append((float(rng.choice([0.0, 1.0, 3.0, 10.0, 2.5])), p, n, din, p, rd))
    z, dn = np.array([0.0, 0.0, 1.0]), np.array([0.3, 0.1, -1.0])
    up = np.array([UP, 0.0, 0.0])                                                  # unit(rd) . unit(n) can round above 1: no clamp
    for exp in (0.0, 1.0, 3.0, 10.0):
        pdf_cases += [(exp, z, z, dn, z, np.array([1.0, 0.0, 0.0])), (exp, z, z, dn, z, z), (exp, z, up, -up, z, up), (exp, z, z * np.nan, dn, z, z),
                      (exp, z, z, -dn, z, -z), (exp, z, z, -dn, z, z), (exp, z, z, dn, z + 1e-6, z), (exp, z, z, dn, z + 5e-8, z)]
    for c in pdf_cases:
        got, ref = R.mixed_pdf(*c), MC.mixed_pdf(*c)
        assert got.tobytes() == ref.tobytes(), (c, got, ref)
    assert R.mixed_pdf(3.0, z, z, dn, z, z) == F(F(1.0 * 4.0) * MC.FRAC_1_2PI)           # cos = 1
    assert R.mixed_pdf(3.0, z, z, dn, z, (1.0, 0.0, 0.0)) == 0.0                        # cos = 0, exp > 0: pow(0, 3) = 0
    assert R.mixed_pdf(0.0, z, z, dn, z, (1.0, 0.0, 0.0)) == MC.FRAC_1_2PI              # cos = 0, exp = 0: pow(0, 0) = 1
    assert R.mixed_pdf(3.0, z, z, -dn, z, z) == 0.0                                     # back-face hit, ray along the normal: cos < 0
    assert R.mixed_pdf(3.0, z, z, -dn, z, -z) > 0.0                                     # ... and into the surface it is lit
    assert R.mixed_pdf(3.0, z, z, dn, z + 1e-6, z) == 0.0                               # another origin
    assert np.isnan(R.mixed_pdf(3.0, z, z * np.nan, dn, z, z))                          # a NaN cosine passes `cos < 0`


# ---- the error figures of DESIGN.md 4.7 -----------------------------------------------------------------------------------------------------
def stream_values():
    return (np.arange(2 ** 24, dtype=np.float64) / 2 ** 24).astype(F)


def pow_cosines():
    return np.concatenate([np.linspace(0, 1, 2 ** 22 + 1), np.random.default_rng(1).random(2 ** 20)]).astype(F)


def stream_phi():
    return ((stream_values() * F(2.0)).astype(F) * MC.PI).astype(F)


def test_pow_error_against_f64():
    base = (F(1.0) - stream_values()).astype(F)
    for ge, bound in POW_GEN.items():
        ge = F(ge)
        e = ulps(R.pow_plain(base, ge), np.power(base.astype(np.float64), float(ge)))
        print(f"pow_plain(1 - xi, {float(ge):.6f}): max {e.max():.4f} ulp at base {float(base[e.argmax()])!r} (recorded {bound})")
        assert e.max() <= bound
    cs = pow_cosines()
    for ex, bound in POW_EXP.items():
        e = ulps(R.pow_plain(cs, F(ex)), np.power(cs.astype(np.float64), ex))
        print(f"pow_plain(cos, {ex}): max {e.max():.4f} ulp at cos {float(cs[e.argmax()])!r} (recorded {bound})")
        assert e.max() <= bound


def test_sin_cos_error_against_f64():
    phi = stream_phi()
    for name, fn, ref, bound in (("sin", R.sin_plain, np.sin, SIN_ULP), ("cos", R.cos_plain, np.cos, COS_ULP)):
        e = ulps(fn(phi), ref(phi.astype(np.float64)))
        print(f"{name}_plain: max {e.max():.4f} ulp at phi {float(phi[e.argmax()])!r} (recorded {bound})")
        assert e.max() <= bound


# ---- the distribution ---------------------------------------------------------------------------------------------------------------------
def ks_uniform(x):
    x = np.sort(np.asarray(x, np.float64))
    n = x.size
    return max(np.max(np.arange(1, n + 1) / n - x), np.max(x - np.arange(n) / n))


@pytest.fixture(scope="module")
def draws():
    rng = LC.Rng(11, 5)
    n = 2 ** 20
    xi = np.array([rng.next() for _ in range(2 * n)], F)
    return xi[0::2].copy(), xi[1::2].copy()                  # (xi_phi, xi_cos) of consecutive on_hit calls


@pytest.mark.parametrize("exp", [1.0, 3.0, 10.0])
def test_distribution_of_mixed_dir(draws, exp):
    """n = (0, 0, 1): the basis is u = (-1, 0, 0), v = (0, 1, 0), w = n, so the direction is (-x, y, z) of the local vector exactly -- formed
    here from the array functions and pinned to rtw_mixed_dir on a sample.  From the pdf cos^exp (exp + 1) / 2 pi: z^(exp + 1) is uniform,
    E z = (exp + 1) / (exp + 2), E z^2 = (exp + 1) / (exp + 3), the azimuth is uniform."""
    xi_phi, xi_cos = draws
    n = xi_phi.size
    gen_exp = F(F(1.0) / F(F(exp) + F(1.0)))
    z = R.pow_plain((F(1.0) - xi_cos).astype(F), gen_exp)
    st = np.sqrt((F(1.0) - (z * z).astype(F)).astype(F)).astype(F)
    phi = ((xi_phi * F(2.0)).astype(F) * MC.PI).astype(F)
    d = np.stack([-(R.cos_plain(phi) * st).astype(F), (R.sin_plain(phi) * st).astype(F), z], axis=1)
    for k in range(0, n, n // 512):
        assert np.array_equal(R.mixed_dir(exp, xi_phi[k], xi_cos[k], (0.0, 0.0, 1.0)), d[k]), k
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    mean = (exp + 1.0) / (exp + 2.0)
    var = (exp + 1.0) / (exp + 3.0) - mean * mean
    zm = z.astype(np.float64).mean()
    print(f"exp {exp}: mean z {zm:.6f} (expected {mean:.6f}, standard error {np.sqrt(var / n):.2e})")
    assert abs(zm - mean) <= 5.0 * np.sqrt(var / n)
    crit = np.sqrt(-np.log(1e-6 / 2.0) / (2.0 * n))          # Kolmogorov-Smirnov, level 1e-6
    ks_z = ks_uniform(z.astype(np.float64) ** (exp + 1.0))
    az = np.mod(np.arctan2(d[:, 1].astype(np.float64), -d[:, 0].astype(np.float64)), 2 * np.pi) / (2 * np.pi)
    ks_a = ks_uniform(az)
    print(f"exp {exp}: KS z^(exp+1) {ks_z:.5f}, azimuth {ks_a:.5f} (critical {crit:.5f})")
    assert ks_z < crit and ks_a < crit


@pytest.mark.parametrize("exp", [0.0, 1.0, 3.0, 10.0])
def test_material_pdf_integrates_to_one(exp):
    x, w = np.polynomial.legendre.leggauss(96)
    th = 0.25 * np.pi * (x + 1.0)
    z = np.zeros(3)
    n, din = (0.0, 0.0, 1.0), (0.2, 0.1, -1.0)
    pdf = np.array([float(R.mixed_pdf(exp, z, n, din, z, (np.sin(t), 0.0, np.cos(t)))) for t in th])
    total = float(np.sum(w * pdf * 2.0 * np.pi * np.sin(th)) * 0.25 * np.pi)
    print(f"exp {exp}: integral of material_pdf over the hemisphere {total:.7f}")
    assert abs(total - 1.0) <= 1e-4
    assert float(R.mixed_pdf(exp, z, n, din, z, (0.6, 0.0, -0.8))) == 0.0            # nothing below the surface


# ---- validation ---------------------------------------------------------------------------------------------------------------------------
def test_validation_returns():
    ms, g = MC.golden()
    for integ in range(7):
        p = ms.params(8, 6, integ, 3)
        assert R.mixed_validate(ms.scene, p) == R.RTW_OK                              # without the flag nothing is checked
        p.flags = R.FLAG_MIXED_MATERIAL | R.FLAG_GLOBAL_NODES
        ok = integ in (R.INTEGRATOR_RUST2, R.INTEGRATOR_LIGHT_CAST, R.INTEGRATOR_LIGHT_BIASED)
        assert R.mixed_validate(ms.scene, p) == (R.RTW_OK if ok else E_UNSUPPORTED), integ
        plain, _ = LC.golden()                                                        # no object with opacity < 0: the integrator rule alone
        assert R.mixed_validate(plain.scene, p) == (R.RTW_OK if ok else E_UNSUPPORTED), integ
    p = ms.params(8, 6, R.INTEGRATOR_LIGHT_BIASED, 3)
    p.flags = R.FLAG_MIXED_MATERIAL
    for bad in (-1.0, -1e-30, float("inf"), float("nan")):
        for where in ("quad", "sphere", "box"):
            q, sp, boxes = [dict(x) for x in g["quads"]], [dict(x) for x in g["spheres"]], []
            if where == "quad":
                q[2]["exp"] = bad
            elif where == "sphere":
                sp.append({"origin": [0, 0, 3], "radius": 0.2, "material": "mixed", "exp": bad, "color": [1, 1, 1], "emitted": [0, 0, 0]})
            else:
                boxes = [{"a": [0, 0, 0], "b": [1, 1, 1], "material": "mixed", "exp": bad, "color": [1, 1, 1]}]
            s = MC.MixedScene(sp, q, ms.lights, g["background"], boxes=boxes)
            assert R.mixed_validate(s.scene, p) == E_INVALID, (bad, where)
            p0 = R.RtwParams.from_buffer_copy(p)
            p0.flags = 0
            assert R.mixed_validate(s.scene, p0) == R.RTW_OK
    assert R.mixed_validate(ms.scene, p, n_triangles=1) == E_UNSUPPORTED
    assert R.mixed_validate(ms.scene, p, texture_noise=True) == E_UNSUPPORTED
    smoke = R.Instance.new_box((0, 0, 0), (1, 1, 1), (1, 1, 1), (0.0, 0.0, 1.0))
    smoke.const_density(0.5)
    s = R.Scene([ms.scene._spheres[0]], quads=[ms.scene._quads[k] for k in range(len(ms.quads))], instances=[smoke])
    assert R.mixed_validate(s, p) == E_UNSUPPORTED
    plain, _ = LC.golden()
    assert R.mixed_validate(plain.scene, p, n_triangles=1, texture_noise=True) == R.RTW_OK     # no mixed object: as without the flag


# ---- the reference's recursion against the device's front-to-back form ------------------------------------------------------------------------
def test_reference_form_against_device_form_on_the_golden_scene():
    """DESIGN.md 4.6's rounding bound between the recursion and the front-to-back form holds unchanged with the mixed pdf (every term is
    still >= 0); observed on the golden scene at 40 x 30, depth 9: at most 0.20 of the bound."""
    ms, g = MC.golden()
    w, h = 40, 30
    cam = LC.camera_no_rand(g, w, h)
    for integ, depth in ((R.INTEGRATOR_LIGHT_BIASED, g["depth_light_biased"]), (R.INTEGRATOR_RUST2, g["depth_light_biased"]),
                         (R.INTEGRATOR_LIGHT_CAST, g["depth_light_cast"])):
        p = ms.params(w, h, integ, depth, seed=1)
        p.flags = R.FLAG_MIXED_MATERIAL
        img, seg, info = MC.render(ms, cam, p, check=True)
        print(f"integrator {integ}: {info['mixed_hits']} mixed hits, {seg} segments, |front to back - recursion| at most {info['max_rel']:.3f} of the bound")
        assert np.isfinite(img).all() and info["mixed_hits"] > 0 and info["max_rel"] <= 1.0
