"""The hot path's arithmetic sequences, evaluated on the GPU itself (rtw_ctx_device_math / rtw_ctx_device_sweep, csrc/rtw_probe.hip).

csrc/rtw_device.h replaces hipcc's IEEE sqrt and divide by shorter sequences wherever a whole wave's operands are "plain", and DESIGN.md 2
rests on those giving the same bits.  Every other test meets them through an image or a ray query, at the operands a scene happens to
produce; here sqrt_plain runs on EVERY argument of its range and div_plain on 2^32 pairs per kind, each result judged exactly in integers
(tests/test_device_math_cpu.py tests that judge), the callers are run with whole waves inside and outside the plain range, and the device
compiles of atan2_plain / acos_plain / ln_f32 / pow_plain / sincos_plain / exp_plain are held against the host compiles and the oracle's copies.

Every comparison is on the bits; a NaN is compared as "is NaN".  There is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests import oracle_binding as O
from tests.test_device_math_cpu import SQRT_HI, SQRT_LO, bits, f32, pow2
from tests.test_guided_cpu import EXP_SPECIAL_X, exp_arguments, exp_threshold_arguments
from tests.test_mixed_cpu import POW_GEN, POW_EXP, POW_SPECIAL_X, POW_SPECIAL_Y, elementary_arguments, pow_cosines, stream_phi, stream_values
from tests.test_oracle_golden import small_view
from tests.test_round3_cpu import UV_SPECIAL, uv_normals

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
E_INVALID = -1
SPOILED_LANE = 17
CHUNK = 1 << 28                                        # arguments per sweep call: well under a second of kernel time each


def up(v):
    return np.nextafter(F(v), F(np.inf))


def dn(v):
    return np.nextafter(F(v), F(-np.inf))


def mismatches(got, ref):
    """indices where got and ref differ: bits, except that any NaN equals any NaN"""
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    assert got.shape == ref.shape
    both_nan = np.isnan(got) & np.isnan(ref)
    return np.flatnonzero(((bits(got) != bits(ref)) & ~both_nan).reshape(len(got), -1).any(axis=1))


def assert_same(got, ref, args, what):
    bad = mismatches(got, ref)
    assert bad.size == 0, (f"{what}: {bad.size} of {len(got)} differ; first at {bad[:4]}: arguments {[np.asarray(a)[bad[:4]] for a in args]}, "
                           f"device {np.asarray(got)[bad[:4]]} ({bits(np.asarray(got)[bad[:4]])}), reference {np.asarray(ref)[bad[:4]]} "
                           f"({bits(np.asarray(ref)[bad[:4]])})")


def random_f32(rng, n, e_lo, e_hi, signed=True):
    """random mantissas, exponents uniform over [e_lo, e_hi): |v| in [2^e_lo, 2^e_hi)"""
    m = rng.integers(0, 1 << 23, n, dtype=np.uint64)
    e = rng.integers(e_lo + 127, e_hi + 127, n, dtype=np.uint64)
    s = rng.integers(0, 2, n, dtype=np.uint64) if signed else np.zeros(n, np.uint64)
    return f32(((s << 31) | (e << 23) | m).astype(U))


def sweep(gpu, which, first, count, seed=0):
    """`count` arguments from index `first`, in calls of CHUNK: (wrong, kernel ms, records of the failures)"""
    wrong, ms, records, done = 0, 0.0, [], 0
    while done < count:
        n = min(CHUNK, count - done)
        res = gpu.device_sweep(which, first + done, n, seed)
        assert res.tested == n and res.n_records == min(res.wrong, R.SWEEP_RECORDS)
        wrong += res.wrong; ms += res.kernel_ms; records += res.failures(); done += n
    return wrong, ms, records


# ---- sqrt ----------------------------------------------------------------------------------------------------------------------------------
def test_sqrt_plain_is_correctly_rounded_on_every_argument(gpu):
    """Every f32 in [2^-96, 2^127): exactly the arguments sqrt_ieee sends down the plain sequence."""
    count = SQRT_HI - SQRT_LO
    assert count == 1_870_659_584
    wrong, ms, records = sweep(gpu, R.SWEEP_SQRT, SQRT_LO, count)
    print(f"sweep sqrt: {count} arguments, {wrong} wrong, {ms:.1f} ms of kernel time")
    assert wrong == 0, records


def test_sweeps_report_wrong_results(gpu):
    """The sweep's own plumbing: the judge refuses an argument that is not a positive normal number, so +0 and the first subnormals all count
    as wrong -- the count, the cap on the records and what a record holds."""
    res = gpu.device_sweep(R.SWEEP_SQRT, 0, 4096)                                    # +0 and the first subnormals
    assert res.tested == 4096 and res.wrong == 4096 and res.n_records == R.SWEEP_RECORDS
    for r in res.records[:res.n_records]:
        assert r.a < 4096 and r.b == 0
        assert r.got == bits(gpu.device_math(R.MATH_SQRT_PLAIN, f32(U(r.a))))[0]
    res = gpu.device_sweep(R.SWEEP_SQRT, SQRT_LO, 1)
    assert (res.tested, res.wrong, res.n_records) == (1, 0, 0) and res.kernel_ms > 0.0


def test_sqrt_ieee_with_mixed_waves(gpu):
    rng = np.random.default_rng(31)
    ends = f32(np.concatenate([np.arange(SQRT_LO - 3, SQRT_LO + 4), np.arange(SQRT_HI - 3, SQRT_HI + 4)]).astype(U))
    special = np.array([0.0, -0.0, 1e-45, 1e-40, 1.1754942e-38, np.inf, -np.inf, np.nan, -1.0, -1e-30, -3e38, 2.0 ** -126, 3.4028235e38], F)
    plain = f32(rng.integers(SQRT_LO, SQRT_HI, 1 << 16, dtype=np.uint64).astype(U))
    # whole waves in the plain range, then waves that each hold one or more of the others, then all of them shuffled
    tail = np.concatenate([ends, special, plain[:4096 - len(ends) - len(special)]])
    x = np.concatenate([plain, np.concatenate([ends, special, plain])[rng.permutation(len(plain) + len(ends) + len(special))], tail, special])
    with np.errstate(invalid="ignore"):
        ref = np.sqrt(x)
    assert_same(gpu.device_math(R.MATH_SQRT_IEEE, x), ref, [x], "sqrt_ieee")
    # ... and the plain sequence itself at the ends of its range
    inside = f32(np.concatenate([np.arange(SQRT_LO, SQRT_LO + 64), np.arange(SQRT_HI - 64, SQRT_HI)]).astype(U))
    assert_same(gpu.device_math(R.MATH_SQRT_PLAIN, inside), np.sqrt(inside), [inside], "sqrt_plain")


# ---- the quotient ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 0x9E3779B9])
@pytest.mark.parametrize("which,name", [(R.SWEEP_DIV_RANDOM, "div_random"), (R.SWEEP_DIV_MIDPOINT, "div_midpoint")])
def test_div_plain_is_correctly_rounded(gpu, which, name, seed):
    count = 1 << 30
    first = (seed & 0xFF) << 30                                                       # (indices beyond 2^32 as well)
    wrong, ms, records = sweep(gpu, which, first, count, seed)
    print(f"sweep {name}, seed {seed:#x}: {count} pairs, {wrong} wrong, {ms:.1f} ms of kernel time")
    assert wrong == 0, records


def test_sweep_operands_are_the_host_entry_points(gpu):
    """A pair the host forms (rtw_sweep_operands, pinned by the CPU tests) gives on the device the quotient the sweep judged: the midpoint
    pairs element-wise against numpy."""
    for which in (R.SWEEP_DIV_RANDOM, R.SWEEP_DIV_MIDPOINT):
        n, d = R.sweep_operands(which, 12345, 1 << 16, 5)
        assert_same(gpu.device_math(R.MATH_DIV, n, d), n / d, [n, d], "div_plain on sweep operands")


def test_div_plain_at_the_ends_of_its_range(gpu):
    """Every combination of |d| in {2^-40, 2^-40 + ulp, 1, 3, 2^40 - ulp, 2^40} with |n| in {0, 2^-60, 2^-60 + ulp, 1, 2^40}, all signs.
    A zero numerator keeps IEEE's sign: -0 / d is -0 for a positive d (the residuals of the refinement are +0 there; div_plain takes the
    sign of n * r.  The hot path's callers, whose numerators cannot be such a zero, call the refinement alone, div_plain_nz: the sweeps
    above judge that one and require div_plain to agree with it)."""
    ds = np.array([pow2(-40), up(pow2(-40)), 1.0, 3.0, dn(pow2(40)), pow2(40)], F)
    ns = np.array([0.0, pow2(-60), up(pow2(-60)), 1.0, pow2(40)], F)
    n, d = [g.ravel() for g in np.meshgrid(ns, ds)]
    n = np.concatenate([n, -n, n, -n]); d = np.concatenate([d, d, -d, -d])
    assert len(n) == 120
    q = gpu.device_math(R.MATH_DIV, n, d)
    assert_same(q, n / d, [n, d], "div_plain")
    assert R.rounding_check(R.SWEEP_DIV_RANDOM, n, d, q).all()


def test_div_plain_on_the_quotients_of_sphere_root(gpu):
    """sphere_root's comment: a in [2^-20, 2^20], a numerator that is 0 or at least 2^-54 in magnitude (and below 2^65)."""
    rng = np.random.default_rng(32)
    n = 1 << 20
    a = random_f32(rng, n, -20, 20, signed=False)
    a[:4096:4] = pow2(-20); a[1:4096:4] = pow2(20); a[2:4096:4] = up(pow2(-20)); a[3:4096:4] = dn(pow2(20))
    num = random_f32(rng, n, -54, 65)
    num[:8192:8] = 0.0; num[4:8192:8] = -0.0; num[1:8192:8] = pow2(-54); num[2:8192:8] = -pow2(-54); num[3:8192:8] = dn(pow2(65))
    assert_same(gpu.device_math(R.MATH_DIV, num, a), num / a, [num, a], "div_plain")


# ---- unit, unit_of_ball_point, sphere_root: the plain path, the generic path, numpy -------------------------------------------------------------
def both_arrangements(gpu, fn, cols, spoilers, ref_fn, what):
    """cols: [n, k] with every wave inside the plain range (n a multiple of 64).  Arrangement 1 runs them as they are: the plain path.
    Arrangement 2 replaces lane 17 of every wave by a spoiler (cycling through `spoilers`): the generic path.  Every result is numpy's."""
    n = len(cols)
    assert n % 64 == 0 and n >= 64 * len(spoilers)
    ref = ref_fn(cols)
    one = gpu.device_math(fn, cols)
    assert_same(one, ref, [cols], f"{what}, whole waves in the plain range")
    spoiled = cols.copy()
    lanes = np.arange(SPOILED_LANE, n, 64)
    spoiled[lanes] = np.asarray(spoilers, F)[np.arange(len(lanes)) % len(spoilers)]
    ref2 = ref_fn(spoiled)
    two = gpu.device_math(fn, spoiled)
    assert_same(two, ref2, [spoiled], f"{what}, a spoiler in lane {SPOILED_LANE} of every wave")
    keep = np.ones(n, bool); keep[lanes] = False
    assert_same(two[keep], one[keep], [cols[keep]], f"{what}: the plain path against the generic path")
    return one


def ref_unit(a):
    with np.errstate(all="ignore"):
        x, y, z = a[:, 0], a[:, 1], a[:, 2]
        s = np.sqrt(x * x + y * y + z * z)
        return np.stack([x / s, y / s, z / s], axis=1)


def test_unit_plain_and_generic(gpu):
    rng = np.random.default_rng(33)
    n = 1 << 20
    a = np.stack([random_f32(rng, n, -40, 40) for _ in range(3)], axis=1)
    ends = np.array([pow2(-40), pow2(40), -pow2(-40), -pow2(40), 1.0, dn(pow2(40)), up(pow2(-40))], F)
    grid = np.stack([g.ravel() for g in np.meshgrid(ends, ends, ends)], axis=1)       # 343 vectors with components at the ends
    a[1000:1000 + len(grid)] = grid
    spoilers = [[0.0, 1.0, 2.0], [1.0, -0.0, 2.0], [0.5, 0.25, 0.0], [1e-40, 1.0, 1.0], [1.0, 1.0, -1e-45], [pow2(41), 1.0, 1.0],
                [1.0, up(pow2(40)), 1.0], [dn(pow2(-40)), 1.0, 1.0], [np.inf, 1.0, 1.0], [1.0, 1.0, -np.inf], [np.nan, 1.0, 1.0], [0.0, 0.0, 0.0],
                [3e38, 3e38, 3e38], [1e-30, 1e-30, 1e-30]]
    both_arrangements(gpu, R.MATH_UNIT, a, spoilers, ref_unit, "unit")


def ref_unit_ball(c):
    with np.errstate(all="ignore"):
        s = np.sqrt(c[:, 3])
        return np.stack([c[:, 0] / s, c[:, 1] / s, c[:, 2] / s], axis=1)


def test_unit_of_ball_point_plain_and_generic(gpu):
    rng = np.random.default_rng(34)
    n = 1 << 20
    k = rng.integers(-(1 << 23), 1 << 23, (2 * n, 3)).astype(np.float64)
    small = rng.integers(-4, 5, (1 << 14, 3)).astype(np.float64)                     # ... down to |p|^2 = 3 * 2^-46
    mixed = np.where(rng.random((1 << 14, 3)) < 0.5, rng.integers(-4, 5, (1 << 14, 3)), rng.integers(-(1 << 23), 1 << 23, (1 << 14, 3))).astype(np.float64)
    p = (np.concatenate([small, mixed, k]) * 2.0 ** -23).astype(F)
    l2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]).astype(F)         # the sampler's expression
    ok = (p != 0).all(axis=1) & (l2 <= 1.0)                                            # accepted points without a zero component: the plain path
    p, l2 = p[ok][:n], l2[ok][:n]
    assert len(p) == n and l2.min() == F(3 * 2.0 ** -46) and l2.max() > 0.999
    cols = np.concatenate([p, l2[:, None]], axis=1)
    t = F(2.0 ** -23)
    spoilers = [[t, 0.0, 0.0, t * t], [0.0, -t, 0.0, t * t], [0.0, 0.0, t, t * t], [0.5, -0.0, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0], [0.25, 0.0, -0.5, 0.3125],
                [np.nan, 0.5, 0.5, np.nan], [-1.0, 0.0, 0.0, 1.0]]
    both_arrangements(gpu, R.MATH_UNIT_BALL, cols, spoilers, ref_unit_ball, "unit_of_ball_point")


def ref_sphere_root(c):
    b, disc, a, mint = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    with np.errstate(all="ignore"):
        sq = np.sqrt(disc)
        x = (-b - sq) / a
        x = np.where(x < mint, (-b + sq) / a, x)
        return np.where(disc < 0.0, F(np.nan), x).astype(F)                              # the kernels do not take the root of a negative disc


def test_sphere_root_plain_and_generic(gpu):
    rng = np.random.default_rng(35)
    n = 1 << 19
    b = random_f32(rng, n, -30, 47)
    disc = random_f32(rng, n, -60, 96, signed=False)
    a = random_f32(rng, n, -20, 20, signed=False)
    mint = np.array([0.001, -np.inf, np.inf, 0.0], F)[rng.integers(0, 4, n)]           # the reference's, "never the + root", "always", zero
    # the ends of disc's range and one ulp inside (one ulp outside is a spoiler below), the ends of a's
    disc[0:4096:8] = pow2(-60); disc[1:4096:8] = pow2(96); disc[2:4096:8] = up(pow2(-60)); disc[3:4096:8] = dn(pow2(96))
    a[4096:8192:4] = pow2(-20); a[4097:8192:4] = pow2(20); a[4098:8192:4] = up(pow2(-20)); a[4099:8192:4] = dn(pow2(20))
    # b and sqrt(disc) that cancel exactly (disc an exact square, b = -+ its root) and nearly (b an ulp or two away)
    m = 1 << 16
    root = random_f32(rng, m, -29, 40, signed=False)
    root = f32(bits(root) & U(0xFFFFF000))                                               # 12-bit mantissas: the square is exact
    sl = slice(8192, 8192 + m)
    disc[sl] = root * root
    assert np.array_equal(np.sqrt(disc[sl]), root)
    sign = np.where(rng.random(m) < 0.5, F(1.0), F(-1.0)).astype(F)
    near = rng.integers(-2, 3, m)
    b[sl] = sign * f32((bits(root).astype(np.int64) + near).astype(U))
    assert (near == 0).sum() > 10000
    cols = np.stack([b, disc, a, mint], axis=1)
    spoilers = [[1.0, -0.0, 1.0, 0.001], [-1.0, -0.0, 2.0, 0.001], [1.0, dn(pow2(-60)), 1.0, 0.001], [0.5, pow2(-61), 1.0, -1.0],
                [1.0, 1e-40, 1.0, 0.001], [1.0, 0.0, 1.0, 0.001], [-3.0, up(pow2(96)), 1.0, 0.001], [-3.0, pow2(97), 4.0, 0.001],
                [1.0, 4.0, pow2(21), 0.001], [-1.0, 4.0, up(pow2(20)), 0.001], [1.0, 4.0, dn(pow2(-20)), 0.001], [-5.0, 4.0, pow2(-21), 0.001],
                [1.0, np.inf, 1.0, 0.001], [1.0, np.nan, 1.0, 0.001], [np.nan, 4.0, 1.0, 0.001], [1.0, 4.0, 0.0, 0.001], [1.0, 4.0, np.inf, 0.001],
                [1.0, -4.0, 1.0, 0.001], [1.0, 4.0, 1e-40, 0.001], [-1.0, 4.0, np.nan, 0.001]]
    got = both_arrangements(gpu, R.MATH_SPHERE_ROOT, cols, spoilers, ref_sphere_root, "sphere_root")
    first = (-b - np.sqrt(disc)) / a
    assert (got[~(first < mint)] == first[~(first < mint)]).all() and (first < mint).sum() > n // 4 and (~(first < mint)).sum() > n // 4
    assert ((got[sl] == 0) & (near == 0)).sum() > 1000                                   # exact cancellation: a zero root was kept where mint allows


# ---- atan2_plain, acos_plain, sphere_uv against the oracle's copy ---------------------------------------------------------------------------
def oracle_uv(normals):
    """[n, 4]: atan2(-z, x), acos(-y), u, v through the oracle's restatement of the device's sequences (`/` and sqrtf)"""
    normals = np.ascontiguousarray(normals, F)
    out = np.empty((len(normals), 4), F)
    fp = C.POINTER(C.c_float)
    O.lib().rtw_oracle_sphere_uv(normals.ctypes.data_as(fp), len(normals), 1, out.ctypes.data_as(fp))
    return out


def device_uv(gpu, normals):
    at = gpu.device_math(R.MATH_ATAN2, -normals[:, 2], normals[:, 0])
    ac = gpu.device_math(R.MATH_ACOS, -normals[:, 1])
    return at, ac, gpu.device_math(R.MATH_SPHERE_UV, normals)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_acos_plain_on_every_argument_above_a_half(gpu, sign):
    """|x| in [0.5, 1], every f32: sqrt_plain then meets every value its caller can hand it, s = (1 - |x|) / 2 = 0 included."""
    x = f32(np.arange(0x3F000000, 0x3F800001, dtype=U)) * F(sign)
    assert len(x) == (1 << 23) + 1 and abs(x[0]) == 0.5 and abs(x[-1]) == 1.0
    normals = np.zeros((len(x), 3), F)
    normals[:, 1] = -x
    ref = oracle_uv(normals)
    assert_same(gpu.device_math(R.MATH_ACOS, x), ref[:, 1], [x], "acos_plain")
    assert_same(gpu.device_math(R.MATH_SPHERE_UV, normals), ref[:, 2:], [x], "sphere_uv")


def test_acos_plain_elsewhere(gpu):
    rng = np.random.default_rng(36)
    x = np.concatenate([(rng.random(1 << 20) - 0.5).astype(F), random_f32(rng, 1 << 16, -126, -1),
                        np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, up(1.0), -up(1.0), 2.0, -2.0, np.inf, -np.inf, np.nan, 0.5, -0.5, up(0.5), -up(0.5),
                                  dn(0.5), 1.0, -1.0, dn(1.0)], F)])
    normals = np.zeros((len(x), 3), F)
    normals[:, 1] = -x
    ref = oracle_uv(normals)
    assert_same(gpu.device_math(R.MATH_ACOS, x), ref[:, 1], [x], "acos_plain")
    assert_same(gpu.device_math(R.MATH_SPHERE_UV, normals), ref[:, 2:], [x], "sphere_uv")


def quotient_class(normals):
    """atan2_plain's quotient min / max for (y, x) = (-z, x), as float32 with one rounding: (strict, t).  strict: the quotient is zero because
    its numerator is, or a normal number -- the class for which div_plain is correctly rounded by its derivation."""
    ax, ay = np.abs(normals[:, 0]), np.abs(normals[:, 2])
    big, small = np.maximum(ax, ay), np.minimum(ax, ay)
    k = np.where(big < pow2(-60), pow2(80), F(1.0)).astype(F)
    mx, mn = big * k, small * k
    with np.errstate(all="ignore"):
        t = np.where(mx == 0, F(0.0), mn / mx).astype(F)
    return (mn == 0) | (t >= F(2.0 ** -126)) | np.isnan(t), t


def tiny_component_normals():
    """one of x, z at m 2^-k for every k from 1 to 149 (a few mantissas m), the other at 1, 0.75, 2^-30 (and 2^-100: the rescaled branch)"""
    rows = []
    for k in range(1, 150):
        for m in (1.0, 1.25, 1.3333334, 1.9999999):
            tiny = np.ldexp(F(m), -k)
            for other in (1.0, 0.75, 2.0 ** -30, 2.0 ** -100):
                for sx in (1.0, -1.0):
                    for sz in (1.0, -1.0):
                        rows.append([sx * tiny, 0.5, sz * other])
                        rows.append([sx * other, -0.25, sz * tiny])
    return np.array(rows, F)


@pytest.fixture(scope="module")
def uv_case(gpu):
    """the normals of the two tests below, the oracle's copy on them and the device's results: formed once"""
    normals = np.concatenate([uv_normals(), UV_SPECIAL, tiny_component_normals()])
    return normals, oracle_uv(normals), device_uv(gpu, normals)


def test_sphere_uv_and_acos_plain_against_the_oracle_copy(uv_case):
    """2 M unit normals, the axes, the special values, and normals with a component of every size down to 2^-149: u, v and acos are the
    oracle copy's bits for every one of them."""
    normals, ref, (at, ac, uv) = uv_case
    assert_same(uv, ref[:, 2:], [normals], "sphere_uv (u, v)")
    assert_same(ac, ref[:, 1], [normals], "acos_plain")


def test_atan2_plain_against_the_oracle_copy(uv_case):
    """atan2_plain's value, bit-equal wherever its quotient min / max is zero or a normal number; for subnormal quotients the differences
    are printed, not asserted ((u, v) above covers those inputs).
    atan2_plain scales a numerator below 2^-60 by 2^64 for the division (div_plain's residual n - d q, a multiple of ulp(d) ulp(q), is
    otherwise no longer a float for quotients near 2^-126) and the quotient back, which is exact while the quotient is normal; a subnormal
    quotient is rounded a second time there."""
    normals, ref, (at, ac, uv) = uv_case
    strict, t = quotient_class(normals)
    sub = ~strict
    assert strict.sum() > 2_000_000 and sub.sum() > 500                              # quotients through the subnormals too
    assert ((t[strict] > 0) & (t[strict] < F(2.0 ** -100))).sum() > 100              # ... and tiny normal ones, numerators far below 2^-60
    differs = (bits(at) != bits(ref[:, 0])) & ~(np.isnan(at) & np.isnan(ref[:, 0]))
    d = np.abs(at.astype(np.float64) - ref[:, 0].astype(np.float64))
    for name, cls in (("zero or normal", strict), ("subnormal or underflowed", sub)):
        w = differs & cls
        print(f"atan2_plain, quotient {name}: {int(cls.sum())} arguments, {int(w.sum())} differ from the oracle's copy" +
              (f"; largest quotient among them {t[w].max()!r}, largest difference {d[w].max() / 2.0 ** -149:.1f} x 2^-149" if w.any() else ""))
    big = strict & ~((t > 0) & (t < F(2.0 ** -100)))
    assert_same(at[big], ref[big, 0], [normals[big]], "atan2_plain, quotient zero or at least 2^-100")
    assert_same(at[strict], ref[strict, 0], [normals[strict]], "atan2_plain, quotient zero or normal")


# ---- ln_f32 ----------------------------------------------------------------------------------------------------------------------------------
def test_ln_f32_on_every_stream_value(gpu):
    x = stream_values()[1:]
    assert len(x) == (1 << 24) - 1 and x[0] == F(2.0 ** -24)
    ref = np.empty_like(x)
    O.lib().rtw_oracle_ln_bulk(x.ctypes.data_as(C.POINTER(C.c_float)), ref.ctypes.data_as(C.POINTER(C.c_float)), x.size)
    assert_same(gpu.device_math(R.MATH_LN, x), ref, [x], "ln_f32")
    zero = gpu.device_math(R.MATH_LN, np.array([0.0, 1.0], F))
    assert zero[0] == -np.inf and zero[1] == 0.0


# ---- pow_plain, sincos_plain, exp_plain: the device compile against the host compile ---------------------------------------------------------
def test_pow_plain_device_equals_host(gpu):
    x, y, _ = elementary_arguments()
    assert_same(gpu.device_math(R.MATH_POW, x, y), R.pow_plain(x, y), [x, y], "pow_plain")
    sx, sy = [g.ravel().astype(F) for g in np.meshgrid(POW_SPECIAL_X, np.array(POW_SPECIAL_Y, F))]
    assert_same(gpu.device_math(R.MATH_POW, sx, sy), R.pow_plain(sx, sy), [sx, sy], "pow_plain, special cases")


@pytest.mark.parametrize("gen_exp", list(POW_GEN))
def test_pow_plain_device_equals_host_on_the_stream(gpu, gen_exp):
    base = (F(1.0) - stream_values()).astype(F)
    y = np.full_like(base, F(gen_exp))
    assert_same(gpu.device_math(R.MATH_POW, base, y), R.pow_plain(base, y), [base, y], "pow_plain(1 - xi, gen_exp)")


def test_pow_plain_device_equals_host_on_cosines(gpu):
    cs = pow_cosines()
    for ex in POW_EXP:
        y = np.full_like(cs, F(ex))
        assert_same(gpu.device_math(R.MATH_POW, cs, y), R.pow_plain(cs, y), [cs, y], f"pow_plain(cos, {ex})")


def test_sincos_plain_device_equals_host(gpu):
    for phi in (elementary_arguments()[2], stream_phi()):
        sc = gpu.device_math(R.MATH_SINCOS, phi)
        assert_same(sc[:, 0], R.sin_plain(phi), [phi], "sin_plain")
        assert_same(sc[:, 1], R.cos_plain(phi), [phi], "cos_plain")


def test_exp_plain_device_equals_host(gpu):
    every_64th = f32(np.arange(0x80000000, 0xC2D00000 + 1, 64, dtype=np.uint64).astype(U))            # -0 down to -104
    assert every_64th[0] == 0 and np.signbit(every_64th[0]) and every_64th[-1] == F(-104.0)
    special = np.concatenate([EXP_SPECIAL_X, np.array([1e-45, 1.0, 88.0, np.inf, 1e-30, -1e-45, -1e-40, up(-104.0), dn(-104.0), -200.0], F)])
    for x in (every_64th, exp_arguments(), exp_threshold_arguments(), special):
        assert_same(gpu.device_math(R.MATH_EXP, x), R.exp_plain(x), [x], "exp_plain")


# ---- the call itself -----------------------------------------------------------------------------------------------------------------------------
def test_a_probe_call_between_two_renders_changes_nothing():
    scene, cam, p = small_view(R.SCENE_C5, 96, 54, 4)
    p.accel = R.ACCEL_BVH
    x = f32(np.arange(SQRT_LO, SQRT_LO + 100000, dtype=U))
    with R.Renderer(0) as r:
        r.set_scene(scene)
        a, st_a = r.render(cam, p)
        s = r.device_math(R.MATH_SQRT_IEEE, x)
        res = r.device_sweep(R.SWEEP_DIV_MIDPOINT, 0, 1 << 20, 3)
        uv = r.device_math(R.MATH_SPHERE_UV, uv_normals()[:1000])
        b, st_b = r.render(cam, p)
        assert np.array_equal(a.view(U), b.view(U)) and st_a.segments == st_b.segments
        assert np.array_equal(s, np.sqrt(x)) and res.wrong == 0 and uv.shape == (1000, 2)


def test_statuses_with_a_device(gpu):
    L = R.lib()
    x = np.ones(8, F); out = np.empty(24, F)
    fp = C.POINTER(C.c_float)
    xp, op = x.ctypes.data_as(fp), out.ctypes.data_as(fp)
    h = gpu._h
    assert L.rtw_ctx_device_math(h, R.MATH_SQRT_PLAIN, xp, 1, 8, op, 1) == 0
    assert L.rtw_ctx_device_math(None, R.MATH_SQRT_PLAIN, xp, 1, 8, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(h, R.MATH_SQRT_PLAIN, None, 1, 8, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(h, R.MATH_SQRT_PLAIN, xp, 1, 8, None, 1) == E_INVALID
    assert L.rtw_ctx_device_math(h, R.MATH_SQRT_PLAIN, xp, 1, 0, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(h, 13, xp, 1, 8, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(h, 0xFFFFFFFF, xp, 1, 8, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(h, R.MATH_UNIT, xp, 1, 2, op, 3) == E_INVALID          # unit reads three columns
    assert L.rtw_ctx_device_math(h, R.MATH_UNIT, xp, 3, 2, op, 1) == E_INVALID          # ... and writes three
    assert L.rtw_ctx_device_math(h, R.MATH_UNIT, xp, 3, 2, op, 3) == 0
    res = R.RtwSweepResult()
    assert L.rtw_ctx_device_sweep(h, R.SWEEP_DIV_RANDOM, 0, 256, 0, C.byref(res)) == 0 and res.tested == 256 and res.wrong == 0
    assert L.rtw_ctx_device_sweep(None, R.SWEEP_DIV_RANDOM, 0, 256, 0, C.byref(res)) == E_INVALID
    assert L.rtw_ctx_device_sweep(h, R.SWEEP_DIV_RANDOM, 0, 256, 0, None) == E_INVALID
    assert L.rtw_ctx_device_sweep(h, R.SWEEP_DIV_RANDOM, 0, 0, 0, C.byref(res)) == E_INVALID
    assert L.rtw_ctx_device_sweep(h, 3, 0, 256, 0, C.byref(res)) == E_INVALID
    assert L.rtw_ctx_device_sweep(h, R.SWEEP_DIV_RANDOM, 0, (1 << 32) + 1, 0, C.byref(res)) == E_INVALID
    assert L.rtw_ctx_device_sweep(h, R.SWEEP_SQRT, (1 << 32) - 16, 17, 0, C.byref(res)) == E_INVALID      # a bit pattern has 32 bits
    # every function, one wave and a bit: the shapes the Python wrapper promises
    for fn, (n_in, n_out) in R.MATH_COLS.items():
        got = gpu.device_math(fn, np.full((70, n_in), -0.5 if fn == R.MATH_EXP else 0.5, F))          # (exp_plain's domain is x <= 0)
        assert got.shape == ((70,) if n_out == 1 else (70, n_out)) and np.isfinite(got).all(), fn
