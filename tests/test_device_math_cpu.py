"""The reference of the device-math sweeps, tested without a GPU (include/rtw.h "device math, for tests", csrc/rtw_probe.h).

rtw_rounding_check is the integer predicate that the sweep kernels of rtw_ctx_device_sweep compile: "is this f32 the correctly rounded sqrt /
quotient".  Here it is held against numpy's float32 sqrt and divide (IEEE on the host) over the whole plain ranges and their edges, it has to
reject both f32 neighbours of every right answer, and it is compared with the same decision in Python integers of unbounded size, written
from the neighbours np.nextafter gives rather than from mantissa arithmetic.  The operands of the div_midpoint sweep are restated from their
definition, and their distance from a rounding boundary is computed exactly."""
import ctypes as C
from fractions import Fraction

import numpy as np

import rtw_amd as R

F = np.float32
U = np.uint32
E_INVALID, E_NO_DEVICE = -1, -2                        # rtw.h
SQRT_LO, SQRT_HI = 0x0F800000, 0x7F000000              # [2^-96, 2^127): what sqrt_ieee sends down the plain sequence
N_RANDOM = 1_000_000
N_BIG = 1 << 13                                        # how many of the random operands also go through Python integers (they are slow)


def f32(bits):
    return np.asarray(bits, U).view(F)


def bits(x):
    return np.asarray(x, F).view(U)


def pow2(e):
    return F(2.0) ** F(e)


def neighbours(x):
    """the f32 below and above, away from and towards zero regardless of sign"""
    x = np.asarray(x, F)
    inf = np.where(np.signbit(x), F(-np.inf), F(np.inf)).astype(F)
    hi = np.nextafter(x, inf)
    return np.where(x == 0, -hi, np.nextafter(x, F(0.0) * x)).astype(F), hi            # (a zero's: the smallest subnormals of either sign)


# ---- operands --------------------------------------------------------------------------------------------------------------------------
def sqrt_random():
    rng = np.random.default_rng(21)
    return f32(rng.integers(SQRT_LO, SQRT_HI, N_RANDOM, dtype=np.uint64).astype(U))


def sqrt_edges():
    k = np.arange(1, 4096, 2, dtype=np.float64)
    squares = [(k * k * 4.0 ** j).astype(F) for j in (-40, -1, 0, 7, 30)]                          # exact squares: k^2 has 24 bits at most
    j = np.arange(-48, 63, dtype=np.float64)
    four = (4.0 ** j).astype(F)                                                                   # roots with mantissa 0x800000 ...
    below = np.nextafter(four[1:], F(0))                                                            # ... and 0xFFFFFF: sqrt(4^j (1 - 2^-24)) rounds down
    top = (f32(U(0x3FFFFFFF) + (np.arange(-3, 4) * 2).astype(U)) * pow2(20)).astype(F)
    ends = np.array([pow2(-96), np.nextafter(pow2(-96), F(1)), f32(SQRT_HI - 1), f32(SQRT_HI - 2), 1.0, 2.0, 3.0, np.nextafter(F(1), F(2)),
                     np.nextafter(F(1), F(0)), np.nextafter(F(2), F(0)), np.nextafter(F(4), F(0))], F)
    return np.concatenate(squares + [four, below, np.nextafter(four, F(np.inf)), top, ends]).astype(F)


def div_random():
    rng = np.random.default_rng(22)

    def draw(e_lo, e_hi):
        m = rng.integers(0, 1 << 23, N_RANDOM, dtype=np.uint64)
        e = rng.integers(e_lo + 127, e_hi + 127, N_RANDOM, dtype=np.uint64)
        s = rng.integers(0, 2, N_RANDOM, dtype=np.uint64)
        return f32(((s << 31) | (e << 23) | m).astype(U))
    return draw(-60, 40), draw(-40, 40)                        # |n| in [2^-60, 2^40), |d| in [2^-40, 2^40)


def div_edges():
    up = lambda v: np.nextafter(F(v), F(np.inf))
    dn = lambda v: np.nextafter(F(v), F(0))
    ds = np.array([pow2(-40), up(pow2(-40)), 1.0, 3.0, dn(pow2(40)), pow2(40), dn(F(1)), up(F(1)), 0.1, 7.0], F)
    ns = np.array([0.0, pow2(-60), up(pow2(-60)), 1.0, dn(pow2(40)), pow2(40), 3.0, dn(F(1)), up(F(1))], F)
    n, d = [g.ravel() for g in np.meshgrid(ns, ds)]
    pairs = [(n * s1, d * s2) for s1 in (F(1), F(-1)) for s2 in (F(1), F(-1))]
    # exact quotients: n = q d with q and d of 12 bits each
    rng = np.random.default_rng(23)
    q = rng.integers(1, 4096, 512).astype(F); dd = rng.integers(1, 4096, 512).astype(F) * pow2(-17)
    pairs.append(((q * dd).astype(F), dd))
    # quotients at and next to a power of two: mantissa 0x800000 (n = d 2^j) and 0xFFFFFF (the f32 below that n)
    dr = f32((rng.integers(0, 1 << 23, 512, dtype=np.uint64) | (127 << 23)).astype(U))
    for j in (-20, 0, 13):
        nn = (dr * pow2(j)).astype(F)
        pairs += [(nn, dr), (dn(nn), dr), (up(nn), dr), (nn, -dr)]
    return np.concatenate([p[0] for p in pairs]).astype(F), np.concatenate([p[1] for p in pairs]).astype(F)


# ---- the same decisions in Python integers -----------------------------------------------------------------------------------------------
K = 400


def big(x):
    """|x| * 2^K as a Python integer (x a finite f32)"""
    m, e = np.frexp(np.float64(abs(float(x))))
    return int(np.ldexp(m, 53)) << (K + int(e) - 53)


def big_sqrt_ok(x, s):
    if not (np.isfinite(s) and s > 0):
        return False
    lo, hi = neighbours(s)
    return (big(s) + big(lo)) ** 2 < (big(x) << (K + 2)) < (big(s) + big(hi)) ** 2


def big_div_ok(n, d, q):
    if not np.isfinite(q) or bool(np.signbit(q)) != (bool(np.signbit(n)) != bool(np.signbit(d))):
        return False
    if n == 0:
        return q == 0
    if q == 0:
        return False
    lo, hi = neighbours(q)
    return big(d) * (big(q) + big(lo)) < (big(n) << (K + 1)) < big(d) * (big(q) + big(hi))


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------
def check_sqrt(x, n_big):
    s = np.sqrt(x)
    assert np.array_equal(s, np.sqrt(x.astype(np.float64)).astype(F))              # numpy's f32 sqrt is the rounded f64 one (53 >= 2 * 24 + 2)
    lo, hi = neighbours(s)
    assert R.rounding_check(R.SWEEP_SQRT, x, None, s).all()
    assert not R.rounding_check(R.SWEEP_SQRT, x, None, lo).any() and not R.rounding_check(R.SWEEP_SQRT, x, None, hi).any()
    for i in range(min(n_big, len(x))):
        assert big_sqrt_ok(x[i], s[i]) and not big_sqrt_ok(x[i], lo[i]) and not big_sqrt_ok(x[i], hi[i]), (x[i], s[i])
    return s


def check_div(n, d, n_big):
    q = n / d
    assert np.array_equal(q, (n.astype(np.float64) / d.astype(np.float64)).astype(F))
    lo, hi = neighbours(q)
    assert R.rounding_check(R.SWEEP_DIV_RANDOM, n, d, q).all()
    assert not R.rounding_check(R.SWEEP_DIV_RANDOM, n, d, lo).any() and not R.rounding_check(R.SWEEP_DIV_RANDOM, n, d, hi).any()
    assert not R.rounding_check(R.SWEEP_DIV_RANDOM, n, d, -q).any()                  # the other sign, a zero's included
    assert np.array_equal(R.rounding_check(R.SWEEP_DIV_MIDPOINT, n, d, q), R.rounding_check(R.SWEEP_DIV_RANDOM, n, d, q))
    for i in range(min(n_big, len(n))):
        assert big_div_ok(n[i], d[i], q[i]) and not big_div_ok(n[i], d[i], lo[i]) and not big_div_ok(n[i], d[i], hi[i]), (n[i], d[i], q[i])
        assert not big_div_ok(n[i], d[i], -q[i])
    return q


def test_sqrt_predicate_on_random_operands():
    x = sqrt_random()
    assert bits(x).min() < SQRT_LO + (1 << 20) and bits(x).max() > SQRT_HI - (1 << 20)
    check_sqrt(x, N_BIG)


def test_sqrt_predicate_on_the_edges():
    x = sqrt_edges()
    assert ((bits(x) >= SQRT_LO) & (bits(x) < SQRT_HI)).all()
    s = check_sqrt(x, len(x))
    man = bits(s) & U(0x7FFFFF)
    assert (man == 0).sum() > 100 and (man == 0x7FFFFF).sum() > 100                 # roots at both ends of a binade
    assert (s.astype(np.float64) ** 2 == x).sum() > 5000                            # exact squares
    for v in (pow2(-96), f32(SQRT_HI - 1)):
        assert v in x


def test_div_predicate_on_random_operands():
    n, d = div_random()
    check_div(n, d, N_BIG)


def test_div_predicate_on_the_edges():
    n, d = div_edges()
    ad, an = np.abs(d), np.abs(n)
    assert ((ad >= pow2(-40)) & (ad <= pow2(40))).all() and ((an == 0) | ((an >= pow2(-60)) & (an <= pow2(40)))).all()
    q = check_div(n, d, len(n))
    man = bits(q) & U(0x7FFFFF)
    assert ((man == 0) & (q != 0)).sum() > 3000 and (man == 0x7FFFFF).sum() > 1000
    assert (q.astype(np.float64) * d.astype(np.float64) == n).sum() > 3000          # exact quotients
    assert (q == 0).sum() >= 40 and np.signbit(q[q == 0]).any() and not np.signbit(q[q == 0]).all()
    for v in (pow2(-40), pow2(40)):
        assert v in ad
    for v in (pow2(-60), pow2(40)):
        assert v in an


def test_predicates_refuse_what_is_outside_their_domain():
    """A result of any other class is never `correctly rounded`: NaN, inf, subnormal, a negative root, a subnormal or zero divisor."""
    one = np.ones(6, F)
    bad = np.array([np.nan, np.inf, -1.0, 1e-40, 0.0, -0.0], F)
    assert not R.rounding_check(R.SWEEP_SQRT, one, None, bad).any()
    assert not R.rounding_check(R.SWEEP_SQRT, np.array([0.0, -1.0, 1e-40, np.inf, np.nan], F), None, np.array([0.0, 1.0, 1e-20, np.inf, np.nan], F)).any()
    assert not R.rounding_check(R.SWEEP_DIV_RANDOM, one[:4], one[:4], bad[:4]).any()
    assert not R.rounding_check(R.SWEEP_DIV_RANDOM, one[:4], np.array([0.0, 1e-40, np.inf, np.nan], F), one[:4]).any()
    # a root or quotient that is off by a binade, not by an ulp
    assert not R.rounding_check(R.SWEEP_SQRT, [F(4.0)] * 2, None, [F(1.0), F(4.0)]).any()
    assert not R.rounding_check(R.SWEEP_DIV_RANDOM, [F(1.0)] * 2, [F(3.0)] * 2, [F(1 / 6), F(2 / 3)]).any()


# ---- the div_midpoint construction, from its definition -------------------------------------------------------------------------------------
def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    return x


def draw(seed, index, k):
    h = mix32(seed + 0x9E3779B9)
    h = mix32(h ^ (index >> 32))
    h = mix32(h ^ (index & 0xFFFFFFFF))
    return mix32(h ^ ((0x85EBCA6B * (k + 1)) & 0xFFFFFFFF))


def frame(r):
    return r & 1, (r >> 1) & 1, -60 + ((((r >> 17) & 0x7FFF) * 100) >> 15), -40 + ((((r >> 2) & 0x7FFF) * 80) >> 15)      # neg_n, neg_d, en, ed


def to_f32(neg, m, e):
    assert 1 << 23 <= m < 1 << 24 and -126 <= e <= 127
    return f32(U((neg << 31) | ((e + 127) << 23) | (m & 0x7FFFFF)))[()]


def midpoint_pair(seed, index):
    """(n, d, c, k): md an odd draw; c the odd 25-bit integer with c md = +-1 (mod 2^k); mn = (c md -+ 1) / 2^k with 24 bits."""
    neg_n, neg_d, en, ed = frame(draw(seed, index, 0))
    md = (1 << 23) | (draw(seed, index, 1) & 0x7FFFFF) | 1
    above = draw(seed, index, 2) & 1
    for side in (above, above ^ 1):                    # the side the draw asks for, else the other one
        for k in (25, 24):
            res = pow(md, -1, 1 << k)
            res = (1 << k) - res if side else res
            c = res if k == 25 else res | (1 << 24)
            mn, rem = divmod(c * md + (1 if side else -1), 1 << k)
            if rem == 0 and c >> 24 == 1 and 1 << 23 <= mn < 1 << 24 and (k == 24 or (c * md) >> 48):
                return to_f32(neg_n, mn, en), to_f32(neg_d, md, ed), c, k
    raise AssertionError((seed, index))


def boundary_distance_ulp(n, d):
    """exact distance of n / d from the nearer rounding boundary of f32, in ulps of the rounded quotient"""
    exact = Fraction(float(n)) / Fraction(float(d))
    q = F(n) / F(d)
    lo, hi = neighbours(q)
    ulp = abs(Fraction(float(hi)) - Fraction(float(q)))
    mids = [(Fraction(float(q)) + Fraction(float(v))) / 2 for v in (lo, hi)]
    return min(abs(exact - m) for m in mids) / ulp


def test_div_midpoint_operands_sit_on_a_rounding_boundary():
    count = 6000
    for seed in (1, 0xC0FFEE):
        first = (seed * 977) << 20                                                        # beyond 2^32 too: the index is 64 bits wide
        n, d = R.sweep_operands(R.SWEEP_DIV_MIDPOINT, first, count, seed)
        an, ad = np.abs(n), np.abs(d)
        assert ((ad >= pow2(-40)) & (ad < pow2(40))).all() and ((an >= pow2(-60)) & (an < pow2(40))).all()
        worst, sides = Fraction(0), set()
        for i in range(count):
            pn, pd, c, k = midpoint_pair(seed, first + i)
            assert (pn, pd) == (n[i], d[i]), (seed, i, pn, pd, n[i], d[i])
            dist = boundary_distance_ulp(n[i], d[i])
            assert 0 < dist <= Fraction(1, 1 << 24), (seed, i, n[i], d[i], float(dist))
            worst = max(worst, dist)
            sides.add(F(n[i]) / F(d[i]) > 0 and abs(Fraction(float(n[i])) / Fraction(float(d[i]))) > abs(Fraction(float(F(n[i]) / F(d[i])))))
        print(f"div_midpoint seed {seed:#x}: {count} pairs, farthest {float(worst) * 2 ** 24:.4f} x 2^-24 ulp from a boundary")
        assert len(sides) == 2                                                            # quotients that round down and quotients that round up
        # every sign combination and both ends of both exponent ranges occur
        assert len({(bool(a), bool(b)) for a, b in zip(np.signbit(n), np.signbit(d))}) == 4
        e_n, e_d = np.frexp(an)[1] - 1, np.frexp(ad)[1] - 1
        assert e_n.min() == -60 and e_n.max() == 39 and e_d.min() == -40 and e_d.max() == 39
        assert R.rounding_check(R.SWEEP_DIV_MIDPOINT, n, d, n / d).all()


def test_div_random_operands_cover_the_ranges():
    n, d = R.sweep_operands(R.SWEEP_DIV_RANDOM, (1 << 33) + 5, 200000, 7)
    for i in (0, 1, 77777, 199999):
        neg_n, neg_d, en, ed = frame(draw(7, (1 << 33) + 5 + i, 0))
        assert n[i] == to_f32(neg_n, (1 << 23) | (draw(7, (1 << 33) + 5 + i, 1) & 0x7FFFFF), en)
        assert d[i] == to_f32(neg_d, (1 << 23) | (draw(7, (1 << 33) + 5 + i, 2) & 0x7FFFFF), ed)
    an, ad = np.abs(n), np.abs(d)
    e_n, e_d = np.frexp(an)[1] - 1, np.frexp(ad)[1] - 1
    assert e_n.min() == -60 and e_n.max() == 39 and e_d.min() == -40 and e_d.max() == 39
    # uniform over the exponents: each of the 100 / 80 binades holds its share within 5 standard deviations
    for e, lo, k in ((e_n, -60, 100), (e_d, -40, 80)):
        h = np.bincount(e - lo, minlength=k)
        assert np.abs(h - len(e) / k).max() < 5 * np.sqrt(len(e) / k), h
    assert len({(bool(a), bool(b)) for a, b in zip(np.signbit(n[:64]), np.signbit(d[:64]))}) == 4
    m = bits(n) & U(0x7FFFFF)
    assert m.min() < 1 << 10 and m.max() > (1 << 23) - (1 << 10) and len(np.unique(m)) > 190000
    other = R.sweep_operands(R.SWEEP_DIV_RANDOM, (1 << 33) + 5, 64, 8)
    assert not np.array_equal(other[0], n[:64])                                            # the seed matters


# ---- argument checks that need no device ------------------------------------------------------------------------------------------------------
def test_argument_checks_without_a_device():
    L = R.lib()
    x = np.ones(4, F); out = np.empty(4, F)
    fp = C.POINTER(C.c_float)
    xp, op = x.ctypes.data_as(fp), out.ctypes.data_as(fp)
    res = R.RtwSweepResult()
    # no context: RTW_E_INVALID whatever else is passed
    assert L.rtw_ctx_device_math(None, R.MATH_SQRT_PLAIN, xp, 1, 4, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(None, R.MATH_SQRT_PLAIN, None, 1, 4, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(None, R.MATH_SQRT_PLAIN, xp, 1, 0, op, 1) == E_INVALID
    assert L.rtw_ctx_device_math(None, 13, xp, 1, 4, op, 1) == E_INVALID
    assert L.rtw_ctx_device_sweep(None, R.SWEEP_SQRT, SQRT_LO, 1024, 0, C.byref(res)) == E_INVALID
    assert L.rtw_ctx_device_sweep(None, R.SWEEP_SQRT, SQRT_LO, 1024, 0, None) == E_INVALID
    assert L.rtw_ctx_device_sweep(None, 3, 0, 1024, 0, C.byref(res)) == E_INVALID
    if R.device_count() == 0:                          # ... and there is none to be had: no CPU evaluation stands in
        h = C.c_void_p()
        assert L.rtw_ctx_create(0, C.byref(h)) == E_NO_DEVICE and not h.value
        try:
            R.Renderer(0)
            raise AssertionError("a context without a device")
        except R.RtwError as e:
            assert e.status == E_NO_DEVICE
    # the host entry points
    a = np.ones(4, U); ok = np.empty(4, np.uint8)
    assert L.rtw_rounding_check(R.SWEEP_SQRT, a.ctypes.data, None, a.ctypes.data, 4, ok.ctypes.data) == 0
    assert L.rtw_rounding_check(R.SWEEP_DIV_RANDOM, a.ctypes.data, None, a.ctypes.data, 4, ok.ctypes.data) == E_INVALID
    assert L.rtw_rounding_check(R.SWEEP_SQRT, None, None, a.ctypes.data, 4, ok.ctypes.data) == E_INVALID
    assert L.rtw_rounding_check(R.SWEEP_SQRT, a.ctypes.data, None, None, 4, ok.ctypes.data) == E_INVALID
    assert L.rtw_rounding_check(R.SWEEP_SQRT, a.ctypes.data, None, a.ctypes.data, 4, None) == E_INVALID
    assert L.rtw_rounding_check(R.SWEEP_SQRT, a.ctypes.data, None, a.ctypes.data, 0, ok.ctypes.data) == E_INVALID
    assert L.rtw_rounding_check(3, a.ctypes.data, a.ctypes.data, a.ctypes.data, 4, ok.ctypes.data) == E_INVALID
    pairs = np.empty((4, 2), U)
    assert L.rtw_sweep_operands(R.SWEEP_DIV_MIDPOINT, 0, 4, 0, pairs.ctypes.data) == 0
    assert L.rtw_sweep_operands(R.SWEEP_SQRT, 0, 4, 0, pairs.ctypes.data) == E_INVALID
    assert L.rtw_sweep_operands(R.SWEEP_DIV_RANDOM, 0, 4, 0, None) == E_INVALID
    assert L.rtw_sweep_operands(R.SWEEP_DIV_RANDOM, 0, 0, 0, pairs.ctypes.data) == E_INVALID
    assert C.sizeof(R.RtwSweepResult) == 24 + 16 * R.SWEEP_RECORDS + 8
    assert sorted(R.MATH_COLS) == list(range(13))
