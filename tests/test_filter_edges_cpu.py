"""The post-process pass (csrc/rtw_filter.hip) at its value, size and sum-order edges, on the host: the library's host path against the numpy
references of filter_edges_common.py, exactly -- and the self-checks that make the same cases worth running on the GPU
(test_gpu_filter_edges.py): the quantisation values tell the rounding rules apart, the thin frames pin the order of the gradient sum, and
every non-finite guide case leaves a live frame that differs from the one ordinary guides give."""
import numpy as np
import pytest

import rtw_amd as R
from tests import filter_edges_common as E
from tests.guided_common import mismatch, ref_guided
from tests.test_bilateral_cpu import F, ref_avg_gradient, ref_bilateral


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- A. quantisation at its ties and specials ----------------------------------------------------------------------------------------
def test_value_set_tells_the_rounding_rules_apart():
    v = E.quantize_values()
    ref = E.ref_quantize_rust2(v)
    p = E.product(v).astype(np.float64)
    with np.errstate(invalid="ignore"):
        exact = np.isfinite(p) & (p - np.floor(p) == 0.5)
        above_even = np.floor(p) % 2 == 0
    assert len(E.tie_values()) == 1792 and exact.sum() >= 256
    ties = exact & (p > 0) & (p < 255)                                                        # (255.5 is clamped to 255 before it is rounded)
    assert np.array_equal(ref[ties], np.floor(p[ties]) + 1)                                  # a tie goes up: away from zero
    even = E.quantize_half_even(v) != ref
    assert even.sum() >= 100 and np.array_equal(even, ties & above_even)         # ties above an even integer, and only those
    plus_half = np.nonzero(E.quantize_floor_plus_half_f32(v) != ref)[0]
    assert len(plus_half) >= 1
    assert any(E.product(v[i]) == np.nextafter(F(0.5), F(0.0)) and ref[i] == 0 for i in plus_half)      # pred(0.5) + 0.5f rounds to 1
    # the specials, spelled out
    for c, want in ((0.0, 0), (-0.0, 0), (2.0 ** -149, 0), (-(2.0 ** -149), 0), (2.0 ** -126, 0), (1.0, 255), (-1e-3, 0), (1e30, 255),
                    (-1e30, 0), (3.4e38, 255), (np.inf, 255), (-np.inf, 0), (np.nan, 0)):
        assert E.ref_quantize_rust2(F(c)) == want, c
    assert np.isinf(E.product(F(3.4e38)))
    assert np.isnan(E.special_values()).sum() == 4 and len(set(E.bits(E.special_values()[-4:]).tolist())) == 4


def test_host_quantise_equals_the_reference_on_the_value_set():
    v = E.quantize_values()
    got, ref = R.quantize_u8_rust2(v), E.ref_quantize_rust2(v)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, [(v[i], E.product(v[i]), got[i], ref[i]) for i in bad[:5]]
    assert np.array_equal(R.quantize_u8_rust2(E.quantize_frame()), E.ref_quantize_rust2(E.quantize_frame()))


def test_read_out_holds_for_every_byte():
    """Size 1, Edges, avg_gradient 1: the filter's output outside the last row and column IS its input byte, for all 256 of them -- through
    the numpy restatement and through the host path -- so a filter call shows what the quantise step wrote."""
    img = np.zeros((17, 17, 3), np.uint8)
    img[:16, :16] = np.arange(256, dtype=np.uint8).reshape(16, 16, 1) + np.array([0, 85, 170], np.uint8)       # every byte in every channel
    assert all(len(np.unique(img[:16, :16, c])) == 256 for c in range(3))
    ref, _, taps = ref_bilateral(img, 1, True, avg=1.0)
    assert taps == 16 * 16
    E.check_read_out(ref, img)
    out, st = R.bilateral_filter(img, **E.READ_OUT)
    assert st.taps == taps
    E.check_read_out(out, img)
    E.check_read_out(R.guided_filter(img, **E.READ_OUT)[0], img)
    # and the f32 frame of the value set through the host filters
    frame = E.quantize_frame()
    want = E.ref_quantize_rust2(frame)
    E.check_read_out(R.bilateral_filter(frame, **E.READ_OUT)[0], want)
    E.check_read_out(R.guided_filter(frame, **E.READ_OUT)[0], want)


# ---- B. the gradient sum at vector, chunk and tail boundaries ------------------------------------------------------------------------
def test_term_counts_cover_the_boundaries():
    assert {n % 4 for n in E.TERM_COUNTS} == {0, 1, 2, 3} and {n % 4 for n in E.TERM_COUNTS if n > 2048} == {0, 1, 2, 3}
    assert {2047, 2048, 2049, 4095, 4096, 4097, 255, 256, 257} <= set(E.TERM_COUNTS)
    assert [n % 2048 for n in E.TAIL_COUNTS] == [1, 2, 3, 1]
    for o, shape in (("wide", (3, 2051, 3)), ("tall", (2051, 3, 3))):
        assert E.thin_frame(2049, o).shape == shape


@pytest.mark.parametrize("n", E.TERM_COUNTS)
def test_thin_frames_pin_the_order_and_the_host_keeps_it(n):
    for o in E.ORIENTATIONS:
        img = E.thin_frame(n, o)
        terms = E.gradient_terms(img)
        avg = E.thin_avg(n, o)
        assert len(terms) == n and same_bits(avg, F(E.serial_sum(terms) / F(n)))             # gradient_terms are the reference's terms
        if n >= 64:
            for how, s in E.other_order_sums(terms).items():                                 # any other association is visible in avg
                assert not same_bits(s, E.serial_sum(terms)) and not same_bits(F(s / F(n)), avg), (n, o, how)
        out, st = R.bilateral_filter(img, 3)
        assert same_bits(st.avg_gradient, avg), (n, o, st.avg_gradient, avg)
        assert st.spatial == np.ceil(F(F(0.02) * np.sqrt(F(img.shape[0] ** 2 + img.shape[1] ** 2))))
        if n <= E.REF_BYTES_MAX_N:
            ref, taps = E.thin_bytes(n, o)
            assert st.taps == taps and mismatch(out, ref) is None, (n, o, mismatch(out, ref))


@pytest.mark.parametrize("n,last,value", list(E.single_term_cases()), ids=E.SINGLE_TERM_IDS)
def test_single_term_known_answer(n, last, value):
    img, want = E.single_term_frame(n, last, value)
    terms = E.gradient_terms(img)
    assert np.count_nonzero(terms) == 1 and terms[n - 1 if last else 0] > 0
    assert want > 0 and same_bits(ref_avg_gradient(img), want)
    _, st = R.bilateral_filter(img, 1)
    assert same_bits(st.avg_gradient, want), (st.avg_gradient, want)


# ---- C. the guided filter with non-finite and extreme guides -------------------------------------------------------------------------
def test_guided_case_table_holds_what_it_names():
    h, w = E.GUIDED_SHAPES[0]
    g = {name: E.guided_case(name, h, w) for name in E.GUIDED_CASES}
    assert np.isnan(g["depth-nan"]["depth"]).any() and np.isfinite(g["depth-nan"]["depth"]).any()
    inf = g["depth-plus-inf"]["depth"] == np.inf
    assert (inf[:, 1:] & inf[:, :-1]).any() and (inf[:, 1:] & np.isfinite(g["depth-plus-inf"]["depth"][:, :-1])).any()
    assert (g["depth-minus-inf"]["depth"] == -np.inf).any() and np.isnan(g["depth-all-nan"]["depth"]).all()
    with np.errstate(over="ignore"):
        for name, v in (("depth-3e38", 3e38), ("depth-1e20", 1e20)):
            d = g[name]["depth"]
            assert (d == F(v)).any() and (d == F(-v)).any() and np.isfinite(d).all()
            dz = d[:, 1:] - d[:, :-1]
            assert np.isinf(dz * dz).any() and np.isinf(dz).any() == (v == 3e38)             # 3e38: dz overflows; 1e20: only dz * dz
    tiny = F(2.0 ** -126)
    for name, key in (("depth-sigma-1e19", "sigma_depth"), ("normal-sigma-1e19", "sigma_normal")):
        inv = F(F(0.5) / F(F(g[name][key]) * F(g[name][key])))
        assert 0 < inv < tiny                                                                # a denormal inv_*
    for name, key in (("depth-sigma-1e-19", "sigma_depth"), ("normal-sigma-1e-19", "sigma_normal")):
        assert np.isfinite(F(F(0.5) / F(F(g[name][key]) * F(g[name][key]))))
    d = g["depth-sigma-1e19"]["depth"]
    for dz in (np.abs(d[:, 1:] - d[:, :-1]), np.abs(d[1:] - d[:-1])):
        a = F(5e-39) * dz.astype(np.float64) ** 2
        assert (dz > 0.9e18).all() and (dz < 1.1e19).all() and a.min() > 0.004 and a.max() < 0.61
    dz = np.abs(np.diff(g["depth-sigma-1e-19"]["depth"], axis=1))
    assert ((dz * dz)[dz > 0] < tiny).any()                                                  # a denormal dz * dz
    n = g["normal-nonfinite"]["normal"]
    assert np.isnan(n).any() and (n == np.inf).any() and (n == -np.inf).any()
    assert (np.abs(g["normal-1e20"]["normal"]) == F(1e20)).any()
    assert all((~g[name]["normal"].any(axis=2)).any() for name in ("normal-nonfinite", "normal-1e20"))      # the 0 0 0 of a miss is there
    assert {E.I32_MIN, E.I32_MAX, -1, -2, 0} <= set(g["ids-extremes"]["ids"].ravel().tolist())
    c = g["combined"]
    bad_d, bad_n = ~np.isfinite(c["depth"]), ~np.isfinite(c["normal"]).all(axis=2)
    assert bad_d.any() and bad_n.any() and (bad_d ^ bad_n).any() and len(np.unique(c["ids"])) == 5


@pytest.mark.parametrize("h,w", E.GUIDED_SHAPES, ids=[f"{w}x{h}" for h, w in E.GUIDED_SHAPES])
@pytest.mark.parametrize("name", list(E.GUIDED_CASES))
def test_host_guided_equals_the_reference_and_the_case_is_live(name, h, w):
    img = E.guided_image(h, w)
    kw = E.guided_case(name, h, w)
    for size in E.GUIDED_SIZES:
        for prox in E.PROXIMITIES:
            ref = E.guided_ref(name, h, w, size, prox)
            out, st = R.guided_filter(img, size, proximity=prox, avg_gradient=E.GUIDED_AVG, **kw)
            assert st.avg_gradient == F(E.GUIDED_AVG) and mismatch(out, ref) is None, (size, prox, mismatch(out, ref))
            # liveness: the edge values do something, and (but for the all-NaN plane) they have not blacked the frame out
            edges = prox == R.PROXIMITY_EDGES
            ordinary = ref_guided(img, size, edges, E.GUIDED_AVG, **E.ordinary_guides(kw, h, w))
            assert not np.array_equal(ref, ordinary), (size, prox)
            assert ref.any() != (name in E.BLACK_CASES), (size, prox)
            dead = E.dead_centres(kw)
            if dead is not None:                            # known answer: a centre with a NaN or infinite depth gives 0 0 0
                assert not ref[dead].any() and dead.any() == (name in E.DEAD_CENTRE_CASES)
            if name in E.DENORMAL_CASES:                    # with the term off -- what a flushed inv_* or dz * dz amounts to -- >= 1 % of the pixels change
                off = dict(kw, **{E.DENORMAL_CASES[name]: 0.0})
                changed = (ref != ref_guided(img, size, edges, E.GUIDED_AVG, **off)).any(axis=2).mean()
                assert changed >= 0.01, (size, prox, changed)


# ---- D. frame geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", E.GEOMETRY_SHAPES, ids=[f"{w}x{h}" for h, w in E.GEOMETRY_SHAPES])
def test_host_filters_on_small_geometries(h, w):
    img = E.geometry_image(h, w)
    avg = ref_avg_gradient(img)
    gk = E.geometry_guides(h, w)
    for size in E.GEOMETRY_SIZES:
        for prox in E.PROXIMITIES:
            edges = prox == R.PROXIMITY_EDGES
            ref, _, taps = ref_bilateral(img, size, edges, avg=avg)
            out, st = R.bilateral_filter(img, size, prox)
            assert same_bits(st.avg_gradient, avg) and st.taps == taps and mismatch(out, ref) is None, (size, prox, mismatch(out, ref))
            out, st = R.guided_filter(img, size, proximity=prox, **gk)
            ref = ref_guided(img, size, edges, avg, **gk)
            assert same_bits(st.avg_gradient, avg) and st.taps == taps and mismatch(out, ref) is None, (size, prox, mismatch(out, ref))


@pytest.mark.parametrize("avg", E.AVG_EXTREMES)
def test_given_avg_gradient_extremes(avg):
    h, w = 17, 33
    img = E.geometry_image(h, w)
    a = F(avg)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        sq = F(a * a)
        inv_range = F(F(0.5) / sq)
    for prox in E.PROXIMITIES:
        ref, _, _ = ref_bilateral(img, 3, prox == R.PROXIMITY_EDGES, avg=avg)
        out, st = R.bilateral_filter(img, 3, prox, avg_gradient=avg)
        assert same_bits(st.avg_gradient, a) and mismatch(out, ref) is None, (prox, mismatch(out, ref))
        if avg == 1e-30:
            assert sq == 0 and np.isinf(inv_range) and not ref.any()                         # exp(inf * 0) = NaN on the centre tap: all zero
        elif avg == 1e-19:
            assert 0 < sq < F(2.0 ** -126) and np.isfinite(inv_range) and ref.any()
        else:                                                                                # purely spatial: the bytes of any other such avg
            assert np.isinf(sq) and inv_range == 0 and ref.any()
            assert np.array_equal(ref, ref_bilateral(img, 3, prox == R.PROXIMITY_EDGES, avg=1e25)[0])
