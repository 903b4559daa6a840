"""The a-trous filter on the host (rtw_atrous_filter, include/rtw.h): the host form against an independent numpy
restatement bit for bit over frames, levels and terms with NaN, infinite and miss pixels and albedo at its floor, and over strips 259 pixels
long on which the taps of levels 7 and 8 land inside the frame and count; what the rule promises
of NaN pixels; the isolation the guides give; out == in; the argument checks."""
import ctypes as C

import numpy as np
import pytest

import rtw_amd as R
from tests.atrous_common import (DEEP_LEVELS, DEEP_SHAPES, DEEP_TERM_SETS, F, FLOOR, LEVELS, SHAPES, TERM_SETS, call_kwargs, deep_answer, deep_frame,
                                 host_answer, inputs, mismatch, ref_atrous, same_bits, taps_inside)


# ---- 1. the host form against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", list(TERM_SETS))
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_host_equals_restatement(shape, levels, terms):
    h, w = shape
    got = host_answer(h, w, terms, levels)
    want = ref_atrous(inputs(h, w)["frame"], **call_kwargs(h, w, terms, levels))
    assert same_bits(got, want), mismatch(got, want)


@pytest.mark.parametrize("terms", list(DEEP_TERM_SETS))
@pytest.mark.parametrize("levels", DEEP_LEVELS)
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_host_equals_restatement_with_taps_at_levels_7_and_8(shape, levels, terms):
    """259 pixels long: the taps of step 64 and step 128 land inside the frame (tests/atrous_common.py, DEEP_SHAPES)."""
    h, w = shape
    got = deep_answer(h, w, terms, levels)[0]
    want = ref_atrous(deep_frame(h, w), **call_kwargs(h, w, terms, levels))
    assert same_bits(got, want), mismatch(got, want)


@pytest.mark.parametrize("terms", list(DEEP_TERM_SETS))
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_the_taps_of_levels_7_and_8_count(shape, terms):
    """What the cases above are worth: the seventh and the eighth level each change the answer, through finite pixels, and the taps counted
    exceed the centre taps alone by those of step 64 and step 128."""
    h, w = shape
    out = {levels: deep_answer(h, w, terms, levels) for levels in (6, 7, 8)}
    assert all(np.isfinite(o).all(-1).mean() > 0.95 for o, _ in out.values())
    changed = lambda a, b: np.isfinite(a).all(-1) & np.isfinite(b).all(-1) & (a != b).any(-1)
    assert changed(out[8][0], out[7][0]).sum() > 100 and changed(out[7][0], out[6][0]).sum() > 100 and changed(out[8][0], out[6][0]).sum() > 100
    for levels in (7, 8):
        taps, centres = taps_inside(h, w, levels)
        assert out[levels][1] == taps and taps - taps_inside(h, w, levels - 1)[0] > h * w and taps > centres


def test_inputs_hold_the_specials():
    g = inputs(35, 67)
    assert np.isnan(g["frame"]).any() and np.isinf(g["frame"]).any() and np.isnan(g["depth"]).any()
    miss = g["ids"] < 0
    blank = lambda a: int((~(a[miss] != 0).any(-1)).sum())                # (a special may have landed on a miss pixel)
    assert miss.sum() > 100 and blank(g["normal"]) >= miss.sum() - 1 and blank(g["albedo"]) >= miss.sum() - 2
    assert (g["albedo"] == F(FLOOR)).any() and (g["albedo"] == np.nextafter(F(FLOOR), F(0.0))).any()
    assert g["emitted"].any() and len(np.unique(g["ids"])) == 4


def test_filter_does_something():
    """(the matrix compares two implementations of one rule: this one holds the rule to what a filter is for)"""
    rng = np.random.default_rng(2)
    clean = np.broadcast_to(np.array([0.3, 0.5, 0.7], F), (24, 40, 3))
    noisy = (clean + 0.1 * rng.standard_normal(clean.shape)).astype(F)
    out = R.atrous_filter(noisy, levels=4, sigma_color=0.0)[0]
    assert ((out - clean) ** 2).mean() < 0.05 * ((noisy - clean) ** 2).mean()
    flat = np.full((9, 11, 3), 0.25, F)                                   # a constant frame is a fixed point of the weighted mean ...
    assert np.abs(R.atrous_filter(flat, levels=8, sigma_color=1.0)[0] - flat).max() <= 2 ** -24      # ... up to the sum's rounding
    # albedo carries texture through: a textured, evenly lit surface comes back as it went in, up to the roundings of / and *
    tex = (0.2 + 0.6 * rng.random((24, 40, 3))).astype(F)
    lit = (tex * F(0.5)).astype(F)
    out = R.atrous_filter(lit, albedo=tex, levels=5, sigma_color=0.0, albedo_floor=FLOOR)[0]
    assert np.abs(out - lit).max() < 1e-6
    assert np.abs(R.atrous_filter(lit, levels=5, sigma_color=0.0)[0] - lit).max() > 0.05      # without it the texture is blurred away


# ---- 2. NaN pixels ----------------------------------------------------------------------------------------------------------------------
def test_nan_centre_keeps_its_value_and_nan_tap_drops_out():
    rng = np.random.default_rng(3)
    frame = (0.5 + 0.1 * rng.standard_normal((12, 14, 3))).astype(F)
    frame[5, 6] = np.nan
    frame[2, 9, 1] = np.inf
    out = R.atrous_filter(frame, levels=3, sigma_color=0.5)[0]
    assert np.isnan(out[5, 6]).all()
    assert np.isnan(out[2, 9]).all() or np.isinf(out[2, 9, 1])           # an infinite centre: every difference is inf or NaN, no tap is taken
    ok = np.ones((12, 14), bool)
    ok[5, 6] = ok[2, 9] = False
    assert np.isfinite(out[ok]).all()
    # the other pixels are those of a frame where the two are walled off by an object id
    ids = np.zeros((12, 14), np.int32)
    ids[5, 6], ids[2, 9] = 1, 2
    walled = frame.copy()
    walled[5, 6] = walled[2, 9] = 0.5
    ref = R.atrous_filter(walled, ids=ids, levels=3, sigma_color=0.5, same_object=True)[0]
    assert same_bits(out[ok], ref[ok])


# ---- 3. isolation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", ["ids", "depth"])
def test_other_object_never_reaches_a_pixel(guide):
    """With same_object -- or across a depth step under a tiny sigma_depth -- changing every pixel of B leaves A's bytes unchanged."""
    rng = np.random.default_rng(4)
    h, w = 21, 30
    b = np.zeros((h, w), bool)
    b[6:15, 9:22] = True
    b[0, :] = True
    frame = rng.random((h, w, 3)).astype(F)
    other = frame.copy()
    other[b] = (rng.random((int(b.sum()), 3)) * 50.0).astype(F)
    if guide == "ids":
        kw = dict(ids=b.astype(np.int32), same_object=True, sigma_color=0.8)
    else:
        kw = dict(depth=np.where(b, F(100.0), F(1.0)).astype(F), sigma_depth=1e-3, sigma_color=0.8)
    for levels in (1, 4, 8):
        one, two = R.atrous_filter(frame, levels=levels, **kw)[0], R.atrous_filter(other, levels=levels, **kw)[0]
        assert same_bits(one[~b], two[~b]), levels
        assert not same_bits(one[b], two[b])
        free = {k: v for k, v in kw.items() if k == "sigma_color"}
        assert not same_bits(R.atrous_filter(frame, levels=levels, **free)[0][~b], R.atrous_filter(other, levels=levels, **free)[0][~b])


# ---- 4. out == in ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", ["color", "all+albedo+emitted"])
def test_out_may_be_in(terms):
    h, w = 9, 17
    frame = inputs(h, w)["frame"].copy()
    out, _ = R.atrous_filter(frame, **call_kwargs(h, w, terms, 3), out=frame)
    assert out is frame and same_bits(frame, host_answer(h, w, terms, 3))


# ---- 5. stats and argument checks --------------------------------------------------------------------------------------------------------
def test_stats_count_the_taps_inside_the_frame():
    for (h, w), levels in (((1, 1), 8), ((3, 5), 3), ((35, 67), 8)):
        taps = 0
        for i in range(levels):
            taps += sum(max(0, w - abs(d) * 2 ** i) for d in range(-2, 3)) * sum(max(0, h - abs(d) * 2 ** i) for d in range(-2, 3))
        assert R.atrous_filter(np.zeros((h, w, 3), F), levels=levels)[1].taps == taps


def test_error_paths_host():
    frame = inputs(9, 17)["frame"].copy()
    g = inputs(9, 17)
    out = np.full_like(frame, 7.0)
    ip, op = C.c_void_p(frame.ctypes.data), C.c_void_p(out.ctypes.data)
    dp, np_, xp, ap, ep = (C.c_void_p(g[k].ctypes.data) for k in ("depth", "normal", "ids", "albedo", "emitted"))
    call = R.lib().rtw_atrous_filter

    def prm(levels=3, sc=0.5, sd=0.5, sn=0.5, same=1, floor=FLOOR):
        return C.byref(R.RtwAtrous(levels, sc, sd, sn, same, floor))

    def refused(*args):
        assert call(*args) == -1
        assert (out == 7.0).all()

    assert call(ip, 17, 9, dp, np_, xp, ap, ep, prm(), op, None) == 0                          # stats may be NULL
    assert call(ip, 17, 9, None, None, None, None, None, prm(sd=0.0, sn=0.0, same=0, floor=0.0), op, None) == 0     # off terms: NULL guides
    assert call(ip, 17, 9, dp, np_, xp, None, ep, prm(floor=float("nan")), op, None) == 0      # the floor is only read with an albedo
    assert call(ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=R.ATROUS_MAX_LEVELS), op, None) == 0
    out[:] = 7.0
    refused(None, 17, 9, dp, np_, xp, ap, ep, prm(), op, None)
    refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(), None, None)
    refused(ip, 17, 9, dp, np_, xp, ap, ep, None, op, None)
    refused(ip, 0, 9, dp, np_, xp, ap, ep, prm(), op, None)
    refused(ip, 17, 0, dp, np_, xp, ap, ep, prm(), op, None)
    refused(ip, 65536, 65536, dp, np_, xp, ap, ep, prm(), op, None)                            # w * h beyond 32 bits
    refused(ip, 0x7FFFFC01, 1, dp, np_, xp, ap, ep, prm(), op, None)                           # beyond RTW_ATROUS_MAX_SIDE
    refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=0), op, None)
    refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=R.ATROUS_MAX_LEVELS + 1), op, None)
    for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf"), 1e-20, 1e-30):
        refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(sc=v), op, None)
        refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(sd=v), op, None)
        refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(sn=v), op, None)
    # sigma_color halves per level: 1e-18 is fine for one level (0.5 / 1e-36), not for eight (0.5 / (1e-18 / 128)^2 overflows)
    assert call(ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=1, sc=1e-18), op, None) == 0
    out[:] = 7.0
    refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(levels=8, sc=1e-18), op, None)
    refused(ip, 17, 9, None, np_, xp, ap, ep, prm(), op, None)                                 # a term on with its guide NULL
    refused(ip, 17, 9, dp, None, xp, ap, ep, prm(), op, None)
    refused(ip, 17, 9, dp, np_, None, ap, ep, prm(), op, None)
    refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(same=2), op, None)
    for v in (0.0, -0.5, float("nan"), float("inf")):
        refused(ip, 17, 9, dp, np_, xp, ap, ep, prm(floor=v), op, None)
    # the Python layer: shapes and dtypes
    with pytest.raises(ValueError):
        R.atrous_filter(frame[..., :2])
    with pytest.raises(ValueError):
        R.atrous_filter(frame, depth=np.ones((9, 16), F))
    with pytest.raises(ValueError):
        R.atrous_filter(frame, albedo=np.ones((9, 17), F))
    with pytest.raises(ValueError):
        R.atrous_filter(frame, out=np.empty((9, 17, 3), np.float64))
    with pytest.raises(R.RtwError):
        R.atrous_filter(frame, levels=9)


def test_pod_layout():
    assert C.sizeof(R.RtwAtrous) == 24 and R.RtwAtrous.same_object.offset == 16 and R.RtwAtrous.albedo_floor.offset == 20
    assert R.lib().rtw_abi_version() == 4
    assert set(R.ATROUS_DEFAULTS) == {"levels", "sigma_color", "sigma_depth", "sigma_normal", "albedo_floor"}
