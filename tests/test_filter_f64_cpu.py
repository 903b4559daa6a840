"""The host forms of the a-trous filter, the variance estimate, the variance-steered a-trous filter and the blending half of the temporal
accumulation against float64 references of their own, within bounds derived from the roundings (tests/filter_f64_common.py, whose
docstring holds the derivation).  The other tests of these passes show that the kernels, the host forms and float32 restatements agree
bit for bit; these show that what they agree on is the filter include/rtw.h describes, and how accurately.

  1. the inputs: at most 5 % of a case's pixels may have a bound above 2^-12 of the largest value in their window, so that a bound is a
     statement, and every term set must leave taps beside the centre alive at every level (the reference alone; no library call)
  2. the wrong rules: every entry of MUTANTS lies further than twice the bound from the reference somewhere in the matrix, and fails
     the assertion the tests below and tests/test_gpu_filter_f64.py make (the reference alone)
  3. the host forms, one level at a time, levels 1 .. 5; albedo, emission and the floor at levels = 1; the estimate; the temporal
     statistics over six static frames

Which term sets run at which level: LEVEL_TERMS' comment.  Every test prints its worst error as a share of its bound."""
import numpy as np
import pytest

import rtw_amd as R
from tests import filter_f64_common as C
from tests.temporal_common import ALL_OFF, dyadic_camera

SHAPE_IDS = lambda s: f"{s[1]}x{s[0]}"
LEVEL_IDS = lambda c: f"{c[0]}-pre{c[1]}"


# ---- 1. the inputs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_the_inputs_leave_the_bounds_a_statement(shape):
    h, w = shape
    worst, medians = {}, {}

    def note(label, bound, scale):
        over = C.over_the_line(bound, scale)
        assert over <= C.CONDITION_CAP, f"{label}: {over:.1%} of the pixels have a bound above 2^-12 of their window's largest value"
        key = label.split(":")[0]
        worst[key] = max(worst.get(key, 0.0), over)
        medians.setdefault(key, []).append(float(np.median(bound)))

    for terms, pre in C.level_cases():
        for i, (c_in, v_in, res) in enumerate(C.reference_chain(h, w, terms, pre)):
            for what, _value, bound in res:
                note(f"level {what}: {terms}, prefilter {pre}, level {i}", bound, C.window_max(c_in if what == "colour" else v_in, 2, 1 << i))
    frame, variance = C.inputs(h, w)["frame"], C.variance_plane(h, w)
    for name, terms, emi, pre in C.call_cases():
        for what, _got, _value, bound in C.check_call(h, w, terms, emi, pre, None, None):
            note(f"call {what}: {name}, prefilter {pre}", bound, C.window_max(frame if what == "colour" else variance, 2, 1))
    moments, length = C.history(h, w)
    for terms, mh, r in C.variance_cases():
        _value, bound = C.ref_variance64(moments, length, C.guides_of(h, w), C.variance_params(terms, mh, r))
        own = np.abs(moments.astype(np.float64)).max(-1)
        note(f"estimate: {terms}, min_history {mh}, radius {r}", bound, np.where(length >= mh, own, C.window_max(own, r, 1)))
    frames = C.temporal_frames(h, w)
    for alpha, am, mh in C.TEMPORAL_CASES:
        ref = C.ref_temporal_stats64(frames, alpha, am, mh)
        top = np.abs(frames.astype(np.float64)).max((0, 3))
        note(f"temporal colour: alpha {alpha}, max_history {mh}", ref["color"][1], top)
        note(f"temporal moments: alpha {alpha}, max_history {mh}", ref["moments"][1], np.maximum(top, top * top))
        note(f"temporal variance: alpha {alpha}, max_history {mh}", ref["variance"][1], top * top)
    for key in worst:
        print(f"\n[f64 inputs] {w}x{h} {key}: at most {worst[key]:.1%} of the pixels over the line, median bound {np.median(medians[key]):.2e}", end="")


@pytest.mark.parametrize("shape", C.SHAPES[2:], ids=SHAPE_IDS)
def test_every_term_set_leaves_taps_alive_at_every_level(shape):
    """LEVEL_TERMS' comment: the pixels whose taps beside the centre carry more than u of the weight sum are more than the 5 % that the
    condition on the inputs lets go without a statement."""
    h, w = shape
    for terms, pre in C.level_cases():
        for i, (c_in, v_in, _res) in enumerate(C.reference_chain(h, w, terms, pre)):
            alive = C.offcentre_share(terms, pre, h, w, i, c_in, v_in)
            assert (alive > C.U).mean() > C.CONDITION_CAP, (terms, pre, i, float((alive > C.U).mean()))
            print(f"\n[f64 inputs] {w}x{h} {terms} prefilter {pre} level {i}: taps beside the centre count at {(alive > C.U).mean():.0%} of the pixels, "
                  f"with {np.median(alive):.0%} of the weight at the median pixel", end="")


# ---- 2. the wrong rules ----------------------------------------------------------------------------------------------------------------------
def _mutant_rows(name):
    """Yields (label, wrong value, value, bound) over the matrix of the pass the wrong rule belongs to."""
    kind = C.MUTANTS[name][0]
    for h, w in C.SHAPES:
        if kind == "level":
            for terms, pre in C.level_cases():
                chain = C.reference_chain(h, w, terms, pre)
                for i, (c_in, v_in, res) in enumerate(chain):
                    wrong = C.check_level(terms, pre, h, w, i, c_in, v_in, None, None, v_call=chain[0][1], mutant=name)
                    for (what, value, bound), (_w, _g, bad, _b) in zip(res, wrong):
                        yield f"{w}x{h} {terms} prefilter {pre} level {i} {what}", bad, value, bound
        elif kind == "call":
            for cname, terms, emi, pre in C.call_cases():
                for (what, _g, value, bound), (_w, _g2, bad, _b) in zip(C.check_call(h, w, terms, emi, pre, None, None),
                                                                       C.check_call(h, w, terms, emi, pre, None, None, mutant=name)):
                    yield f"{w}x{h} {cname} prefilter {pre} {what}", bad, value, bound
        elif kind == "estimate":
            moments, length = C.history(h, w)
            for terms, mh, r in C.variance_cases():
                args = (moments, length, C.guides_of(h, w), C.variance_params(terms, mh, r))
                yield (f"{w}x{h} estimate {terms} min_history {mh} radius {r}", C.ref_variance64(*args, mutant=name)[0]) + C.ref_variance64(*args)
        else:
            for alpha, am, mh in C.TEMPORAL_CASES:
                good, bad = (C.ref_temporal_stats64(C.temporal_frames(h, w), alpha, am, mh, mutant=m) for m in (None, name))
                for k in ("color", "moments", "variance"):
                    yield (f"{w}x{h} temporal alpha {alpha} max_history {mh} {k}", bad[k][0]) + good[k]


def test_every_wrong_rule_is_caught():
    """Twice the bound: a kernel that computes the wrong rule is itself within one bound of it, so it stays outside the right rule's."""
    missed = []
    for name, (_kind, what) in C.MUTANTS.items():
        far = fails = 0
        for label, bad, value, bound in _mutant_rows(name):
            far += int((np.abs(bad - value) > 2.0 * bound).sum())
            fails += not C.holds(bad.astype(C.F), value, bound)
        print(f"\n[f64 wrong rules] {name}: {far} entries beyond twice the bound, {fails} assertions fail", end="")
        if not (far and fails):
            missed.append(f"{name} ({what})")
    assert not missed, "not caught: " + "; ".join(missed)


# ---- 3. the host forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.level_cases(), ids=LEVEL_IDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_levels_one_at_a_time(shape, case):
    (h, w), (terms, pre) = shape, case
    worst = C.assert_rows(C.run_levels(R.atrous_filter, R.svgf_filter, h, w, terms, pre), f"{w}x{h} {terms} prefilter {pre}")
    print(f"\n[f64 host] levels {w}x{h} {terms} prefilter {pre}: the largest error is {worst:.3f} of its bound", end="")


@pytest.mark.parametrize("case", C.call_cases(), ids=lambda c: f"{c[0]}-pre{c[3]}")
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_albedo_emission_and_the_floor_at_one_level(shape, case):
    (h, w), (name, terms, emi, pre) = shape, case
    worst = C.assert_rows(C.run_call(R.atrous_filter, R.svgf_filter, h, w, terms, emi, pre), f"{w}x{h} {name} prefilter {pre}")
    print(f"\n[f64 host] call {w}x{h} {name} prefilter {pre}: the largest error is {worst:.3f} of its bound", end="")


@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_variance_estimate(shape):
    h, w = shape
    worst = max(C.assert_rows(C.run_variance(R.variance_estimate, h, w, *case), f"{w}x{h} estimate {case}") for case in C.variance_cases())
    print(f"\n[f64 host] estimate {w}x{h}: the largest error is {worst:.3f} of its bound", end="")


def host_accumulate(h, w):
    cam, depth = dyadic_camera(h, w), C.inputs(h, w)["depth"]
    return lambda cur, hist, **kw: R.temporal_accumulate(cur, cam, depth, history=hist, **kw, **ALL_OFF)


@pytest.mark.parametrize("case", C.TEMPORAL_CASES, ids=lambda c: f"alpha{c[0]}-moments{c[1]}-max{c[2]}")
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_temporal_statistics_of_static_frames(shape, case):
    h, w = shape
    worst = C.assert_rows(C.run_temporal(host_accumulate(h, w), h, w, *case), f"{w}x{h} temporal {case}")
    print(f"\n[f64 host] temporal {w}x{h} alpha {case[0]} alpha_moments {case[1]} max_history {case[2]}: the largest error is {worst:.3f} of its bound", end="")
