"""The kernels of the a-trous filter, the variance estimate, the variance-steered a-trous filter and the temporal accumulation
(rtw_ctx_atrous_filter, rtw_ctx_variance_estimate, rtw_ctx_svgf_filter, rtw_ctx_temporal_accumulate) directly against the float64
references of tests/filter_f64_common.py, within the bounds derived there: the matrix of tests/test_filter_f64_cpu.py, not through the
host forms.  Each level's inputs are the device's own outputs at one level less, so that the kernel is what is held to the reference and a
difference between device and host cannot cancel.  Every RTW_OPT_ATROUS_LAYOUT, at 33 x 17 and 17 x 33 (2 x 2 ragged workgroups) and at
32 x 16 (exactly one tile); once more with every buffer a torch tensor on the device."""
import numpy as np
import pytest

import rtw_amd as R
from tests import filter_f64_common as C
from tests.temporal_common import ALL_OFF, dyadic_camera

pytestmark = pytest.mark.gpu

LAYOUTS = [0, 1, 2]                                        # the measured choice, LDS tile wherever it fits, global memory
SHAPE_IDS = lambda s: f"{s[1]}x{s[0]}"


@pytest.fixture()
def layout(gpu, request):
    gpu.set_option(R.OPT_ATROUS_LAYOUT, request.param)
    yield request.param
    gpu.set_option(R.OPT_ATROUS_LAYOUT, 0)


def device_accumulate(r, h, w, wrap=lambda a: a):
    cam, depth = dyadic_camera(h, w), wrap(C.inputs(h, w)["depth"])
    return lambda cur, hist, **kw: r.temporal_accumulate(wrap(cur), cam, depth, history=hist, **kw, **ALL_OFF)


@pytest.mark.parametrize("case", C.level_cases(), ids=lambda c: f"{c[0]}-pre{c[1]}")
@pytest.mark.parametrize("shape", C.GPU_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_levels_one_at_a_time(gpu, layout, shape, case):
    (h, w), (terms, pre) = shape, case
    worst = C.assert_rows(C.run_levels(gpu.atrous_filter, gpu.svgf_filter, h, w, terms, pre), f"layout {layout} {w}x{h} {terms} prefilter {pre}")
    print(f"\n[f64 gpu] layout {layout} levels {w}x{h} {terms} prefilter {pre}: the largest error is {worst:.3f} of its bound", end="")


@pytest.mark.parametrize("shape", C.GPU_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_albedo_emission_and_the_floor_at_one_level(gpu, layout, shape):
    h, w = shape
    for name, terms, emi, pre in C.call_cases():
        worst = C.assert_rows(C.run_call(gpu.atrous_filter, gpu.svgf_filter, h, w, terms, emi, pre), f"layout {layout} {w}x{h} {name} prefilter {pre}")
        print(f"\n[f64 gpu] layout {layout} call {w}x{h} {name} prefilter {pre}: the largest error is {worst:.3f} of its bound", end="")


@pytest.mark.parametrize("shape", C.GPU_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("layout", LAYOUTS, indirect=True)
def test_variance_estimate(gpu, layout, shape):
    h, w = shape
    worst = max(C.assert_rows(C.run_variance(gpu.variance_estimate, h, w, *case), f"layout {layout} {w}x{h} estimate {case}") for case in C.variance_cases())
    print(f"\n[f64 gpu] layout {layout} estimate {w}x{h}: the largest error is {worst:.3f} of its bound", end="")


@pytest.mark.parametrize("shape", C.GPU_SHAPES, ids=SHAPE_IDS)
def test_temporal_statistics_of_static_frames(gpu, shape):
    """(The temporal kernel reads no window: RTW_OPT_ATROUS_LAYOUT does not reach it.)"""
    h, w = shape
    for case in C.TEMPORAL_CASES:
        worst = C.assert_rows(C.run_temporal(device_accumulate(gpu, h, w), h, w, *case), f"{w}x{h} temporal {case}")
        print(f"\n[f64 gpu] temporal {w}x{h} alpha {case[0]} alpha_moments {case[1]} max_history {case[2]}: the largest error is {worst:.3f} of its bound", end="")


def test_inputs_as_torch_tensors_on_the_device(gpu):
    """Every array a tensor on the device, read and written in place: one chain of levels with every term on, a call with albedo and
    emission, the estimate, and the temporal statistics."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.array(a)).to(dev) if isinstance(a, np.ndarray) else a
    down = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a

    def tensors(fn):
        def call(*args, **kw):
            res = fn(*(up(a) for a in args), **{k: up(v) for k, v in kw.items()})
            assert all(hasattr(a, "data_ptr") for a in res[:-1])                # (the results are tensors when the inputs are)
            return tuple(down(a) for a in res)
        return call

    h, w = 17, 33
    atrous, svgf = tensors(gpu.atrous_filter), tensors(gpu.svgf_filter)
    worst = C.assert_rows(C.run_levels(atrous, svgf, h, w, "var+guides", 1), "tensors, levels")
    worst = max(worst, C.assert_rows(C.run_levels(atrous, svgf, h, w, "all", 0), "tensors, a-trous levels"))
    worst = max(worst, C.assert_rows(C.run_call(atrous, svgf, h, w, "var+guides", True, 1), "tensors, call"))
    worst = max(worst, C.assert_rows(C.run_variance(tensors(gpu.variance_estimate), h, w, "all", 4, 3), "tensors, estimate"))
    step = device_accumulate(gpu, h, w, up)

    def accumulate(cur, hist, **kw):
        dev_hist, var = step(cur, hist["device"] if hist else None, **kw)[:2]
        assert hasattr(dev_hist["color"], "data_ptr")
        return dict({k: down(dev_hist[k]) for k in ("color", "moments", "len")}, device=dev_hist), down(var)

    worst = max(worst, C.assert_rows(C.run_temporal(accumulate, h, w, *C.TEMPORAL_CASES[3]), "tensors, temporal"))
    print(f"\n[f64 gpu] tensors on the device {w}x{h}: the largest error is {worst:.3f} of its bound", end="")
