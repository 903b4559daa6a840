#!/usr/bin/env python3
"""exp_plain (csrc/rtw_exp.h) against f64 exp over EVERY f32 in [-104, 0]: the maximum error in ulp, for DESIGN.md 8b and the bound of
tests/test_guided_cpu.py.  Host only (rtw_exp_plain is the definition the kernel compiles); about 1.1e9 arguments, a few minutes.

The error of one argument (tests/guided_common.py ulp_error, the test's own measure): |got - exp(x)| in units of the f32 spacing at exp(x), where
exp(x) >= 2^-126.  Below 2^-126 the required result is +0, which is what must come back (counted in `not_flushed` otherwise); a result that
is +0 although exp(x) >= 2^-126 (`early_flush`) is counted by exp(x)'s distance above 2^-126, the threshold the unflushed value missed.

    python scripts/sweep_exp_plain.py [--procs N]
"""
import argparse
import multiprocessing as mp
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.guided_common import ulp_error       # noqa: E402

CHUNK = 1 << 22


def sweep(span):
    import rtw_amd as R
    lo, hi = span
    worst, at, early, late = 0.0, 0.0, 0, 0
    for b in range(lo, hi, CHUNK):
        x = np.arange(b, min(hi, b + CHUNK), dtype=np.uint32).view(np.float32)
        err, ef, nf = ulp_error(x, R.exp_plain(x))
        i = int(np.argmax(err))
        if err[i] > worst:
            worst, at = float(err[i]), float(x[i])
        early += int(ef.sum())
        late += int(nf.sum())
    return worst, at, early, late


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    lo = int(np.float32(-0.0).view(np.uint32))               # the bit patterns of -0 .. -104 are consecutive integers
    hi = int(np.float32(-104.0).view(np.uint32)) + 1
    step = (hi - lo + 4 * a.procs - 1) // (4 * a.procs)
    spans = [(b, min(hi, b + step)) for b in range(lo, hi, step)]
    with mp.Pool(a.procs) as pool:
        res = pool.map(sweep, spans)
    worst, at = max((r[0], r[1]) for r in res)
    print(f"exp_plain over all {hi - lo} f32 in [-104, -0]: max error {worst:.4f} ulp at x = {at!r}; "
          f"flushed although exp(x) >= 2^-126: {sum(r[2] for r in res)}; not flushed although exp(x) < 2^-126: {sum(r[3] for r in res)}")


if __name__ == "__main__":
    main()
