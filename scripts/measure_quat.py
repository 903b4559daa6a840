#!/usr/bin/env python3
"""Cost of the quaternion transform: Rust2's rotation_test scene (tests/golden/rust2_rotation_scene.json) at 400 x 400 x 25, depth 2, under
RTW_INTEGRATOR_RUST2 -- with the instance rotation set (the quaternion build, SPEC 11) and with no rotation set (the same quads, Euler rotation
0: the existing Rust2 build, SPEC 5) -- ms per frame (render kernel and resolve, median), segments and G segments/s, and the ratio.  The two
frames are different pictures (the box is turned in one), so the segment counts differ a little; the ratio of ms per segment is printed too.
Then the same pair with one top-level sphere list of 60 (the tree kernels).

    python scripts/measure_quat.py [repeats]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtw_amd as R                      # noqa: E402
from tests import quat_common as Q       # noqa: E402


def run(gpu, cam, p, reps):
    gpu.render(cam, p)
    ms, st = [], None
    for _ in range(reps):
        _, st = gpu.render(cam, p)
        ms.append(st.kernel_ms)
    return float(np.median(ms)), min(ms), max(ms), st


def field(n=60, seed=4):
    rng = np.random.default_rng(seed)
    return [{"origin": [float(rng.uniform(-4, 3)), float(rng.uniform(-2, 2)), float(rng.uniform(2.5, 8))], "radius": float(rng.uniform(0.1, 0.4)),
             "material": "lambertian", "color": [0.5, 0.5, 0.5], "emitted": [0.0, 0.0, 0.0]} for _ in range(n)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    g = Q.golden()
    w = h = 400
    cam = Q.camera(g, w, h)
    with R.Renderer(0) as gpu:
        for name, qs in (("rotation_test scene (one box instance: the list walk)", Q.fixture_scene(g)),
                         ("rotation_test scene + 60 spheres (the tree)", Q.fixture_scene(g, spheres=field()))):
            print(name)
            p = qs.params(w, h, R.INTEGRATOR_RUST2, g["depth"], samples=g["samples"], accel=R.ACCEL_BVH)
            out = {}
            for label, rot in (("quaternion set (SPEC 11)", True), ("no rotation  (SPEC 5) ", False)):
                qs.install(gpu, rotations=rot)
                med, lo, hi, st = run(gpu, cam, p, reps)
                out[rot] = (med, st.segments)
                print(f"  {label} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} runs)  {st.segments} segments  "
                      f"{st.segments / med / 1e6:7.3f} G segments/s  kernel: {'render_bvh' if st.node_tests else 'render_brute'}")
            print(f"  ratio quaternion / none: {out[True][0] / out[False][0]:.3f} per frame, "
                  f"{(out[True][0] / out[True][1]) / (out[False][0] / out[False][1]):.3f} per segment")


if __name__ == "__main__":
    main()
