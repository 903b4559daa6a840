#!/usr/bin/env python3
"""Speed of the light-biased integrators: Rust2's light test scene (tests/golden/rust2_light_scene.json) at the reference's 400 x 300 x 100,
depth 9, RTW_INTEGRATOR_LIGHT_BIASED against RTW_INTEGRATOR_RUST2 -- ms per frame and G segments/s (shadow queries counted) --, and the
scheduler census of the tree kernel on that scene with a field of 60 spheres added.

    python scripts/measure_lights.py [repeats]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtw_amd as R                      # noqa: E402
from tests import lights_common as LC    # noqa: E402


def run(gpu, cam, p, reps):
    gpu.render(cam, p)
    ms, st = [], None
    for _ in range(reps):
        _, st = gpu.render(cam, p)
        ms.append(st.kernel_ms)
    return float(np.median(ms)), min(ms), max(ms), st


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ls, g = LC.golden()
    sp = LC.sphere_field(g)
    field = LC.LightScene(sp, g["quads"], ls.lights, g["background"], weight=g["biased_weight"])
    w, h = g["width"], g["height"]
    cam = LC.camera(g, w, h)
    with R.Renderer(0) as gpu:
        for name, scene in (("golden scene (1 sphere + 6 quads: the list walk)", ls), ("golden scene + 60 spheres (the tree)", field)):
            gpu.set_scene(scene.scene)
            gpu.set_lights(scene.lights, scene.weight)
            print(name)
            for integ, label in ((R.INTEGRATOR_RUST2, "RUST2"), (R.INTEGRATOR_LIGHT_BIASED, "LIGHT_BIASED"), (R.INTEGRATOR_LIGHT_CAST, "LIGHT_CAST")):
                p = scene.params(w, h, integ, g["depth_light_biased"], seed=1, sampler=R.SAMPLER_CENTRES, samples=g["samples"], gamma=g["gamma"],
                                 mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
                med, lo, hi, st = run(gpu, cam, p, reps)
                line = (f"  {label:13s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} runs)  {st.segments} segments  "
                        f"{st.segments / med / 1e6:7.3f} G segments/s  kernel: {'render_bvh' if st.node_tests else 'render_brute'}")
                print(line)
                if st.node_tests:
                    for k, ph in enumerate(("traverse", "leaf", "shade")):
                        steps, lanes = st.phase_steps[k], st.phase_lanes[k]
                        print(f"      {ph:9s} {steps:12d} wave steps, {lanes:14d} lanes, SIMD efficiency {lanes / (64.0 * max(steps, 1)):.3f}")


if __name__ == "__main__":
    main()
