#!/usr/bin/env python3
"""Cost of the MixedMaterial branch: Rust2's mixed_material_test scene (tests/golden/rust2_mixed_scene.json) at the reference's
400 x 300 x 100, depth 9 (LIGHT_CAST: 10), under the three Rust2 integrators with RTW_FLAG_MIXED_MATERIAL (the mixed build), and the same
scene with the flag off (both walls Lambertian: the existing light build / RUST2 build) -- ms per frame (render kernel and resolve, median),
segments and G segments/s --, then the scheduler census of the tree kernel with a field of 60 spheres added.

    python scripts/measure_mixed.py [repeats]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtw_amd as R                      # noqa: E402
from tests import lights_common as LC    # noqa: E402
from tests import mixed_common as MC     # noqa: E402


def run(gpu, cam, p, reps):
    gpu.render(cam, p)
    ms, st = [], None
    for _ in range(reps):
        _, st = gpu.render(cam, p)
        ms.append(st.kernel_ms)
    return float(np.median(ms)), min(ms), max(ms), st


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ms0, g = MC.golden()
    field = MC.MixedScene(LC.sphere_field(g), g["quads"], ms0.lights, g["background"], weight=g["biased_weight"])
    w, h = g["width"], g["height"]
    cam = LC.camera(g, w, h)
    with R.Renderer(0) as gpu:
        for name, scene in (("mixed golden scene (1 sphere + 6 quads: the list walk)", ms0), ("mixed golden scene + 60 spheres (the tree)", field)):
            gpu.set_scene(scene.scene)
            gpu.set_lights(scene.lights, scene.weight)
            print(name)
            for integ, label, depth in ((R.INTEGRATOR_RUST2, "RUST2", g["depth_light_biased"]), (R.INTEGRATOR_LIGHT_BIASED, "LIGHT_BIASED", g["depth_light_biased"]),
                                        (R.INTEGRATOR_LIGHT_CAST, "LIGHT_CAST", g["depth_light_cast"])):
                for flags, what in ((R.FLAG_MIXED_MATERIAL, "flag on "), (0, "flag off")):
                    p = scene.params(w, h, integ, depth, seed=1, sampler=R.SAMPLER_CENTRES, samples=g["samples"], gamma=g["gamma"],
                                     mint=g["mint"], maxt=g["maxt"], accel=R.ACCEL_BVH)
                    p.flags = flags
                    med, lo, hi, st = run(gpu, cam, p, reps)
                    print(f"  {label:13s} {what} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} runs)  {st.segments} segments  "
                          f"{st.segments / med / 1e6:7.3f} G segments/s  kernel: {'render_bvh' if st.node_tests else 'render_brute'}")
                    if st.node_tests:
                        for k, ph in enumerate(("traverse", "leaf", "shade")):
                            steps, lanes = st.phase_steps[k], st.phase_lanes[k]
                            print(f"      {ph:9s} {steps:12d} wave steps, {lanes:14d} lanes, SIMD efficiency {lanes / (64.0 * max(steps, 1)):.3f}")


if __name__ == "__main__":
    main()
