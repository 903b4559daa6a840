"""Host-side cost of a render, A/B between two builds of librtw_hip.so with the same ABI (RTW_HIP_LIB selects the build, as in gpu_ab_libs.sh).

usage: python scripts/host_cost_ab.py PARENT_LIB.so [ROUNDS]        (the other side is the library in the tree)

Alternates the two builds, a fresh process each time, ROUNDS (default 5) times:
  (a) C1 at 400 x 225 x 10 on one context: 3 warm-up renders, then 5 whose RtwStats.enqueue_ms / total_ms are printed;
  (b) bench.py --gpus 1 --steps 5 --warmup 1: its ms_per_step.
Prints every raw value, the medians, and the parent's own max - min per figure.  Stops at the first child that fails."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the first rtw call: one HIP runtime in the process)
    import numpy as np
    import rtw_amd as R
    scene = R.Scene.generate(R.SCENE_C1)
    cam, p = R.default_view(R.SCENE_C1)
    out = np.empty((p.height, p.width, 3), np.float32)
    rows = []
    with R.Renderer(0) as r:
        r.set_scene(scene)
        for k in range(8):
            st = r.render(cam, p, out=out)[1]
            if k >= 3:
                rows.append((round(st.enqueue_ms, 4), round(st.total_ms, 4)))
    print(json.dumps(rows))


def run(cmd, lib, limit):
    env = dict(os.environ)
    env.pop("RTW_HIP_LIB", None)
    if lib:
        env["RTW_HIP_LIB"] = lib
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        print(f"FAILED ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
        sys.exit(r.returncode if r.returncode > 0 else 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    parent = os.path.abspath(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    figures = {side: {"enqueue_ms": [], "total_ms": [], "bench_ms_per_step": []} for side in ("parent", "result")}
    for k in range(rounds):
        for side, lib in (("parent", parent), ("result", None)):
            rows = run([sys.executable, os.path.abspath(__file__), "--child"], lib, 120)
            step = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], lib, 300)["ms_per_step"]
            figures[side]["enqueue_ms"] += [a for a, _ in rows]
            figures[side]["total_ms"] += [b for _, b in rows]
            figures[side]["bench_ms_per_step"].append(step)
            print(f"round {k} {side}: C1 400x225x10 (enqueue_ms, total_ms) {rows}  bench ms_per_step {step}", flush=True)
    for name in ("enqueue_ms", "total_ms", "bench_ms_per_step"):
        a, b = figures["parent"][name], figures["result"][name]
        ma, mb = statistics.median(a), statistics.median(b)
        print(f"{name}: median parent {ma:.4f} result {mb:.4f} (result - parent {mb - ma:+.4f}); parent max - min {max(a) - min(a):.4f}; "
              f"{'within' if mb - ma <= max(a) - min(a) else 'OUTSIDE'} the parent's spread", flush=True)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
