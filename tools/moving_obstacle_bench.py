"""What moving obstacles cost (fx_set_obstacle_bodies; csrc/fx_obstacle.hip): a table for docs/LAB.md, not a figure of bench.py.

    python tools/moving_obstacle_bench.py [--grid 256] [--iters 40] [--steps 100] [--warmup 20] [--repeats 3] [--storage fp32] [--resting-only] [--json out.json]

One process, two contexts on one grid with the ball of tests/test_obstacle_ref.py `ball_mask` (centre (0.5, 0.45, 0.5), radius 0.22) as the
mask, stepped in turn so that both legs see the same device state; the times are the device events of fx_timing.  Legs:
  R  the ball at rest (no bodies): k_obstacle_enforce, k_divergence_obs, k_project_bnd with MOV = 0 -- the launches of a library without the call
  M  one translating body whose box encloses the ball: the same three with MOV = 1; the sweeps are the same k_jacobi_bnd_v4 launches
Every repeat prints one line per leg: the step in ms and its split (advect_ms holds the enforce pass).  --resting-only runs leg R alone and
also takes a library that predates the call (FLUIDX_LIB_PATH=...): the resting figure of an older build, for the comparison across commits.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fluidx12_amd import capi  # noqa: E402


def ball(n, center=(0.5, 0.45, 0.5), radius=0.22):
    c = (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return ((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2 <= radius * radius).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--storage", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--resting-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.resting_only:                                 # (a library from before the call lacks the two symbols; leg R never asks for them)
        for name in ("fx_set_obstacle_bodies", "fx_get_obstacle_bodies"):
            capi.SYMBOLS.pop(name, None)
    import fluidx12_amd as fx
    n = a.grid
    mask = ball(n)
    body = {"box_lo": (0.27, 0.22, 0.27), "box_hi": (0.73, 0.68, 0.73), "linear": (0.25, 0.0, 0.0)}
    legs = [("R", None)] + ([] if a.resting_only else [("M", [body])])
    ctx = {}
    for name, bodies in legs:
        f = fx.Fluid()
        if not f.Init(0, 0, (n, n, n), jacobi_iters=a.iters, storage=a.storage):
            raise SystemExit("Init failed: %d" % f.last_status)
        f.SetObstacles(mask)
        if bodies:
            f.SetObstacleBodies(bodies)
        ctx[name] = f
    dt = np.float32(ctx["R"].default_time_step())
    frame = {k: 0 for k in ctx}

    def run(name, count):
        f = ctx[name]
        for _ in range(count):
            f.UpdateFrame(dt, frame[name] % 3)
            f.Simulate(frame[name] % 3)
            frame[name] += 1
        f.Synchronize()

    for name in ctx:
        run(name, a.warmup)
    rows = []
    keys = ("advect_ms", "divergence_ms", "jacobi_ms", "project_ms", "step_ms")
    print("leg rep  advect_ms  divergence_ms  jacobi_ms  project_ms  step_ms  launches/step   (%s, grid %d^3 %s, %d sweeps, %d steps per leg and repeat)"
          % (os.environ.get("FLUIDX_LIB_PATH", "the tree's library"), n, a.storage, a.iters, a.steps))
    for rep in range(a.repeats):
        for name in ctx:                               # alternating: R M, R M, ...
            f = ctx[name]
            f.timing_enable(True)
            f.timing_read(True)
            run(name, a.steps)
            t = f.timing_read(True)
            f.timing_enable(False)
            steps = max(int(t.steps), 1)
            row = {"leg": name, "repeat": rep, "advect_ms": t.advect_ms / steps, "divergence_ms": t.divergence_ms / steps, "jacobi_ms": t.jacobi_ms / steps,
                   "project_ms": t.project_ms / steps, "launches_per_step": int(t.jacobi_launches) / steps}
            row["step_ms"] = row["advect_ms"] + row["divergence_ms"] + row["jacobi_ms"] + row["project_ms"]
            rows.append(row)
            print("%-3s %3d  %9.4f  %13.4f  %9.4f  %10.4f  %7.4f  %13.1f" % ((name, rep) + tuple(row[k] for k in keys) + (row["launches_per_step"],)), flush=True)
    med = {k: {m: float(np.median([r[m] for r in rows if r["leg"] == k])) for m in keys} for k in ctx}
    spread = {k: {m: float(np.ptp([r[m] for r in rows if r["leg"] == k])) for m in keys} for k in ctx}
    for k in ctx:
        print("%s median (spread) ms: " % k + "  ".join("%s %.4f (%.4f)" % (m[:-3], med[k][m], spread[k][m]) for m in keys))
    if "M" in ctx:
        print("moving - resting (medians), ms: " + "  ".join("%s %+.4f" % (m[:-3], med["M"][m] - med["R"][m]) for m in keys))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"grid": n, "storage": a.storage, "iters": a.iters, "steps": a.steps, "library": os.environ.get("FLUIDX_LIB_PATH"), "rows": rows,
                       "median": med, "spread": spread}, fh, indent=1)
    for f in ctx.values():
        f.Release()


if __name__ == "__main__":
    main()
