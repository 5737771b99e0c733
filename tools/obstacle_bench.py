"""What the obstacle-aware pressure solve costs (fx_set_obstacles, csrc/fx_obstacle.hip): a table for docs/LAB.md, not a figure of bench.py.

    python tools/obstacle_bench.py [--grid 256] [--iters 40] [--steps 50] [--warmup 10] [--repeats 3] [--json out.json]

One process, four contexts on one grid (fp32 storage, fixed sweep count), stepped in turn so that every leg sees the same device state; the
times are the device events of fx_timing.  Legs:
  A  no mask, FX_FLAG_JACOBI_FUSE = 1: one k_jacobi_v4 sweep per launch -- the yardstick of the obstacle sweep (12 bytes per cell and sweep)
  B  an all-fluid mask: k_jacobi_bnd_v4<CODE = 1, OPEN = 0> (13 bytes per cell and sweep), k_divergence_obs, k_project_bnd<HALF, 1, 0>
  C  a ball of radius 0.15 at (0.5, 0.45, 0.5): the same kernels, and the enforce launch over the ball's bounding box
  D  no mask, default plan: what a context without obstacles runs (several sweeps per launch)
Every repeat prints one line per leg: us per sweep, and divergence / projection / advection (with the enforce pass) / step in ms.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fluidx12_amd as fx  # noqa: E402


def ball(n, center=(0.5, 0.45, 0.5), radius=0.15):
    c = (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return ((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2 <= radius * radius).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.grid
    legs = [("A", dict(jacobi_fuse=1), None), ("B", {}, np.zeros((n, n, n), np.uint8)), ("C", {}, ball(n)), ("D", {}, None)]
    ctx = {}
    for name, kw, mask in legs:
        f = fx.Fluid()
        if not f.Init(0, 0, (n, n, n), jacobi_iters=a.iters, **kw):
            raise SystemExit("Init failed: %d" % f.last_status)
        if mask is not None:
            f.SetObstacles(mask)
        ctx[name] = f
    dt = np.float32(ctx["A"].default_time_step())
    frame = {k: 0 for k in ctx}

    def run(name, count):
        f = ctx[name]
        for _ in range(count):
            f.UpdateFrame(dt, frame[name] % 3)
            f.Simulate(frame[name] % 3)
            frame[name] += 1
        f.Synchronize()

    for name in ctx:                                   # warm-up: every leg the same number of steps, so the plumes are of one age
        run(name, a.warmup)
    rows = []
    print("leg rep  us/sweep  sweeps/launch  divergence_ms  project_ms  advect_ms  step_ms   (grid %d^3, %d sweeps, %d steps per leg and repeat)" % (n, a.iters, a.steps))
    for rep in range(a.repeats):
        for name in ctx:                               # alternating: A B C D, A B C D, ...
            f = ctx[name]
            f.timing_enable(True)
            f.timing_read(True)
            run(name, a.steps)
            t = f.timing_read(True)
            f.timing_enable(False)
            steps = max(int(t.steps), 1)
            row = {"leg": name, "repeat": rep, "us_per_sweep": 1e3 * t.jacobi_ms / max(int(t.jacobi_sweeps), 1),
                   "sweeps_per_launch": t.jacobi_sweeps / max(int(t.jacobi_launches), 1), "divergence_ms": t.divergence_ms / steps,
                   "project_ms": t.project_ms / steps, "advect_ms": t.advect_ms / steps,
                   "step_ms": (t.advect_ms + t.divergence_ms + t.jacobi_ms + t.project_ms) / steps, "solid_cells": f.GetObstacles()[1]}
            rows.append(row)
            print("%-3s %3d  %8.2f  %13.2f  %13.4f  %10.4f  %9.4f  %7.4f" % (name, rep, row["us_per_sweep"], row["sweeps_per_launch"], row["divergence_ms"],
                                                                        row["project_ms"], row["advect_ms"], row["step_ms"]), flush=True)
    # the enforce pass alone: leg C's advection against leg B's
    adv = {k: np.median([r["advect_ms"] for r in rows if r["leg"] == k]) for k in ctx}
    sw = {k: np.median([r["us_per_sweep"] for r in rows if r["leg"] == k]) for k in ctx}
    print("median us/sweep: " + "  ".join("%s %.2f" % (k, sw[k]) for k in ctx) + "   B/A %.3f  C/A %.3f  (bytes 13/12 = %.3f)" % (sw["B"] / sw["A"], sw["C"] / sw["A"], 13 / 12))
    print("enforce (C - B advect_ms, medians): %.4f ms over %d solid cells" % (adv["C"] - adv["B"], ctx["C"].GetObstacles()[1]))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"grid": n, "iters": a.iters, "steps": a.steps, "rows": rows}, fh, indent=1)
    for f in ctx.values():
        f.Release()


if __name__ == "__main__":
    main()
