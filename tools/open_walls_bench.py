"""What open walls cost (fx_set_open_walls; csrc/fx_open.hip, the sweeps and the projection: csrc/fx_obstacle.hip): a table for docs/LAB.md, not a figure of bench.py.

    python tools/open_walls_bench.py [--grid 256] [--iters 40] [--steps 30] [--warmup 10] [--repeats 3] [--storage fp32] [--stage-reps 200] [--json out.json]

One process, four contexts on one grid, stepped in turn so that every leg sees the same device state; the times are the device events of
fx_timing.  Legs:
  A  all walls closed, no mask: the planner's solve (several sweeps per launch) -- the yardstick of the step
  B  Y+ open, no mask: k_jacobi_bnd_v4<CODE = 0, OPEN = 1>, no code bytes (12 bytes per cell and sweep)
  C  Y+ open, an all-fluid mask: k_jacobi_bnd_v4<1, 1> with code bytes (13)
  D  all walls closed, an all-fluid mask: k_jacobi_bnd_v4<1, 0> (13) -- the yardstick of the sweep
Every repeat prints one line per leg: us per sweep (jacobi_ms / jacobi_sweeps) and the step in ms.  Then the inflow stage alone:
fx_open_inflow --stage-reps times on leg B's context with one face open and with all six, us per launch, on the state the steps left.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fluidx12_amd as fx  # noqa: E402
from fluidx12_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--storage", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--stage-reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.grid
    fluid_mask = np.zeros((n, n, n), np.uint8)
    legs = [("A", 0, False), ("B", capi.WALL_Y_HI, False), ("C", capi.WALL_Y_HI, True), ("D", 0, True)]
    ctx = {}
    for name, faces, mask in legs:
        f = fx.Fluid()
        if not f.Init(0, 0, (n, n, n), jacobi_iters=a.iters, storage=a.storage):
            raise SystemExit("Init failed: %d" % f.last_status)
        if mask:
            f.SetObstacles(fluid_mask)
        f.SetOpenWalls(faces)
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
    print("leg rep  sweep_us  launches/step  advect_ms  step_ms   (grid %d^3 %s, %d sweeps, %d steps per leg and repeat)" % (n, a.storage, a.iters, a.steps))
    for rep in range(a.repeats):
        for name in ctx:                               # alternating: A B C D, A B C D, ...
            f = ctx[name]
            f.timing_enable(True)
            f.timing_read(True)
            run(name, a.steps)
            t = f.timing_read(True)
            f.timing_enable(False)
            steps = max(int(t.steps), 1)
            row = {"leg": name, "repeat": rep, "sweep_us": 1e3 * t.jacobi_ms / max(int(t.jacobi_sweeps), 1),
                   "launches_per_step": int(t.jacobi_launches) / steps, "advect_ms": t.advect_ms / steps,
                   "step_ms": (t.advect_ms + t.divergence_ms + t.jacobi_ms + t.project_ms) / steps}
            rows.append(row)
            print("%-3s %3d  %8.2f  %13.1f  %9.4f  %7.4f" % (name, rep, row["sweep_us"], row["launches_per_step"], row["advect_ms"], row["step_ms"]), flush=True)
    keys = ("sweep_us", "advect_ms", "step_ms")
    med = {k: {m: float(np.median([r[m] for r in rows if r["leg"] == k])) for m in keys} for k in ctx}
    spread = {k: {m: float(np.ptp([r[m] for r in rows if r["leg"] == k])) for m in keys} for k in ctx}
    print("median us per sweep: " + "  ".join("%s %.2f (spread %.2f)" % (k, med[k]["sweep_us"], spread[k]["sweep_us"]) for k in ctx))
    print("median step_ms:      " + "  ".join("%s %.4f (spread %.4f)" % (k, med[k]["step_ms"], spread[k]["step_ms"]) for k in ctx))
    print("open against the yardstick sweep (medians): B - D %.2f us   C - D %.2f us;   open step against the planner's: B - A %.4f ms"
          % (med["B"]["sweep_us"] - med["D"]["sweep_us"], med["C"]["sweep_us"] - med["D"]["sweep_us"], med["B"]["step_ms"] - med["A"]["step_ms"]))
    # the inflow stage alone, back to back on the state the steps left
    stage = {}
    f = ctx["B"]
    all_faces = capi.WALL_ALL
    for name, faces in (("one face (y+)", capi.WALL_Y_HI), ("all six", all_faces)):
        f.SetOpenWalls(faces)
        reps = []
        for _ in range(a.repeats):
            for _ in range(10):
                f.OpenInflow()
            f.Synchronize()
            f.timing_enable(True)
            f.timing_read(True)
            for _ in range(a.stage_reps):
                f.OpenInflow()
            f.Synchronize()
            t = f.timing_read(True)
            f.timing_enable(False)
            reps.append(1e3 * t.advect_ms / a.stage_reps)
        stage[name] = {"us_per_launch": float(np.median(reps)), "spread": float(np.ptp(reps))}
        print("k_open_inflow alone, %s: %.1f us per launch (spread %.1f)" % (name, stage[name]["us_per_launch"], stage[name]["spread"]))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"grid": n, "storage": a.storage, "iters": a.iters, "steps": a.steps, "rows": rows, "median": med, "spread": spread, "stage": stage},
                      fh, indent=1)
    for f in ctx.values():
        f.Release()


if __name__ == "__main__":
    main()
