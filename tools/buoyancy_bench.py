"""What the buoyancy pass costs (fx_set_buoyancy, csrc/fx_heat.hip: k_heat): a table for docs/LAB.md, not a figure of bench.py.

    python tools/buoyancy_bench.py [--grid 256] [--iters 40] [--steps 50] [--warmup 10] [--repeats 3] [--storage fp32] [--stage-reps 200] [--json out.json]

One process, three contexts on one grid, stepped in turn so that every leg sees the same device state; the times are the device events of
fx_timing.  Legs:
  A  buoyancy off: what a context that never calls fx_set_buoyancy runs -- the default path, and the yardstick of the step
  B  buoyancy on, default `up` (the force touches one velocity plane), one heat source at the built-in ball's place
  C  the same with up = (0.3, 1, -0.2): all three velocity planes are read and written
Every repeat prints one line per leg: advection (with the pass) and step in ms.  Then the stage alone: fx_heat --stage-reps times on leg B's
and leg C's context, us per launch, and that time against the pass's compulsory traffic at --floor-tbs TB/s (fp32 storage, default up:
T in + out 8, u0 12, the colour texel 16, u_y read + write 8 = 44 bytes per cell; fp16 storage halves all but the temperature: 26).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fluidx12_amd as fx  # noqa: E402


def floor_bytes(storage, planes):
    es = 4 if storage == "fp32" else 2
    return 8 + 3 * es + 4 * es + 2 * es * planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--storage", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--stage-reps", type=int, default=200)
    ap.add_argument("--floor-tbs", type=float, default=6.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.grid
    source = [dict(center=(0.5, 0.1, 0.5), radius=1.0 / 16, rate=40.0)]
    legs = [("A", None), ("B", (0.0, 1.0, 0.0)), ("C", (0.3, 1.0, -0.2))]
    ctx = {}
    for name, up in legs:
        f = fx.Fluid()
        if not f.Init(0, 0, (n, n, n), jacobi_iters=a.iters, storage=a.storage):
            raise SystemExit("Init failed: %d" % f.last_status)
        if up is not None:
            f.SetBuoyancy(ambient=0.0, density_weight=0.5, lift=2.0, cooling=0.2, up=up)
            f.SetHeatSources(source)
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
    print("leg rep  advect_ms  step_ms   (grid %d^3 %s, %d sweeps, %d steps per leg and repeat)" % (n, a.storage, a.iters, a.steps))
    for rep in range(a.repeats):
        for name in ctx:                               # alternating: A B C, A B C, ...
            f = ctx[name]
            f.timing_enable(True)
            f.timing_read(True)
            run(name, a.steps)
            t = f.timing_read(True)
            f.timing_enable(False)
            steps = max(int(t.steps), 1)
            row = {"leg": name, "repeat": rep, "advect_ms": t.advect_ms / steps,
                   "step_ms": (t.advect_ms + t.divergence_ms + t.jacobi_ms + t.project_ms) / steps}
            rows.append(row)
            print("%-3s %3d  %9.4f  %7.4f" % (name, rep, row["advect_ms"], row["step_ms"]), flush=True)
    med = {k: {m: float(np.median([r[m] for r in rows if r["leg"] == k])) for m in ("advect_ms", "step_ms")} for k in ctx}
    spread = {k: float(np.ptp([r["step_ms"] for r in rows if r["leg"] == k])) for k in ctx}
    print("median step_ms: " + "  ".join("%s %.4f (spread %.4f)" % (k, med[k]["step_ms"], spread[k]) for k in ctx))
    print("the pass inside the step (advect_ms, medians): B - A %.4f ms   C - A %.4f ms" % (med["B"]["advect_ms"] - med["A"]["advect_ms"],
                                                                                         med["C"]["advect_ms"] - med["A"]["advect_ms"]))
    # the stage alone, back to back on the state the steps left
    stage = {}
    for name, planes in (("B", 1), ("C", 3)):
        f = ctx[name]
        for _ in range(10):
            f.Heat()
        f.Synchronize()
        f.timing_enable(True)
        f.timing_read(True)
        for _ in range(a.stage_reps):
            f.Heat()
        f.Synchronize()
        t = f.timing_read(True)
        f.timing_enable(False)
        us = 1e3 * t.advect_ms / a.stage_reps
        b = floor_bytes(a.storage, planes)
        floor_us = b * float(n) ** 3 / (a.floor_tbs * 1e12) * 1e6
        stage[name] = {"us_per_launch": us, "bytes_per_cell": b, "tb_per_s": b * float(n) ** 3 / (us * 1e-6) / 1e12, "floor_us": floor_us}
        print("k_heat alone, leg %s: %.1f us per launch = %.2f TB/s of its %d compulsory bytes per cell (floor at %.1f TB/s: %.1f us, reached %.0f %%)"
              % (name, us, stage[name]["tb_per_s"], b, a.floor_tbs, floor_us, 100.0 * floor_us / us))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"grid": n, "storage": a.storage, "iters": a.iters, "steps": a.steps, "rows": rows, "median": med, "spread": spread, "stage": stage},
                      fh, indent=1)
    for f in ctx.values():
        f.Release()


if __name__ == "__main__":
    main()
