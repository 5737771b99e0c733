"""What MacCormack advection costs (fx_set_advection_scheme, csrc/fx_maccormack.hip: k_mc_predict, k_mc_correct): a table for docs/LAB.md, not a
figure of bench.py.

    python tools/maccormack_bench.py [--grid 256] [--iters 40] [--steps 50] [--warmup 10] [--repeats 3] [--storage fp32] [--stage-reps 200] [--stage-only] [--json out.json]

One process, two contexts on one grid, stepped in turn so that both legs see the same device state; the times are the device events of fx_timing.
  A  the scheme never set: the default path, and the yardstick of the step
  B  FX_ADVECT_MACCORMACK
Every repeat prints one line per leg: advection and step in ms.  Then the stage alone: fx_advect --stage-reps times on each context, us per call,
on the state the steps left -- for leg B that is the predictor plus the corrector, held against their compulsory traffic at --floor-tbs TB/s
(fp32 storage: the predictor reads 28 bytes per cell and writes 28, the corrector reads 28 + 28 and writes 28; fp16 storage: 14 + 28, and
14 + 28 + 14; the render's alpha side volume, 4 more, is not written by a context that does not render).  The events time a call, not a
kernel: the split between the two launches comes from a kernel trace of `--stage-only` (the stage loops alone, no steps timed).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fluidx12_amd as fx  # noqa: E402
from fluidx12_amd import capi  # noqa: E402


def floor_bytes(storage):
    """(predictor, corrector) compulsory bytes per cell"""
    q = 28 if storage == "fp32" else 14
    return q + 28, q + 28 + q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--storage", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--stage-reps", type=int, default=200)
    ap.add_argument("--stage-only", action="store_true")
    ap.add_argument("--floor-tbs", type=float, default=6.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.grid
    ctx = {}
    for name, scheme in (("A", None), ("B", capi.ADVECT_MACCORMACK)):
        f = fx.Fluid()
        if not f.Init(0, 0, (n, n, n), jacobi_iters=a.iters, storage=a.storage):
            raise SystemExit("Init failed: %d" % f.last_status)
        if scheme is not None:
            f.SetAdvectionScheme(scheme)
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

    for name in ctx:                                   # warm-up: both legs the same number of steps, so the plumes are of one age
        run(name, a.warmup)
    rows, med, spread = [], {}, {}
    if not a.stage_only:
        print("leg rep  advect_ms  step_ms   (grid %d^3 %s, %d sweeps, %d steps per leg and repeat)" % (n, a.storage, a.iters, a.steps))
        for rep in range(a.repeats):
            for name in (("A", "B") if rep % 2 == 0 else ("B", "A")):      # alternating, each first in turn
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
        print("the scheme inside the step (medians): advect_ms B / A %.4f / %.4f = %.2f x   step_ms B - A %.4f ms"
              % (med["B"]["advect_ms"], med["A"]["advect_ms"], med["B"]["advect_ms"] / med["A"]["advect_ms"], med["B"]["step_ms"] - med["A"]["step_ms"]))
    # the stage alone, back to back on the state the steps left
    stage = {}
    for name in ctx:
        f = ctx[name]
        f.UpdateFrame(dt, 0)
        for _ in range(10):
            f.Advect()
        f.Synchronize()
        f.timing_enable(True)
        f.timing_read(True)
        for _ in range(a.stage_reps):
            f.Advect()
        f.Synchronize()
        t = f.timing_read(True)
        f.timing_enable(False)
        stage[name] = {"us_per_call": 1e3 * t.advect_ms / a.stage_reps}
    bp, bc = floor_bytes(a.storage)
    cells = float(n) ** 3
    floor_us = (bp + bc) * cells / (a.floor_tbs * 1e12) * 1e6
    us = stage["B"]["us_per_call"]
    stage["B"].update({"bytes_per_cell": [bp, bc], "tb_per_s": (bp + bc) * cells / (us * 1e-6) / 1e12, "floor_us": floor_us})
    print("fx_advect alone: semi-Lagrangian %.1f us per call; MacCormack (k_mc_predict + k_mc_correct) %.1f us = %.2f x, %.2f TB/s of their %d + %d "
          "compulsory bytes per cell (floor at %.1f TB/s: %.1f us, reached %.0f %%)"
          % (stage["A"]["us_per_call"], us, us / stage["A"]["us_per_call"], stage["B"]["tb_per_s"], bp, bc, a.floor_tbs, floor_us, 100.0 * floor_us / us))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"grid": n, "storage": a.storage, "iters": a.iters, "steps": a.steps, "rows": rows, "median": med, "spread": spread, "stage": stage},
                      fh, indent=1)
    for f in ctx.values():
        f.Release()


if __name__ == "__main__":
    main()
