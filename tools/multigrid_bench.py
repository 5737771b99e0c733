"""What the multigrid pressure solve costs and buys (fx_set_pressure_solver, csrc/fx_multigrid.hip): a table for docs/LAB.md, not a figure of
bench.py.

    python tools/multigrid_bench.py [--grid 256] [--iters 40] [--develop 160] [--steps 50] [--repeats 3] [--solve-only] [--json out.json]

One process, three contexts on one grid, fp32.  All three are stepped --develop steps with the default Jacobi solve first, so that they hold the
same developed plume; then each leg gets its solver and the legs are stepped in turn; the times are the device events of fx_timing.
  A  the solver never set: --iters Jacobi sweeps, the yardstick
  B  FX_PRESSURE_MULTIGRID with the Python mirror's defaults (2 V(2,2) cycles, 16 coarse sweeps)
  C  the same with FX_MG_NO_TAIL: every level as launches of its own
Every repeat prints one line per leg: jacobi_ms and the step in ms, and the launches per solve.  Then what each solver leaves: from the
developed state of leg A (velocity behind the advection, the warm-start pressure), fx_divergence and one fx_pressure_solve on every leg, and the
rms of the mean-removed residual (float64 on the host) as a share of the warm start's.
--solve-only: only that last part, 20 solves per leg -- the run to put under a kernel trace (rocprofv3 --kernel-trace --stats, on its own) for
the per-kernel times.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fluidx12_amd as fx  # noqa: E402
from fluidx12_amd import capi  # noqa: E402

LEGS = (("A", None), ("B", 0), ("C", capi.MG_NO_TAIL))


def rms_residual(p, b):
    """rms of the mean-removed residual b - (sum(q) - 6 p), clamped neighbours, float64"""
    p = p.astype(np.float64)
    s = np.zeros_like(p)
    for axis in range(3):
        n = p.shape[axis]
        if n > 1:
            s += np.take(p, np.clip(np.arange(n) - 1, 0, n - 1), axis=axis) + np.take(p, np.clip(np.arange(n) + 1, 0, n - 1), axis=axis)
    r = 6.0 * p + b - s
    r -= r.mean()
    return float(np.sqrt((r * r).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--develop", type=int, default=160)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--solve-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.grid
    ctx = {}
    for name, _ in LEGS:
        f = fx.Fluid()
        if not f.Init(0, 0, (n, n, n), jacobi_iters=a.iters):
            raise SystemExit("Init failed: %d" % f.last_status)
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

    for name in ctx:                                   # the developed plume, the same on every leg
        run(name, a.develop)
    for name, flags in LEGS:
        if flags is not None:
            ctx[name].SetPressureSolver("multigrid", flags=flags)
    levels = ctx["B"].GetPressureSolver()["max_levels"]
    rows, med, spread = [], {}, {}
    if not a.solve_only:
        print("leg rep  jacobi_ms  step_ms  launches/solve   (grid %d^3 fp32, A: %d sweeps, B / C: %d levels, %d steps per leg and repeat)" % (n, a.iters, levels, a.steps))
        for rep in range(a.repeats):
            order = [k for k, _ in LEGS]
            order = order[rep % 3:] + order[:rep % 3]  # each leg first in turn
            for name in order:
                f = ctx[name]
                f.timing_enable(True)
                f.timing_read(True)
                run(name, a.steps)
                t = f.timing_read(True)
                f.timing_enable(False)
                steps = max(int(t.steps), 1)
                row = {"leg": name, "repeat": rep, "jacobi_ms": t.jacobi_ms / steps, "launches": t.jacobi_launches / steps,
                       "step_ms": (t.advect_ms + t.divergence_ms + t.jacobi_ms + t.project_ms) / steps}
                rows.append(row)
                print("%-3s %3d  %9.4f  %7.4f  %8.1f" % (name, rep, row["jacobi_ms"], row["step_ms"], row["launches"]), flush=True)
        med = {k: {m: float(np.median([r[m] for r in rows if r["leg"] == k])) for m in ("jacobi_ms", "step_ms")} for k in ctx}
        spread = {k: float(np.ptp([r["jacobi_ms"] for r in rows if r["leg"] == k])) for k in ctx}
        print("median jacobi_ms: " + "  ".join("%s %.4f (spread %.4f)" % (k, med[k]["jacobi_ms"], spread[k]) for k in ctx))
    # what each solver leaves, from one state: leg A's
    src = ctx["A"]
    src.UpdateFrame(dt, frame["A"] % 3)
    src.Advect()
    src.Synchronize()
    vel1, p0 = src.download(fx.FIELD_VELOCITY1), src.download(fx.FIELD_PRESSURE)
    left = {}
    for name in ctx:
        f = ctx[name]
        f.UpdateFrame(dt, 0)
        f.upload(fx.FIELD_VELOCITY1, vel1)
        f.Divergence()
        for _ in range(20 if a.solve_only else 1):
            f.upload(fx.FIELD_PRESSURE, p0)
            f.PressureSolve()
        f.Synchronize()
        b = f.download(fx.FIELD_DIVERGENCE).astype(np.float64)
        r0 = rms_residual(p0, b)
        left[name] = {"start": r0, "share_left": rms_residual(f.download(fx.FIELD_PRESSURE), b) / r0}
    print("residual left of the warm start's (rms, mean removed): " + "  ".join("%s %.4f" % (k, left[k]["share_left"]) for k in ctx))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"grid": n, "iters": a.iters, "levels": levels, "steps": a.steps, "rows": rows, "median": med, "spread": spread, "left": left}, fh, indent=1)
    for f in ctx.values():
        f.Release()


if __name__ == "__main__":
    main()
