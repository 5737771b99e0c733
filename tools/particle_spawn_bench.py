#!/usr/bin/env python3
"""What the particle spawners cost (docs/LAB.md section 33), on docs/LAB.md section 32's terms: 256^3, 40 sweeps, the default time step, the
built-in impulse, 160 steps to develop the plume the move is timed in.  Everything is timed through fx_timing.project_ms (HIP events around
the launches of the stage): three windows of 10 launches behind a warm-up, per row

  spawn    fx_spawn_particles alone: the count over the ages, the scan, the tick and the placement
  move     fx_move_particles on the same set with the spawners off, for scale

for pools of 2^20 and 2^22 records, half of them dead: uniform in [0,1)^3 with the dead slots scattered ("shuffled"), the same pool sorted by
the device, the dead in the tail ("sorted"), and the shuffled pool with a rate of 0 ("no_births": the count, the scan and the tick, and a
placement whose every workgroup leaves at once).  Two spawners, a box and a ball, bear `--births` records per launch between them; a window
takes a few per cent of the dead slots at the most, so the last launch of a row sees the pool the first one saw.

  python tools/particle_spawn_bench.py [--grid 256] [--steps 160] [--log2 20 22] [--births 4096] [--storage fp16] [--json FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidx12_amd as fx                                                     # noqa: E402

f32 = np.float32


def windows(f, launch, n=10, reps=3):
    """project_ms per launch of `launch`: `reps` windows of `n` launches behind a warm-up"""
    out = []
    for _ in range(reps):
        launch()
        f.Synchronize()
        f.timing_read(reset=True)
        for _ in range(n):
            launch()
        f.Synchronize()
        out.append(f.timing_read(reset=True).project_ms / n)
    return out


def spawners(births, dt):
    rate = births / 2.0 / dt
    return [dict(shape="box", seed=1, center=(0.5, 0.2, 0.5), half_extent=(0.2, 0.05, 0.2), rate=rate, age_spread=1.0),
            dict(shape="ball", seed=2, center=(0.5, 0.5, 0.5), half_extent=(0.25, 0.25, 0.25), rate=rate, age_spread=1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--births", type=int, default=4096)
    ap.add_argument("--storage", nargs="+", default=["fp16"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    G = args.grid
    med = lambda v: float(np.median(v))
    rows = []
    for storage in args.storage:
        f = fx.Fluid()
        assert f.Init(0, 0, (G, G, G), storage=storage, jacobi_iters=40)
        dt = f.default_time_step()
        for i in range(args.steps):
            f.UpdateFrame(dt, i % 3)
            f.Simulate(i % 3)
        f.Synchronize()
        f.UpdateFrame(dt, 0)
        rng = np.random.default_rng(33)
        f.SetParticleSort(True)
        f.timing_enable(True)
        for lg in args.log2:
            n = 1 << lg
            rec = np.zeros((n, 4), f32)
            rec[:, :3] = rng.random((n, 3), dtype=f32)
            rec[rng.permutation(n)[:n // 2], 3] = -1.0
            for name in ("shuffled", "sorted", "no_births"):
                f.SetParticleSpawners(None)
                f.SetParticles(rec)
                if name == "sorted":
                    f.SortParticles()
                row = {"storage": storage, "pool": n, "dead": n // 2, "arrangement": name}
                row["move_ms"] = windows(f, f.MoveParticles)
                f.SetParticles(rec)
                if name == "sorted":
                    f.SortParticles()
                f.SetParticleSpawners(spawners(0 if name == "no_births" else args.births, dt))
                row["spawn_ms"] = windows(f, f.SpawnParticles)
                info = f.ParticleSpawnInfo()
                row["born"], row["dropped"] = info["born"], info["dropped"]
                row["spawn_over_move"] = med(row["spawn_ms"]) / med(row["move_ms"])
                row["GBps_of_16B_per_record"] = 16.0 * n / med(row["spawn_ms"]) / 1e6
                rows.append(row)
                print(json.dumps(row), flush=True)
        f.Release()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
