#!/usr/bin/env python3
"""What the particle sort costs and what it buys (docs/LAB.md section 31), on docs/LAB.md section 30's terms: 256^3 fp16, 40 sweeps, the default
time step, the built-in impulse, 160 steps to develop the plume; midpoint scheme, no drift, immortal particles.  Everything is timed through
fx_timing.project_ms (HIP events around the launches of the particle stage): three windows of 10 launches behind a warm-up, per row

  a  fx_move_particles on the unsorted set
  b  fx_sort_particles on the unsorted set (a fresh fx_set_particles in front of every launch: a sort leaves a sorted set behind)
  c  fx_move_particles on the set the device sorted
  d  fx_sort_particles on that sorted set (the steady state)

for 2^20 and 2^22 particles, positions uniform in [0,1)^3 ("random") and drawn cell by cell with probability proportional to alpha where
alpha > 0.01 ("plume").  Also checks, once per row, that the device's order is numpy's stable argsort of the keys.

  python tools/particle_sort_bench.py [--grid 256] [--steps 160] [--log2 20 22] [--json FILE]
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


def keys(rec, G):
    c = [np.minimum((np.clip(rec[:, a], 0, 1) * f32(G)).astype(f32).astype(np.int64), G - 1) for a in range(3)]
    return (c[2] * G + c[1]) * G + c[0]


def windows(f, prepare, launch, fresh_each=False, n=10, reps=3):
    """ms per launch of `launch`, `reps` windows of `n` launches; prepare() in front of every window (and of every launch if fresh_each)"""
    out = []
    for _ in range(reps):
        prepare()
        launch()                                                              # warm-up
        f.Synchronize()
        if not fresh_each:
            f.timing_read(reset=True)
            for _ in range(n):
                launch()
            f.Synchronize()
            out.append(f.timing_read(reset=True).project_ms / n)
        else:
            total = 0.0
            for _ in range(n):
                prepare()
                f.timing_read(reset=True)
                launch()
                f.Synchronize()
                total += f.timing_read(reset=True).project_ms
            out.append(total / n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    G = args.grid
    f = fx.Fluid()
    assert f.Init(0, 0, (G, G, G), storage="fp16", jacobi_iters=40)
    dt = f.default_time_step()
    for i in range(args.steps):
        f.UpdateFrame(dt, i % 3)
        f.Simulate(i % 3)
    f.Synchronize()
    alpha = f.download(fx.FIELD_COLOR)[..., 3].astype(np.float64).ravel()
    alpha[alpha <= 0.01] = 0.0
    rng = np.random.default_rng(31)
    f.SetParticleParams("midpoint")
    f.SetParticleSort(True)
    f.timing_enable(True)
    rows = []
    for lg in args.log2:
        n = 1 << lg
        sets = {"random": rng.random((n, 3))}
        cell = rng.choice(alpha.size, size=n, p=alpha / alpha.sum())
        ijk = np.stack([cell % G, (cell // G) % G, cell // (G * G)], axis=1)
        sets["plume"] = (ijk + rng.random((n, 3))) / G
        for name, pos in sets.items():
            rec = np.zeros((n, 4), f32)
            rec[:, :3] = pos.astype(f32)
            f.SetParticles(rec)
            f.SortParticles()
            ok = bool(np.array_equal(f.ParticleOrder(), np.argsort(keys(rec, G), kind="stable").astype(np.uint32)))
            row = {"particles": n, "arrangement": name, "order_is_numpy_stable_argsort": ok, "live": f.ParticleSortInfo()[0]}
            row["a_move_unsorted_ms"] = windows(f, lambda: f.SetParticles(rec), f.MoveParticles)
            row["b_sort_unsorted_ms"] = windows(f, lambda: f.SetParticles(rec), f.SortParticles, fresh_each=True)
            row["c_move_sorted_ms"] = windows(f, lambda: (f.SetParticles(rec), f.SortParticles()), f.MoveParticles)
            row["d_sort_sorted_ms"] = windows(f, lambda: (f.SetParticles(rec), f.SortParticles()), f.SortParticles)
            med = lambda k: float(np.median(row[k]))
            row["b_plus_c_ms"] = med("b_sort_unsorted_ms") + med("c_move_sorted_ms")
            row["pays_in_its_own_step"] = row["b_plus_c_ms"] < med("a_move_unsorted_ms")
            gain = med("a_move_unsorted_ms") - med("c_move_sorted_ms")
            row["break_even_every"] = med("b_sort_unsorted_ms") / gain if gain > 0 else None
            rows.append(row)
            print(json.dumps(row), flush=True)
    f.Release()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
