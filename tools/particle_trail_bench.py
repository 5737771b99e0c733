#!/usr/bin/env python3
"""What the particle trail costs (docs/LAB.md section 32), on docs/LAB.md section 30's terms: 256^3, 40 sweeps, the default time step, the
built-in impulse, 160 steps to develop the plume.  Everything is timed through fx_timing.advect_ms (HIP events around the launches of the
stage): three windows of 10 launches behind a warm-up, per row

  splat    k_trail_splat alone (the scatter of fx_particle_density; its copy to the host lies outside the events), merged and -- on a lab build of
           the library, FLUIDX_LIB_PATH=tools/_variants/libfluidx_hip_lab.so -- with TRAIL_MERGE = 0
  deposit  fx_deposit_particles, both launches; apply = deposit - splat
  floor    k_trail_apply on an accumulator one record has touched: 8 bytes per cell read and nothing else
  step     fx_simulate with and without the trail (all four marks of fx_timing summed)

for 2^20 and 2^22 particles: uniform in [0,1)^3 ("shuffled"), the same set sorted by the device ("sorted"), drawn cell by cell with
probability proportional to alpha where alpha > 0.01 and then shuffled ("plume"), and all on one point ("one_point").  The splat does not
read a field, so it is timed on the fp16 context only.

  python tools/particle_trail_bench.py [--grid 256] [--steps 160] [--log2 20 22] [--storage fp16 fp32] [--json FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidx12_amd as fx                                                     # noqa: E402
from fluidx12_amd import capi                                                 # noqa: E402

f32 = np.float32


def windows(f, launch, n=10, reps=3):
    """advect_ms per launch of `launch`: `reps` windows of `n` launches behind a warm-up"""
    out = []
    for _ in range(reps):
        launch()
        f.Synchronize()
        f.timing_read(reset=True)
        for _ in range(n):
            launch()
        f.Synchronize()
        out.append(f.timing_read(reset=True).advect_ms / n)
    return out


def step_ms(f, dt, n=20, reps=3):
    out = []
    for _ in range(reps):
        f.UpdateFrame(dt, 0); f.Simulate(0)
        f.Synchronize()
        f.timing_read(reset=True)
        for i in range(n):
            f.UpdateFrame(dt, i % 3); f.Simulate(i % 3)
        f.Synchronize()
        t = f.timing_read(reset=True)
        out.append((t.advect_ms + t.divergence_ms + t.jacobi_ms + t.project_ms) / n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--storage", nargs="+", default=["fp16", "fp32"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    G = args.grid
    lab = "TRAIL_MERGE" in capi.knob_names()
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
        alpha = f.download(fx.FIELD_COLOR)[..., 3].astype(np.float64).ravel()
        alpha[alpha <= 0.01] = 0.0
        rng = np.random.default_rng(31)
        f.SetParticleSort(True)
        f.SetParticleTrail(1.0, (1e-4, 1e-4, 1e-4, 1e-4), 0.0)
        f.timing_enable(True)
        one = np.zeros((1, 4), f32)
        one[0, :3] = 0.5
        f.SetParticles(one)
        floor = windows(f, f.DepositParticles)
        row = {"storage": storage, "row": "apply_floor", "ms": floor, "GBps_of_8B_per_cell": 8.0 * G ** 3 / med(floor) / 1e6}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for lg in args.log2:
            n = 1 << lg
            sets = {"shuffled": rng.random((n, 3)), "sorted": None}
            cell = rng.choice(alpha.size, size=n, p=alpha / alpha.sum())
            ijk = np.stack([cell % G, (cell // G) % G, cell // (G * G)], axis=1)
            sets["plume"] = rng.permutation((ijk + rng.random((n, 3))) / G)
            sets["one_point"] = np.tile(np.array([[0.5, 0.3, 0.5]]), (n, 1))
            for name, pos in sets.items():
                rec = np.zeros((n, 4), f32)
                rec[:, :3] = (sets["shuffled"] if pos is None else pos).astype(f32)
                f.SetParticles(rec)
                if name == "sorted":
                    f.SortParticles()
                row = {"storage": storage, "particles": n, "arrangement": name}
                if storage == args.storage[0]:
                    total = int(f.ParticleDensity().sum())
                    row["sum_is_live_times_2_24"] = total == n << 24
                    row["splat_merged_ms"] = windows(f, f.ParticleDensity)
                    if lab:
                        capi.set_knob("TRAIL_MERGE", "0")
                        row["splat_unmerged_ms"] = windows(f, f.ParticleDensity)
                        capi.set_knob("TRAIL_MERGE", None)
                        row["merge_speedup"] = med(row["splat_unmerged_ms"]) / med(row["splat_merged_ms"])
                    row["G_particles_per_s"] = n / med(row["splat_merged_ms"]) / 1e6
                row["deposit_ms"] = windows(f, f.DepositParticles)
                rows.append(row)
                print(json.dumps(row), flush=True)
        # the step with the plume-shaped set of the last count, with and without the trail (particles moving, sorted every 8th step)
        rec = np.zeros((1 << args.log2[-1], 4), f32)
        rec[:, :3] = sets["plume"].astype(f32)
        f.SetParticleSort(True, 8)
        row = {"storage": storage, "row": "step", "particles": len(rec)}
        f.SetParticles(rec)
        row["step_with_trail_ms"] = step_ms(f, dt)
        f.SetParticleTrail(None)
        f.SetParticles(rec)
        row["step_without_trail_ms"] = step_ms(f, dt)
        f.SetParticles(None)
        row["step_without_particles_ms"] = step_ms(f, dt)
        rows.append(row)
        print(json.dumps(row), flush=True)
        f.Release()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
