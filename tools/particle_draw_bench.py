#!/usr/bin/env python3
"""What the particle draw costs (docs/LAB.md section 36), on docs/LAB.md section 30's terms: 256^3, 40 sweeps, the default time step, the
built-in impulse, 132 steps to develop the plume (bench.py's developed frame), a 1280 x 720 viewport under the demo's camera, 2^20 particles
born by one ball spawner inside the plume with ages spread over the lifetime.  Everything is timed with HIP events through fx_timing (the marks
around the launches of a call): three windows of 10 launches behind a warm-up, per row

  splat    k_draw_splat alone (fx_particle_splats; its copy to the host lies outside the events)           fx_timing.resolve_ms
  draw     fx_draw_particles, both launches; resolve = draw - splat                                         fx_timing.resolve_ms
  floor    k_draw_resolve on an all-zero accumulator (no set of particles): 16 bytes per pixel read, 16 written
  march    the direct view march of the same frame (fx_render, merged and with the separate light pass)     fx_timing.view_ms (+ light_ms)
  move     fx_move_particles of the same set                                                                fx_timing.project_ms

for the set as the spawner leaves it ("shuffled": a record's place is a hash of its serial) and sorted by the device ("sorted"), with
FX_OPT_RENDER_ACCEL on and off (the draw's own march gathers every sample under either; the switch changes the view march beside it).

  python tools/particle_draw_bench.py [--grid 256] [--steps 132] [--log2 20] [--viewport 1280 720] [--storage fp16 fp32] [--json FILE]
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

LIFETIME = 4.0


def windows(f, launch, field, n=10, reps=3):
    """the sum of the fx_timing members `field` per launch of `launch`: `reps` windows of `n` launches behind a warm-up"""
    out = []
    for _ in range(reps):
        launch()
        f.Synchronize()
        f.timing_read(reset=True)
        for _ in range(n):
            launch()
        f.Synchronize()
        t = f.timing_read(reset=True)
        out.append(sum(getattr(t, k) for k in field) / n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--steps", type=int, default=132)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--viewport", type=int, nargs=2, default=[1280, 720])
    ap.add_argument("--storage", nargs="+", default=["fp16", "fp32"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    G, (W, H), n = args.grid, args.viewport, 1 << args.log2
    med = lambda v: float(np.median(v))
    rows = []
    for storage in args.storage:
        f = fx.Fluid()
        assert f.Init(W, H, (G, G, G), storage=storage, jacobi_iters=40)
        view, proj, eye = fx.default_camera(W, H)
        dt = f.default_time_step()
        for i in range(args.steps):
            f.UpdateFrame(dt, i % 3, view, proj, eye)
            f.Simulate(i % 3)
        f.Synchronize()
        # the set: a pool of n dead records filled in one run of the spawn stage
        f.SetParticleParams(lifetime=LIFETIME)
        f.SetParticlePool(n)
        f.SetParticleSpawners([{"shape": "ball", "seed": 34, "center": (0.5, 0.3, 0.5), "half_extent": (0.15, 0.25, 0.15),
                                "rate": (n + 0.5) / dt, "age_spread": LIFETIME}])
        f.SpawnParticles()
        born = f.ParticleSpawnInfo()["born"]
        f.SetParticleSpawners(None)
        f.SetParticleSort(True)
        f.SetParticleDraw((1.0, 0.6, 0.2, 4.0), (0.6, 0.1, 0.0, 1.0))
        f.timing_enable(True)
        shuffled = f.GetParticles()
        for accel in (1, 0):
            f.set_option(capi.OPT_RENDER_ACCEL, accel)
            row = {"storage": storage, "accel": accel, "row": "march", "viewport": [W, H]}
            row["direct_merged_view_ms"] = windows(f, lambda: f.Render(0, fx.Fluid.RAY_MARCH_DIRECT), ("view_ms",))
            row["direct_separate_light_plus_view_ms"] = windows(f, lambda: f.Render(0, fx.Fluid.SEPARATE_LIGHT_PASS), ("light_ms", "view_ms"))
            rows.append(row)
            print(json.dumps(row), flush=True)
            for name in ("shuffled", "sorted"):
                f.SetParticles(shuffled)
                if name == "sorted":
                    f.SortParticles()
                acc = f.ParticleSplats()
                row = {"storage": storage, "accel": accel, "particles": n, "born": int(born), "arrangement": name,
                       "pixels_hit": int(((acc[..., 0] | acc[..., 1]) != 0).sum()), "mean_transmittance": float(acc.sum()) / float(n << 37)}
                row["splat_ms"] = windows(f, f.ParticleSplats, ("resolve_ms",))
                row["draw_ms"] = windows(f, lambda: f.DrawParticles(0), ("resolve_ms",))
                row["resolve_ms"] = med(row["draw_ms"]) - med(row["splat_ms"])
                row["G_particles_per_s"] = n / med(row["splat_ms"]) / 1e6
                rows.append(row)
                print(json.dumps(row), flush=True)
        f.SetParticles(shuffled)
        f.SortParticles()
        row = {"storage": storage, "row": "move", "particles": n, "move_sorted_ms": windows(f, f.MoveParticles, ("project_ms",))}
        f.SetParticles(shuffled)
        row["move_shuffled_ms"] = windows(f, f.MoveParticles, ("project_ms",))
        f.SetParticles(None)
        row["resolve_floor_ms"] = windows(f, lambda: f.DrawParticles(0), ("resolve_ms",))
        rows.append(row)
        print(json.dumps(row), flush=True)
        f.Release()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
