"""What a new obstacle mask costs per call (fx_set_obstacles against fx_set_obstacle_meshes; csrc/fx_voxelize.hip): a table for docs/LAB.md,
not a figure of bench.py.

    python tools/voxelize_bench.py [--grid 256] [--calls 60] [--warmup 10] [--repeats 3] [--storage fp32] [--mask-only] [--legs a,b,c] [--json out.json]

One process, one context.  A call blocks until the mask is installed (both setters synchronise their stream), so the wall time around a call
is the stream-synchronised time of everything it enqueues.  Legs:
  a  fx_set_obstacles with a host mask: the ball of tools/moving_obstacle_bench.py, X * Y * Z bytes uploaded per call
  b  fx_set_obstacle_meshes with a UV sphere of about 100 000 triangles (224 x 224 segments), positions and indices resident on the device,
     a new 48-byte transform (on the device too) per call
  c  the same call with three thin slabs that reach through the y and z walls: twelve wall-sized triangles, every column covered six times
     (and 24 edge-on triangles that close the slabs); about the solid cells of leg b -- the launch that builds the code volume
     (k_obstacle_codes) costs by the solid cells it counts, the same for either setter
Every repeat prints one line per leg: the minimum, the median and the range over its calls, in ms.  --mask-only runs leg a alone and also takes
a library that predates the mesh setter (FLUIDX_LIB_PATH=...): the figure of an older build, for the comparison across commits.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fluidx12_amd import capi  # noqa: E402


def ball(n, center=(0.5, 0.45, 0.5), radius=0.22):
    c = (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return ((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2 <= radius * radius).astype(np.uint8)


def uv_sphere(center, radius, stacks, slices):
    th = np.pi * np.arange(1, stacks) / stacks
    ph = 2.0 * np.pi * np.arange(slices) / slices
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(slices)), np.outer(np.sin(th), np.sin(ph))], axis=2).reshape(-1, 3)
    v = np.vstack([[[0.0, 1.0, 0.0]], ring, [[0.0, -1.0, 0.0]]]) * radius + np.asarray(center)[None, :]
    i, j = np.meshgrid(np.arange(1, stacks - 1), np.arange(slices), indexing="ij")
    at = lambda i, j: 1 + (i - 1) * slices + j % slices
    quads = np.stack([at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)], axis=2).reshape(-1, 4)
    j = np.arange(slices)
    south = 1 + (stacks - 1) * slices
    tri = np.vstack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]], np.stack([np.zeros_like(j), at(1, j), at(1, j + 1)], axis=1),
                     np.stack([np.full_like(j, south), at(stacks - 1, j + 1), at(stacks - 1, j)], axis=1)])
    return v.astype(np.float32), tri.astype(np.uint32)


def box(lo, hi):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], np.float32)
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)


def slabs(at=(0.3, 0.5, 0.7), thick=0.03):
    """three sheared slabs that reach through the y and z walls: each has four triangles that cover every column of the grid and eight that
    are edge-on; about as many solid cells as leg b's ball, so that the code volume's launch costs both legs the same"""
    vs, ts = [], []
    for k, x in enumerate(at):
        v, t = box((x, -0.5, -0.5), (x + thick, 1.5, 1.5))
        v[:, 0] += 0.04 * (v[:, 1] - 0.5) + 0.02 * (v[:, 2] - 0.5)
        vs.append(v)
        ts.append(t + 8 * k)
    return np.vstack(vs), np.vstack(ts).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--storage", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--mask-only", action="store_true")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    legs = ["a"] if a.mask_only else [x for x in a.legs.split(",") if x]
    if a.mask_only:                                    # (a library from before the call lacks the symbol; leg a never asks for it)
        capi.SYMBOLS.pop("fx_set_obstacle_meshes", None)
    import fluidx12_amd as fx
    n = a.grid
    f = fx.Fluid()
    if not f.Init(0, 0, (n, n, n), jacobi_iters=40, storage=a.storage):
        raise SystemExit("Init failed: %d" % f.last_status)
    calls, report = {}, {}
    if "a" in legs:
        mask = ball(n)
        calls["a"] = lambda k: f.SetObstacles(mask)
    if "b" in legs or "c" in legs:
        import torch
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        # the transforms of a ball that walks along x, one per call, resident like the mesh: what a caller's animation system leaves on the device
        xfs = dev(np.stack([np.array([1, 0, 0, 0.2 * np.sin(0.1 * k), 0, 1, 0, 0, 0, 0, 1, 0], np.float32) for k in range(64)]))
        for leg, (v, t) in (("b", uv_sphere((0.5, 0.45, 0.5), 0.22, 224, 224)), ("c", slabs())):
            if leg in legs:
                dv, dt = dev(v), dev(t.view(np.int32))
                calls[leg] = (lambda k, dv=dv, dt=dt, leg=leg: report.__setitem__(leg, f.SetObstacleMeshes([(dv, dt, xfs[k % 64])])))
                print("leg %s: %d triangles, %d vertices" % (leg, len(t), len(v)))
    rows = []
    print("leg rep    min_ms  median_ms  range_ms   (%s, grid %d^3 %s, %d calls per leg and repeat)" % (os.environ.get("FLUIDX_LIB_PATH", "the tree's library"), n, a.storage, a.calls))
    for leg in legs:
        for k in range(a.warmup):
            calls[leg](k)
    for rep in range(a.repeats):
        for leg in legs:                               # alternating: a b c, a b c, ...
            ms = []
            for k in range(a.calls):
                f.Synchronize()
                t0 = time.perf_counter()
                calls[leg](k)
                ms.append((time.perf_counter() - t0) * 1e3)
            row = {"leg": leg, "repeat": rep, "min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "range_ms": float(np.ptp(ms))}
            rows.append(row)
            print("%-3s %3d  %8.4f  %9.4f  %8.4f" % (leg, rep, row["min_ms"], row["median_ms"], row["range_ms"]), flush=True)
    for leg in legs:
        mine = [r for r in rows if r["leg"] == leg]
        print("%s: min %.4f ms, medians %.4f .. %.4f ms%s" % (leg, min(r["min_ms"] for r in mine), min(r["median_ms"] for r in mine), max(r["median_ms"] for r in mine),
                                                           "" if leg == "a" else "  report %s" % (report.get(leg),)))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"grid": n, "storage": a.storage, "calls": a.calls, "library": os.environ.get("FLUIDX_LIB_PATH"), "rows": rows}, fh, indent=1)
    f.Release()


if __name__ == "__main__":
    main()
