#!/usr/bin/env python3
"""What the obstacle draw costs (docs/LAB.md section 37): 256^3, a 1920 x 1080 viewport under the demo's camera, the shipped cast (the brick
walk inside the solids' bounding box) against the flat walk (one code byte per cell, no box, no bricks: the library built with
-DFX_ODRAW_FLAT, build.build_variant -- a timing build, not a shipped knob), on two masks:

  ball     the demo's ball (centre (.5, .45, .5), radius .15) handed over as a triangle mesh, fx_set_obstacle_meshes
  empty    an all-zero mask whose kernels stay in force: no ray ever hits, the longest walks the flat variant can take (the shipped cast
           knows the box is empty and casts like no mask)

The two libraries cannot live in one process (one set of symbols), so the variants alternate as child processes, `--rounds` rounds of
`--calls` timed fx_draw_obstacles each behind a warm-up; every call is timed on its own with HIP events (fx_timing.resolve_ms, the marks
around its launches).  Reported: median [min .. max] over all timed calls of a variant.  Beside them, for scale, the merged direct march of
the same frame (132 steps of the plume around the ball, the obstacle depth attached), fx_timing.view_ms.

  python tools/obstacle_draw_bench.py [--grid 256] [--viewport 1920 1080] [--rounds 4] [--calls 6] [--flat PATH] [--json FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ball_mesh(center, radius, stacks=16, slices=32):
    """the demo's UV sphere: poles on y"""
    v = [(0.0, 1.0, 0.0)]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        v += [(np.sin(th) * np.cos(2 * np.pi * j / slices), np.cos(th), np.sin(th) * np.sin(2 * np.pi * j / slices)) for j in range(slices)]
    v.append((0.0, -1.0, 0.0))
    v = (np.asarray(center)[None, :] + np.asarray(v) * radius).astype(np.float32)
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    south = 1 + (stacks - 1) * slices
    tri = []
    for j in range(slices):
        tri += [(0, ring(1, j), ring(1, j + 1)), (south, ring(stacks - 1, j + 1), ring(stacks - 1, j))]
    for i in range(1, stacks - 1):
        for j in range(slices):
            tri += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    return v, np.array(tri, np.uint32), None


def child(args):
    import fluidx12_amd as fx
    G, (W, H) = args.grid, args.viewport
    f = fx.Fluid()
    assert f.Init(W, H, (G, G, G), storage="fp16", jacobi_iters=40)
    view, proj, eye = fx.default_camera(W, H)
    f.UpdateFrame(f.default_time_step(), 0, view, proj, eye)
    f.SetObstacleDraw((0.8, 0.8, 0.8, 1.0))
    f.timing_enable(True)
    out = {}

    def timed(launch, field, n):
        for _ in range(3):
            launch()
        f.Synchronize()
        f.timing_read(reset=True)
        ms = []
        for _ in range(n):
            launch()
            f.Synchronize()
            ms.append(getattr(f.timing_read(reset=True), field))
        return ms

    for name in ("ball", "empty"):
        if name == "ball":
            rep = f.SetObstacleMeshes([ball_mesh((0.5, 0.45, 0.5), 0.15)])
            out["ball_solid_cells"] = rep["solid_cells"]
        else:
            f.SetObstacles(np.zeros((G, G, G), np.uint8))
        out[name + "_ms"] = timed(lambda: f.DrawObstacles(0), "resolve_ms", args.calls)
        hits, _ = f.ObstacleHits()
        out[name + "_hit_pixels"] = int((hits != 0).sum())
    if args.march:
        f.SetObstacleMeshes([ball_mesh((0.5, 0.45, 0.5), 0.15)])
        for i in range(132):
            f.UpdateFrame(f.default_time_step(), i % 3, view, proj, eye)
            f.Simulate(i % 3)
        f.DrawObstacles(0)
        f.AttachObstacleDepth()
        out["direct_march_ms"] = timed(lambda: f.Render(0, fx.Fluid.RAY_MARCH_DIRECT), "view_ms", args.calls)
        f.SetSceneDepth(None)
    f.Release()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--viewport", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--flat", default=os.path.join(ROOT, "tools", "_variants", "libfluidx_hip_odraw_flat.so"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--march", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not os.path.exists(args.flat):
        sys.exit("the flat variant %s is missing: python -c \"from fluidx12_amd import build; build.build_variant('odraw_flat', ['-DFX_ODRAW_FLAT'], "
                 "sources=('fx_obstacle_draw.hip',))\"" % args.flat)
    res = {"brick": {}, "flat": {}}
    for r in range(args.rounds):
        for variant in ("brick", "flat"):
            env = dict(os.environ)
            env.pop("FLUIDX_LIB_PATH", None)
            if variant == "flat":
                env["FLUIDX_LIB_PATH"] = args.flat
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--grid", str(args.grid), "--viewport", str(args.viewport[0]), str(args.viewport[1]),
                   "--calls", str(args.calls)] + (["--march"] if variant == "brick" and r == 0 else [])
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit("%s round %d failed (%d):\n%s" % (variant, r, p.returncode, p.stdout[-2000:]))   # nothing more is started
            for k, v in json.loads(line[0][7:]).items():
                if isinstance(v, list):
                    res[variant].setdefault(k, []).extend(v)
                else:
                    res[variant][k] = v
    for variant in ("brick", "flat"):
        for k, v in sorted(res[variant].items()):
            if isinstance(v, list):
                print("%-6s %-16s median %.4f ms [%.4f .. %.4f] over %d calls" % (variant, k, float(np.median(v)), min(v), max(v), len(v)))
            else:
                print("%-6s %-16s %s" % (variant, k, v))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
