"""numpy model of the moving obstacles (include/fluidx_hip.h fx_set_obstacle_bodies, fluidx12_amd/csrc/fx_obstacle.hip): the rules in
fp32, every operation rounded as written.

  wall_velocity   w(n) = linear + angular x r of every cell as if it were solid: the first body whose closed box holds the cell centre, +0 if none
  ref_enforce     a solid cell's VELOCITY1 = w(c) (rounded once to the storage), its colour +0
  ref_divergence  v_a(n) read as S(n) ? w_a(n) : v_a(n), b = 0 in a solid cell
  ref_jacobi      tests/open_ref.py's: the relaxation does not see the bodies
  ref_project     open_ref.ref_project with u[a] = the wall's w_a beside a solid along a (their mean between two), w(c) in a solid cell
  ref_step        enforce, divergence, sweeps, projection behind an advected state

With no bodies, or bodies whose boxes hold no solid cell, the first, third and fifth are tests/obstacle_ref/ and open_ref bit for bit
(tests/test_moving_obstacle_ref.py holds them to that).  The fused multiply-adds are tests/fma_ref.py's, correctly rounded.

Layouts as Fluid.upload / download: velocity float32[3][Z][Y][X], colour float32[Z][Y][X][4], pressure, divergence and masks [Z][Y][X].
A body is a dict with the keys of Fluid.SetObstacleBodies: box_lo, box_hi, linear, angular, pivot (all given)."""
import numpy as np

import open_ref as orf
from fma_ref import fma
from open_ref import NEIGHBOURS, KD3, _q, _shift, _solid

f32 = np.float32
ref_jacobi = orf.ref_jacobi


def body(box_lo, box_hi, linear=(0.0, 0.0, 0.0), angular=(0.0, 0.0, 0.0), pivot=None):
    lo, hi = [float(f32(v)) for v in box_lo], [float(f32(v)) for v in box_hi]
    if pivot is None:
        pivot = [0.5 * (a + b) for a, b in zip(lo, hi)]
    return {"box_lo": tuple(lo), "box_hi": tuple(hi), "linear": tuple(float(f32(v)) for v in linear),
            "angular": tuple(float(f32(v)) for v in angular), "pivot": tuple(float(f32(v)) for v in pivot)}


def cell_centres(shape):
    """pos_a of every cell, a = x, y, z, each broadcast to [Z][Y][X]: ((float)i + 0.5f) / (float)N"""
    Z, Y, X = shape
    out = []
    for n, sh in ((X, (1, 1, X)), (Y, (1, Y, 1)), (Z, (Z, 1, 1))):
        pos = (np.arange(n, dtype=f32) + f32(0.5)) / f32(n)
        out.append(np.broadcast_to(pos.astype(f32).reshape(sh), shape))
    return out


def body_of(shape, bodies):
    """index of B(n) per cell, -1 = none"""
    pos = cell_centres(shape)
    is3d = shape[0] > 1
    who = np.full(shape, -1, np.int32)
    for k, b in enumerate(bodies or ()):
        inside = np.ones(shape, bool)
        for a in range(3 if is3d else 2):
            inside &= (f32(b["box_lo"][a]) <= pos[a]) & (pos[a] <= f32(b["box_hi"][a]))
        who = np.where((who < 0) & inside, k, who)
    return who


def wall_velocity(shape, bodies):
    """float32[3][Z][Y][X]: w(n) of every cell as if it were solid"""
    pos = cell_centres(shape)
    is3d = shape[0] > 1
    who = body_of(shape, bodies)
    w = np.zeros((3,) + tuple(shape), f32)
    for k, b in enumerate(bodies or ()):
        lin, ang = [f32(v) for v in b["linear"]], [f32(v) for v in b["angular"]]
        r = [(pos[a] - f32(b["pivot"][a])).astype(f32) for a in range(3)]
        if is3d:
            wk = [fma(ang[1], r[2], fma(-ang[2], r[1], lin[0])),
                  fma(ang[2], r[0], fma(-ang[0], r[2], lin[1])),
                  fma(ang[0], r[1], fma(-ang[1], r[0], lin[2]))]
        else:
            wk = [fma(-ang[2], r[1], lin[0]), fma(ang[2], r[0], lin[1]), np.zeros(shape, f32)]
        for a in range(3):
            w[a] = np.where(who == k, np.broadcast_to(np.asarray(wk[a], f32), shape), w[a])
    return w


def ref_enforce(vel, col, mask, bodies, half=False):
    """-> (vel, col): solid cells at w(c) / +0"""
    v, c = np.array(vel, f32), np.array(col, f32)
    solid = _solid(mask, c.shape[:3])
    w = wall_velocity(solid.shape, bodies)
    if half:
        w = w.astype(np.float16).astype(f32)
    for a in range(3):
        v[a] = np.where(solid, w[a], v[a])
    c[solid] = f32(0.0)
    return v, c


def ref_divergence(vel, mask, bodies):
    vel = np.asarray(vel, f32)
    shape = vel.shape[1:]
    solid = _solid(mask, shape)
    is3d = shape[0] > 1
    w = wall_velocity(shape, bodies)
    dd = []
    for a in range(3 if is3d else 2):
        (ax, dm, _), (_, dp, _) = NEIGHBOURS[2 * a], NEIGHBOURS[2 * a + 1]
        va = np.where(solid, w[a], vel[a]).astype(f32)
        dd.append((-_shift(va, ax, dm) + _shift(va, ax, dp)).astype(f32))
    S = (dd[2] + (dd[1] + dd[0])) if is3d else (dd[0] + dd[1])
    return np.where(solid, f32(0.0), f32(0.5) * S).astype(f32)


def ref_project(vel, p, mask, bodies, faces=0, half=False):
    vel, p = np.asarray(vel, f32), np.asarray(p, f32)
    Z, Y, X = p.shape
    solid = _solid(mask, p.shape)
    is3d = Z > 1
    assert is3d or not (faces & (orf.Z_LO | orf.Z_HI))
    kd = KD3 if is3d else f32(0.5)
    w = wall_velocity(p.shape, bodies)
    u = [vel[a].copy() for a in range(3)]
    for a in range(3 if is3d else 2):
        (ax, dm, bm), (_, dp, bp) = NEIGHBOURS[2 * a], NEIGHBOURS[2 * a + 1]
        grad = -_q(p, solid, faces, ax, dm, bm) + _q(p, solid, faces, ax, dp, bp)
        u[a] = fma(-grad, kd, u[a])
        sm, sp = _shift(solid, ax, dm), _shift(solid, ax, dp)
        wm, wp = _shift(w[a], ax, dm), _shift(w[a], ax, dp)
        slip = np.where(sm & sp, f32(0.5) * (wm + wp), np.where(sm, wm, wp)).astype(f32)
        u[a] = np.where(sm | sp, slip, u[a]).astype(f32)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    out = np.empty_like(vel)
    for a, (cell, n) in enumerate(((x, X), (y, Y), (z, Z))):
        pos = (cell.astype(f32) + f32(0.5)) / f32(n)
        if is3d or a < 2:
            pos = fma(pos, f32(2.0), f32(-1.0))
        f = (-np.abs(pos) + f32(0.970000029)) * f32(33.3333359)
        f = np.minimum(np.maximum(f, f32(-1.0)), f32(1.0))
        opened = ((pos < 0) & bool(faces & (1 << (2 * a)))) | ((pos > 0) & bool(faces & (2 << (2 * a))))
        damp = np.where((f32(0.0) < u[a] * pos) & ~opened, f, f32(1.0)).astype(f32)
        r = np.where(solid, w[a], u[a] * damp).astype(f32)
        out[a] = r.astype(np.float16).astype(f32) if half else r
    return out


def ref_step(vel1, col, p, mask, bodies, sweeps, faces=0, half=False):
    """the step behind the advection (no emitters, buoyancy or confinement): -> (velocity1, colour, b, pressure, velocity)"""
    v1, c1 = ref_enforce(vel1, col, mask, bodies, half)
    b = ref_divergence(v1, mask, bodies)
    q = ref_jacobi(p, b, mask, faces, sweeps)
    return v1, c1, b, q, ref_project(v1, q, mask, bodies, faces, half)
