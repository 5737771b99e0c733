"""numpy model of the multigrid pressure solver (include/fluidx_hip.h fx_set_pressure_solver, fluidx12_amd/csrc/fx_multigrid.hip): the rules in
fp32, every operation rounded as written, fused multiply-adds exact (fma_ref.fma).

  plan       the levels of a grid: level l + 1 halves every extent that is halved (X, Y, and Z of a 3-D grid) while each of them is even and >= 4
  smooth     p' = fma(omega, J - p, p),  J = ((((((L - b) + R) + U) + D) + F) + B) * INV6     (2-D: ((((L - b) + R) + U) + D) * 0.25)
  residual   r = fma(6, p, b - S),  S = (((((L + R) + U) + D) + F) + B)                        (2-D: 4 and four neighbours)
  restrict   b_c = 0.5 * (((r000 + r100) + (r010 + r110)) + ((r001 + r101) + (r011 + r111)))   (2-D: (r00 + r10) + (r01 + r11))
  prolong    per axis j = i >> 1, o = clamp(j + (i odd ? 1 : -1)), v = fma(0.25, e[o] - e[j], e[j]); x, then y, then z
  solve      `cycles` V-cycles; returns the pressure and what every coarse level holds afterwards

Neighbours by clamped index.  Layout [Z][Y][X] as Fluid.download; a 2-D grid has Z = 1.  The *_loops functions restate the four rules cell by
cell in plain Python (tests/test_multigrid_ref.py holds the array forms to them)."""
import math
import struct

import numpy as np

from fma_ref import fma
from open_ref import INV6

f32 = np.float32
MAX_LEVELS = 12
TAIL_CELLS = 4096


def defaults(dims):
    """the Python mirror's defaults: 2 V(2,2) cycles, 16 coarse sweeps, omega 6/7 in 3-D and 4/5 in 2-D"""
    return dict(cycles=2, pre=2, post=2, coarse=16, max_levels=0, omega=f32(6.0 / 7.0) if dims[2] > 1 else f32(4.0 / 5.0))


def plan(dims, max_levels=0):
    """[(X, Y, Z)] per level"""
    X, Y, Z = dims
    is3d = Z > 1
    cap = max_levels if 0 < max_levels < MAX_LEVELS else MAX_LEVELS
    out = [(X, Y, Z)]
    while len(out) < cap:
        halved = (X, Y, Z) if is3d else (X, Y)
        if any(n % 2 or n < 4 for n in halved):
            break
        X, Y, Z = X // 2, Y // 2, (Z // 2 if is3d else 1)
        out.append((X, Y, Z))
    return out


def tail_level(levels):
    """the first level >= 1 with at most TAIL_CELLS cells whose tail fits 64 KiB of LDS, or 0"""
    n = [x * y * z for x, y, z in levels]
    for l in range(1, len(levels)):
        if n[l] <= TAIL_CELLS and 4 * (n[l] + 2 * sum(n[l:])) <= 64 * 1024:
            return l
    return 0


def _shift(a, axis, d):
    n = a.shape[axis]
    return np.take(a, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def smooth(p, b, omega, n=1):
    p, b, omega = np.asarray(p, f32), np.asarray(b, f32), f32(omega)
    is3d = p.shape[0] > 1
    for _ in range(int(n)):
        s = _shift(p, 2, -1) - b
        s = s + _shift(p, 2, 1)
        s = s + _shift(p, 1, -1)
        s = s + _shift(p, 1, 1)
        if is3d:
            s = s + _shift(p, 0, -1)
            s = s + _shift(p, 0, 1)
            J = s * INV6
        else:
            J = s * f32(0.25)
        p = fma(omega, J - p, p)
    return p


def residual(p, b):
    p, b = np.asarray(p, f32), np.asarray(b, f32)
    is3d = p.shape[0] > 1
    S = _shift(p, 2, -1) + _shift(p, 2, 1)
    S = S + _shift(p, 1, -1)
    S = S + _shift(p, 1, 1)
    if is3d:
        S = S + _shift(p, 0, -1)
        S = S + _shift(p, 0, 1)
    return fma(f32(6.0 if is3d else 4.0), p, b - S)


def restrict(r):
    r = np.asarray(r, f32)
    is3d = r.shape[0] > 1
    sx = r[:, :, 0::2] + r[:, :, 1::2]                 # r0.. + r1..
    sy = sx[:, 0::2, :] + sx[:, 1::2, :]               # (r00. + r10.) + (r01. + r11.)
    if not is3d:
        return sy
    return f32(0.5) * (sy[0::2] + sy[1::2])


def _prolong_axis(e, axis, n_fine):
    nc = e.shape[axis]
    i = np.arange(n_fine)
    j = i >> 1
    o = np.clip(j + np.where(i & 1, 1, -1), 0, nc - 1)
    ej, eo = np.take(e, j, axis=axis), np.take(e, o, axis=axis)
    return fma(f32(0.25), eo - ej, ej)


def prolong(e, fine_shape):
    """the correction on the fine grid (the caller adds it)"""
    e = np.asarray(e, f32)
    Z, Y, X = fine_shape
    v = _prolong_axis(e, 2, X)
    v = _prolong_axis(v, 1, Y)
    if Z > 1:
        v = _prolong_axis(v, 0, Z)
    return v


def _cycle(l, levels, e, b, prm):
    """-> the level's new solution; fills e[l + 1 ..], b[l + 1 ..]"""
    p = e[l]
    if l == len(levels) - 1:
        e[l] = smooth(p, b[l], prm["omega"], prm["coarse"])
        return e[l]
    p = smooth(p, b[l], prm["omega"], prm["pre"])
    b[l + 1] = restrict(residual(p, b[l]))
    e[l + 1] = np.zeros_like(b[l + 1])
    _cycle(l + 1, levels, e, b, prm)
    p = p + prolong(e[l + 1], p.shape)
    e[l] = smooth(p, b[l], prm["omega"], prm["post"])
    return e[l]


def solve(p, b, prm=None, **kw):
    """one fx_pressure_solve -> (p, [None, (e_1, b_1), (e_2, b_2), ...]): the pressure and what every coarse level holds afterwards"""
    p, b = np.asarray(p, f32), np.asarray(b, f32)
    Z, Y, X = p.shape
    prm = dict(defaults((X, Y, Z)) if prm is None else prm, **kw)
    levels = plan((X, Y, Z), prm.get("max_levels", 0))
    e, bb = [p] + [None] * (len(levels) - 1), [b] + [None] * (len(levels) - 1)
    for _ in range(int(prm["cycles"])):
        _cycle(0, levels, e, bb, prm)
    return e[0], [None] + [(e[l], bb[l]) for l in range(1, len(levels))]


def residual64(p, b):
    """the residual of the same fp32 arrays evaluated in float64 (no rounding to speak of): what `residual` is measured against"""
    p, b = np.asarray(p, np.float64), np.asarray(b, np.float64)
    S, k = np.zeros_like(p), 0
    for axis in range(3):
        if p.shape[axis] > 1:
            S += _shift(p, axis, -1) + _shift(p, axis, 1)
            k += 2
    return k * p + (b - S)


def residual_error(p, b):
    """rms of what fp32 adds to the residual of this pressure: `residual` against `residual64`"""
    d = residual(p, b).astype(np.float64) - residual64(p, b)
    return float(np.sqrt((d * d).mean()))


def rms_residual(p, b):
    """rms of the mean-removed residual, in float64"""
    r = residual(p, b).astype(np.float64)
    r -= r.mean()
    return float(np.sqrt((r * r).mean()))


def plume_rhs(dims, seed=7):
    """two Gaussians of opposite sign plus 0.05 sigma seeded noise, the mean removed: the divergence of a velocity that does not cross the
    closed walls sums to zero, and only such a right-hand side has a solution"""
    X, Y, Z = dims
    z, y, x = np.meshgrid((np.arange(Z) + 0.5) / Z, (np.arange(Y) + 0.5) / Y, (np.arange(X) + 0.5) / X, indexing="ij")
    if Z == 1:
        z = np.full_like(z, 0.5)

    def g(cx, cy, cz, r):
        return np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (r * r))
    b = g(0.5, 0.25, 0.5, 0.12) - g(0.45, 0.6, 0.55, 0.18)
    b += 0.05 * b.std() * np.random.default_rng(seed).standard_normal(b.shape)
    return (b - b.mean()).astype(f32)


# ---- the same rules cell by cell ----------------------------------------------------------------------------------------------------------------
def _f(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _fma1(a, b, c):
    return float(fma(f32(a), f32(b), f32(c)))


def _cl(i, n):
    return min(max(i, 0), n - 1)


def smooth_loops(p, b, omega):
    Z, Y, X = p.shape
    out = np.empty_like(p)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                s = _f(float(p[z, y, _cl(x - 1, X)]) - float(b[z, y, x]))
                s = _f(s + float(p[z, y, _cl(x + 1, X)]))
                s = _f(s + float(p[z, _cl(y - 1, Y), x]))
                s = _f(s + float(p[z, _cl(y + 1, Y), x]))
                if Z > 1:
                    s = _f(s + float(p[_cl(z - 1, Z), y, x]))
                    s = _f(s + float(p[_cl(z + 1, Z), y, x]))
                    J = _f(s * float(INV6))
                else:
                    J = _f(s * 0.25)
                out[z, y, x] = _fma1(omega, _f(J - float(p[z, y, x])), p[z, y, x])
    return out


def residual_loops(p, b):
    Z, Y, X = p.shape
    out = np.empty_like(p)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                S = _f(float(p[z, y, _cl(x - 1, X)]) + float(p[z, y, _cl(x + 1, X)]))
                S = _f(S + float(p[z, _cl(y - 1, Y), x]))
                S = _f(S + float(p[z, _cl(y + 1, Y), x]))
                if Z > 1:
                    S = _f(S + float(p[_cl(z - 1, Z), y, x]))
                    S = _f(S + float(p[_cl(z + 1, Z), y, x]))
                out[z, y, x] = _fma1(6.0 if Z > 1 else 4.0, p[z, y, x], _f(float(b[z, y, x]) - S))
    return out


def restrict_loops(r):
    Z, Y, X = r.shape
    is3d = Z > 1
    out = np.empty((Z // 2 if is3d else 1, Y // 2, X // 2), f32)
    for zc in range(out.shape[0]):
        for yc in range(out.shape[1]):
            for xc in range(out.shape[2]):
                def R(i, j, k):
                    return float(r[(2 * zc + k) if is3d else 0, 2 * yc + j, 2 * xc + i])
                lo = _f(_f(R(0, 0, 0) + R(1, 0, 0)) + _f(R(0, 1, 0) + R(1, 1, 0)))
                if is3d:
                    hi = _f(_f(R(0, 0, 1) + R(1, 0, 1)) + _f(R(0, 1, 1) + R(1, 1, 1)))
                    out[zc, yc, xc] = _f(0.5 * _f(lo + hi))
                else:
                    out[zc, yc, xc] = lo
    return out


def prolong_loops(e, fine_shape):
    Z, Y, X = fine_shape
    Zc, Yc, Xc = e.shape

    def other(i, nc):
        return _cl((i >> 1) + (1 if i & 1 else -1), nc)

    def lerp(ej, eo):
        return _fma1(0.25, _f(eo - ej), ej)
    out = np.empty(fine_shape, f32)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                def along_x(zz, yy):
                    return lerp(float(e[zz, yy, x >> 1]), float(e[zz, yy, other(x, Xc)]))

                def along_y(zz):
                    return lerp(along_x(zz, y >> 1), along_x(zz, other(y, Yc)))
                out[z, y, x] = lerp(along_y(z >> 1), along_y(other(z, Zc))) if Z > 1 else along_y(0)
    return out


assert math.isclose(float(INV6), 1.0 / 6.0, rel_tol=1e-6)
