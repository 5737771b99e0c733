"""numpy model of the buoyancy pass (include/fluidx_hip.h fx_set_buoyancy, fluidx12_amd/csrc/fx_heat.hip: k_heat).

The pass in fp32, operation by operation (rules 1-6 of the header comment), with the liberty of tests/emitter_ref.py: the basis of a heat
source is evaluated in float64 and rounded once.  (A fused multiply-add is fmaf's, correctly rounded: tests/fma_ref.py.)  So the tests compare
  * outside every heat source's support: bit for bit, temperature and velocity, and
  * inside: rel-L2 < 1e-6, the project's figure for exp2 in fp32 against float64 (tests/test_gpu_emitters.py),
and they assert first (emitter_ref.near_threshold) that no cell's basis sits so close to e^-4 that an ulp of exp2 decides its side.

Layouts as Fluid.upload / download: velocity float32[3][Z][Y][X], colour float32[Z][Y][X][4], temperature and masks [Z][Y][X]."""
import numpy as np

import emitter_ref as er
from fma_ref import fma

f32, f64 = np.float32, np.float64

# Where the tests put their heat sources: the six (centre, radius) pairs SIX of tests/test_gpu_emitters.py (tests/test_gpu_buoyancy.py asserts
# that the two agree) -- the built-in ball's place, one well inside, one clipped by two walls, one more, the whole grid, one without a cell --
# with a rate each (the second is a cold source), and the grids of the GPU tests: rows shorter than a tile; a ragged second x tile; a power of
# two; the staged advection's grid; 150-cell rows; the tuned row length; 2-D.  One copy, so that the CPU check "no cell near the threshold"
# (tests/test_buoyancy_ref.py) covers exactly what the GPU tests run.
SIX = [((0.5, 0.1, 0.5), 1 / 16), ((0.3, 0.6, 0.4), 0.11), ((0.02, 0.97, 0.5), 0.2), ((0.7, 0.3, 0.55), 0.13), ((0.5, 0.5, 0.5), 1.0),
       ((0.41, 0.37, 0.52), 0.004)]
RATES = [30.0, -12.0, 55.0, 20.0, 8.0, 70.0]
SHAPES = [(20, 20, 12), (70, 70, 5), (32, 32, 32), (64, 64, 16), (150, 150, 6), (256, 256, 6), (36, 36, 1), (64, 64, 1)]

DEFAULTS = dict(ambient=0.0, density_weight=0.0, lift=0.0, cooling=0.0, up=(0.0, 1.0, 0.0))


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def source(center, radius, rate):
    return dict(center=tuple(center), radius=radius, rate=rate)


def list_a():
    """the first four places and the sixth, which covers no cell"""
    return [source(SIX[k][0], SIX[k][1], RATES[k]) for k in (0, 1, 2, 3, 5)]


def list_b():
    """all six: the fifth covers the whole grid"""
    return [source(c, r, RATES[k]) for k, (c, r) in enumerate(SIX)]


def as_emitter(s):
    """the emitter with a heat source's support (centre, radius): what emitter_ref's exponent / support / near_threshold take"""
    return er.emitter(s["center"], s["radius"])


def near_threshold(dims, sources):
    return er.near_threshold(dims, [as_emitter(s) for s in sources])


def supports(dims, sources):
    """cells inside at least one source's support"""
    X, Y, Z = dims
    m = np.zeros((Z, Y, X), bool)
    for s in sources:
        m |= er.support(dims, as_emitter(s))
    return m


def lerp(a, b, f):
    return fma(f, b - a, a)


def addr_tap(i, n, address):
    """D3D addressing of integer taps: clamp, or mirror with period 2n"""
    if address == "mirror":
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    return np.clip(i, 0, n - 1)


def cell_centres(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return ((x.astype(f32) + f32(0.5)) / f32(X), (y.astype(f32) + f32(0.5)) / f32(Y), (z.astype(f32) + f32(0.5)) / f32(Z))


def sample(T, u0, dt, address):
    """rule 1: the temperature at the back-traced place of every cell, k_advect's trace and colour sampler"""
    Z, Y, X = T.shape
    dt = f32(dt)
    p = cell_centres((X, Y, Z))
    idx, frac = [], []
    for a, n in enumerate((X, Y, Z)):
        t = fma(-u0[a].astype(f32), dt, p[a]) * f32(n) - f32(0.5)
        fl = np.floor(t)
        frac.append((t - fl).astype(f32))
        i0 = fl.astype(np.int64)
        idx.append((addr_tap(i0, n, address), addr_tap(i0 + 1, n, address)))
    (x0, x1), (y0, y1), (z0, z1) = idx
    fx_, fy_, fz_ = frac

    def plane(zi):
        return lerp(lerp(T[zi, y0, x0], T[zi, y0, x1], fx_), lerp(T[zi, y1, x0], T[zi, y1, x1], fx_), fy_)
    return lerp(plane(z0), plane(z1), fz_)          # (a 2-D grid: z0 = z1 = 0, the z lerp runs on equal operands)


def axes(dims, up):
    """the axes the force acts on: up[a] != 0, and never z on a 2-D grid"""
    return [a for a in range(3) if f32(up[a]) != 0 and (a < 2 or dims[2] > 1)]


def apply(T, vel0, vel1, col, prm, sources, dt, address="clamp", half=False, solid=None):
    """the pass: (temperature, VELOCITY1) behind it.  half: velocity and colour are fp16-stored -- vel0 / vel1 / col must hold
    fp16-representable values; every stored velocity component is rounded once (RNE).  The temperature is fp32 either way."""
    Z, Y, X = T.shape
    dims = (X, Y, Z)
    dt = f32(dt)
    Ta, weight, lift, cooling = f32(prm["ambient"]), f32(prm["density_weight"]), f32(prm["lift"]), f32(prm["cooling"])
    Ts = sample(T.astype(f32), vel0, dt, address)
    keep = np.maximum(fma(-dt, cooling, f32(1.0)), f32(0.0))
    T1 = fma(Ts - Ta, keep, Ta)
    for s in sources:
        ex = er.exponent(dims, as_emitter(s))[0]
        with np.errstate(over="ignore", invalid="ignore"):
            basis = np.exp2(ex.astype(f64)).astype(f32)
            m = basis >= er.THRESHOLD
        T1 = np.where(m, fma(np.where(m, basis, f32(0)) * dt, f32(s["rate"]), T1), T1)
    if solid is None:
        solid = np.zeros((Z, Y, X), bool)
    solid = np.asarray(solid) != 0
    T1 = np.where(solid, Ta, T1).astype(f32)
    rho = col[..., 3].astype(f32)
    sc = fma(lift, T1 - Ta, -(weight * rho))
    out = vel1.astype(f32).copy()
    for a in axes(dims, prm["up"]):
        new = fma(f32(prm["up"][a]) * sc, dt, vel1[a].astype(f32))
        if half:
            new = new.astype(np.float16).astype(f32)
        out[a] = np.where(solid, vel1[a], new)
    return T1, out


def apply_loops(T, vel0, vel1, col, prm, sources, dt, address="clamp", solid=None):
    """the same, cell by cell in plain loops (fp32 storage): what tests/test_buoyancy_ref.py holds `apply` against"""
    Z, Y, X = T.shape
    N = (X, Y, Z)
    dt = f32(dt)
    Ta, weight, lift, cooling = f32(prm["ambient"]), f32(prm["density_weight"]), f32(prm["lift"]), f32(prm["cooling"])
    up = [f32(v) for v in prm["up"]]
    To, vo = np.empty((Z, Y, X), f32), vel1.copy()

    def tap(i, n):
        if address == "mirror":
            m = i % (2 * n)
            return m if m < n else 2 * n - 1 - m
        return min(max(i, 0), n - 1)

    def lp(a, b, f):
        return fma(f, f32(b) - f32(a), a)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                cell = (x, y, z)
                p = [(f32(cell[a]) + f32(0.5)) / f32(N[a]) for a in range(3)]
                i0, i1, fr = [], [], []
                for a in range(3):
                    t = f32(fma(-vel0[a, z, y, x], dt, p[a])) * f32(N[a]) - f32(0.5)
                    fl = np.floor(t)
                    fr.append(f32(t - fl))
                    i0.append(tap(int(fl), N[a]))
                    i1.append(tap(int(fl) + 1, N[a]))
                c = []
                for zi in (i0[2], i1[2]):
                    lo = lp(T[zi, i0[1], i0[0]], T[zi, i0[1], i1[0]], fr[0])
                    hi = lp(T[zi, i1[1], i0[0]], T[zi, i1[1], i1[0]], fr[0])
                    c.append(lp(lo, hi, fr[1]))
                Ts = lp(c[0], c[1], fr[2])
                T1 = fma(f32(Ts) - Ta, max(fma(-dt, cooling, f32(1.0)), f32(0.0)), Ta)
                for s in sources:
                    dx, dy = p[0] - f32(s["center"][0]), p[1] - f32(s["center"][1])
                    dz = p[2] - f32(s["center"][2]) if Z > 1 else f32(0)
                    d2 = fma(dz, dz, fma(dy, dy, dx * dx))
                    r = f32(s["radius"])
                    basis = f32(2.0 ** float(((d2 * f32(-4.0)) / (r * r)) * er.LOG2E))
                    if basis >= er.THRESHOLD:
                        T1 = fma(basis * dt, f32(s["rate"]), T1)
                if solid is not None and solid[z, y, x]:
                    To[z, y, x] = Ta
                    continue
                To[z, y, x] = T1
                sc = fma(lift, f32(T1) - Ta, -(weight * col[z, y, x, 3]))
                for a in range(3):
                    if up[a] != 0 and (a < 2 or Z > 1):
                        vo[a, z, y, x] = fma(up[a] * f32(sc), dt, vo[a, z, y, x])
    return To, vo
