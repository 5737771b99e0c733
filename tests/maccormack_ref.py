"""numpy model of the MacCormack advection (include/fluidx_hip.h fx_set_advection_scheme, fluidx12_amd/csrc/fx_maccormack.hip: k_mc_predict,
k_mc_correct).

Rules 1-5 of the header comment in fp32, operation by operation, with the conventions of tests/buoyancy_ref.py and tests/emitter_ref.py: `fma`
(tests/fma_ref.py: fmaf, correctly rounded), `lerp`, `addr_tap`, `cell_centres` and `sample` (k_advect's trace and colour sampler) are theirs, and the built-in impulse is emitter_ref's
BUILTIN_3D / BUILTIN_2D emitter, whose basis is evaluated in float64 and rounded once.  So the tests compare
  * outside the built-in ball's support (everywhere with the impulse off): bit for bit, velocity and colour, and
  * inside: rel-L2 < 1e-6, the project's figure for exp2 in fp32 against float64 (tests/test_gpu_emitters.py).
`limit=False` leaves the limiter of rule 4 out: the unlimited scheme exists here only, to show what the limiter does (tests/test_maccormack_ref.py).

Layouts as Fluid.upload / download: velocity float32[3][Z][Y][X], colour float32[Z][Y][X][4]."""
import numpy as np

import buoyancy_ref as br
import emitter_ref as er
from fma_ref import fma

f32, f64 = np.float32, np.float64
lerp, addr_tap, cell_centres, sample = br.lerp, br.addr_tap, br.cell_centres, br.sample


def back_taps(q, u0, dt, address):
    """rule 1: the eight taps of every cell's back-trace in the order 000, 100, 010, 110, 001, 101, 011, 111 (x fastest)"""
    Z, Y, X = q.shape
    p = cell_centres((X, Y, Z))
    idx = []
    for a, n in enumerate((X, Y, Z)):
        t = fma(-u0[a].astype(f32), f32(dt), p[a]) * f32(n) - f32(0.5)
        i0 = np.floor(t).astype(np.int64)
        idx.append((addr_tap(i0, n, address), addr_tap(i0 + 1, n, address)))
    return [q[zi, yi, xi] for zi in idx[2] for yi in idx[1] for xi in idx[0]]


def bounds(taps):
    """rule 1: lo / hi over the taps in order, starting at the first, by selects (the earlier of +0 / -0 stays, a NaN never replaces a bound)"""
    lo, hi = taps[0], taps[0]
    with np.errstate(invalid="ignore"):
        for v in taps:
            lo = np.where(v < lo, v, lo)
            hi = np.where(v > hi, v, hi)
    return lo, hi


def advect_field(q, u0, dt, address="clamp", limit=True):
    """rules 1-4 for one quantity q float32[Z][Y][X] traced with u0 float32[3][Z][Y][X]"""
    q = q.astype(f32)
    neg = [-u0[a].astype(f32) for a in range(3)]
    hat = sample(q, u0, dt, address)                              # rules 1, 2
    bar = sample(hat, neg, dt, address)                           # rule 3: fma(-(-u0), dt, p) = fma(u0, dt, p)
    r = fma(f32(0.5), q - bar, hat)                               # rule 4
    if limit:
        lo, hi = bounds(back_taps(q, u0, dt, address))
        with np.errstate(invalid="ignore"):
            r = np.where(r < lo, lo, np.where(r > hi, hi, r))
    return r.astype(f32)


def semi_lagrangian_field(q, u0, dt, address="clamp"):
    """the first-order scheme on the same terms (rule 1's hat_q alone): what the MacCormack results are held against"""
    return sample(q.astype(f32), u0, dt, address)


def attenuation(dt):
    return np.maximum(fma(-f32(dt), f32(0.2), f32(1.0)), f32(0.0))


def impulse_support(dims):
    """cells the built-in impulse touches"""
    return er.support(dims, er.BUILTIN_3D if dims[2] > 1 else er.BUILTIN_2D)


def near_threshold(dims):
    return er.near_threshold(dims, [er.BUILTIN_3D if dims[2] > 1 else er.BUILTIN_2D])


def tail(u, c, dt, impulse=True, half=False):
    """rule 5 on r = (u float32[3][Z][Y][X], c float32[Z][Y][X][4]): the built-in impulse, the attenuation, the stores"""
    _, Z, Y, X = u.shape
    if impulse:
        u, c, _ = er.apply(u, c, [er.BUILTIN_3D if Z > 1 else er.BUILTIN_2D], dt)
    at = attenuation(dt)
    vo, co = (u * at).astype(f32), (c * at).astype(f32)
    if half:
        vo, co = vo.astype(np.float16).astype(f32), co.astype(np.float16).astype(f32)
    return vo, co


def corrected(vel0, col, dt, address="clamp", limit=True, scheme="maccormack"):
    """rules 1-4 for all seven quantities: r = (u float32[3][Z][Y][X], c float32[Z][Y][X][4]).  scheme "semi-lagrangian": rule 1's hat alone"""
    adv = (lambda q: advect_field(q, vel0, dt, address, limit)) if scheme == "maccormack" else (lambda q: semi_lagrangian_field(q, vel0, dt, address))
    return np.stack([adv(vel0[a]) for a in range(3)]), np.stack([adv(col[..., i]) for i in range(4)], axis=-1)


def step(vel0, col, dt, address="clamp", impulse=True, half=False, limit=True, scheme="maccormack"):
    """the advection stage: (VELOCITY1, COLOR) behind it.  half: the fields are fp16-stored -- vel0 / col must hold fp16-representable values,
    the scratch is fp32 and every stored value is rounded once (RNE).  scheme "semi-lagrangian": k_advect on the same terms"""
    u, c = corrected(vel0, col, dt, address, limit, scheme)
    return tail(u, c, dt, impulse, half)


def step_loops(vel0, col, dt, address="clamp", limit=True):
    """rules 1-5 with the impulse off, cell by cell in plain loops (fp32 storage): what tests/test_maccormack_ref.py holds `step` against"""
    _, Z, Y, X = vel0.shape
    N = (X, Y, Z)
    dt = f32(dt)
    Q = [vel0[0], vel0[1], vel0[2]] + [col[..., i] for i in range(4)]

    def tap(i, n):
        if address == "mirror":
            m = i % (2 * n)
            return m if m < n else 2 * n - 1 - m
        return min(max(i, 0), n - 1)

    def lp(a, b, f):
        return fma(f, f32(b) - f32(a), a)

    def trace(cell, sign):
        i0, i1, fr = [], [], []
        for a in range(3):
            p = (f32(cell[a]) + f32(0.5)) / f32(N[a])
            t = f32(fma(f32(sign) * vel0[a][cell[2], cell[1], cell[0]], dt, p)) * f32(N[a]) - f32(0.5)
            fl = np.floor(t)
            fr.append(f32(t - fl))
            i0.append(tap(int(fl), N[a]))
            i1.append(tap(int(fl) + 1, N[a]))
        return [(zi, yi, xi) for zi in (i0[2], i1[2]) for yi in (i0[1], i1[1]) for xi in (i0[0], i1[0])], fr

    def tri(v, fr):
        return lp(lp(lp(v[0], v[1], fr[0]), lp(v[2], v[3], fr[0]), fr[1]), lp(lp(v[4], v[5], fr[0]), lp(v[6], v[7], fr[0]), fr[1]), fr[2])
    hat = [np.empty((Z, Y, X), f32) for _ in Q]
    traces = {}
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                traces[x, y, z] = where, fr = trace((x, y, z), -1)
                for k, q in enumerate(Q):
                    hat[k][z, y, x] = tri([q[w] for w in where], fr)
    out = [np.empty((Z, Y, X), f32) for _ in Q]
    at = max(fma(-dt, f32(0.2), f32(1.0)), f32(0.0))
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                where, fr = traces[x, y, z]
                fwd, ff = trace((x, y, z), 1)
                for k, q in enumerate(Q):
                    v = [q[w] for w in where]
                    bar = tri([hat[k][w] for w in fwd], ff)
                    r = fma(f32(0.5), f32(q[z, y, x]) - f32(bar), hat[k][z, y, x])
                    if limit:
                        lo = hi = v[0]
                        for t in v:
                            lo = t if t < lo else lo
                            hi = t if t > hi else hi
                        r = lo if r < lo else (hi if r > hi else r)
                    out[k][z, y, x] = f32(r) * at
    return np.stack(out[:3]), np.stack(out[3:], axis=-1)


# ---- the two demonstrations of the issue's table: a Gaussian blob and a step edge carried by the uniform velocity (0.37, 0.23, 0) for 40 steps of
# 1/60 (7.9 cells in x and 4.9 in y on the 32-cell grid), clamp addressing
CARRY_U, CARRY_STEPS, CARRY_DT = (0.37, 0.23, 0.0), 40, f32(1.0 / 60.0)
CARRY_DIMS = [(32, 32, 8), (48, 48, 1)]


def uniform_velocity(dims, u=CARRY_U):
    X, Y, Z = dims
    return np.stack([np.full((Z, Y, X), f32(v)) for v in u])


def blob(dims, centre=(0.3, 0.35), sigma=0.055):
    """a Gaussian of x and y (the same in every z plane) whose centre lies between cell centres: its peak on the grid is a little below 1"""
    px, py, _ = cell_centres(dims)
    d2 = (px.astype(f64) - centre[0]) ** 2 + (py.astype(f64) - centre[1]) ** 2
    return np.exp(-d2 / (2 * sigma * sigma)).astype(f32)


def edge(dims):
    """1 for x < 0.5, else 0"""
    px, _, _ = cell_centres(dims)
    return (px < f32(0.5)).astype(f32)


def carry(q, dims, scheme, limit=True, steps=CARRY_STEPS):
    """q after `steps` steps of the scheme, no attenuation"""
    u0 = uniform_velocity(dims)
    for _ in range(steps):
        q = advect_field(q, u0, CARRY_DT, "clamp", limit) if scheme == "maccormack" else semi_lagrangian_field(q, u0, CARRY_DT)
    return q
