"""numpy model of the particle trail (include/fluidx_hip.h fx_set_particle_trail / fx_deposit_particles / fx_particle_density,
fluidx12_amd/csrc/fx_particle_trail.hip: k_trail_splat, k_trail_apply).

The rule, fp32, every operation rounded as written; N = (X, Y, Z), c = particle_ref.c01:
  scatter  a record deposits iff age >= 0 (-0.0 is live, a NaN is dead).  Per axis a of a live record: s = c(p_a), t = s * N_a - 0.5, fl = floor(t),
           f = t - fl, q = (int)rint(f * 256) in 0 .. 256; taps (int)fl and (int)fl + 1 clamped to [0, N_a - 1], weights 256 - q and q.  A 2-D
           grid does not look at z: one tap, plane 0, weight 256.  acc[cell] += w_x * w_y * w_z for each tap combination, in uint64: 2^24 per
           live record in total, two taps that clamp onto one wall cell both adding to it
  apply    for a cell with acc != 0 that is not solid: A = (float)acc * 2^-24 (one round-to-nearest-even conversion of the integer),
           g = rate * dt, colour_ch = fma(A, tint_ch * g, colour_ch); with a temperature and heat != 0, T = fma(A, heat * dt, T).
           fp16 storage rounds the result once.  Every other cell keeps its bits.
The scatter is integers, the apply has no transcendental: the GPU tests compare bit for bit.  `density` / `apply` are vectorised (np.add.at on
uint64), `density_loops` / `apply_loops` their plain-loop twins in Python integers (tests/test_particle_trail_ref.py holds one against the other).

Layouts as Fluid.upload / download: colour float32[Z][Y][X][4], temperature and masks [Z][Y][X]; records float32[n][4]; the volume uint64[Z][Y][X]."""
import numpy as np

import particle_ref as pr
import particle_sort_ref as ps
from fma_ref import fma

f32 = np.float32
ONE = 1 << 24                                                    # what one live record adds

SHAPES = list(pr.SHAPES)
COUNTS = list(pr.COUNTS)                                         # 257 and 4099: a wave edge and a workgroup edge inside runs

DEFAULTS = dict(rate=0.0, tint=(0.0, 0.0, 0.0, 0.0), heat=0.0)


def trail(**kw):
    t = dict(DEFAULTS)
    t.update(kw)
    return t


def live_of(rec):
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(rec, f32).reshape(-1, 4)[:, 3] >= 0


def axis(pa, n):
    """-> (tap 0, tap 1, weight 0, weight 1) of every coordinate on an axis of n cells"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = pr.c01(pa)
        t = (s * f32(n) - f32(0.5)).astype(f32)
        fl = np.floor(t)
        f = (t - fl).astype(f32)
        q = np.rint((f * f32(256)).astype(f32)).astype(np.int64)
    i0 = fl.astype(np.int64)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), 256 - q, q


def base_cell(rec, dims):
    """(int)fl per axis (a 2-D grid: 0 for z): the triple that decides which lanes the kernel merges"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    out = np.zeros((len(rec), 3), np.int64)
    for a in range(3 if dims[2] > 1 else 2):
        out[:, a] = np.floor((pr.c01(rec[:, a]) * f32(dims[a]) - f32(0.5)).astype(f32)).astype(np.int64)
    return out


def density(rec, dims):
    """the accumulator volume behind the scatter: uint64 [Z][Y][X]"""
    X, Y, Z = dims
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    p = rec[live_of(rec)]
    acc = np.zeros(X * Y * Z, np.uint64)
    tx = axis(p[:, 0], X)
    ty = axis(p[:, 1], Y)
    if Z > 1:
        tz = axis(p[:, 2], Z)
    else:
        zero = np.zeros(len(p), np.int64)
        tz = (zero, zero, zero + 256, zero)
    for k in range(2 if Z > 1 else 1):
        for j in range(2):
            for i in range(2):
                w = tx[2 + i] * ty[2 + j] * tz[2 + k]
                np.add.at(acc, (tz[k] * Y + ty[j]) * X + tx[i], w.astype(np.uint64))
    return acc.reshape(Z, Y, X)


def amount(acc):
    """A = (float)acc * 2^-24"""
    return (np.asarray(acc, np.uint64).astype(f32) * f32(2.0 ** -24)).astype(f32)


def apply(acc, col, dt, t, temp=None, solid=None, half=False):
    """the apply pass on the colour (and the temperature, if one is given) as stored -> (colour, temperature or None)"""
    acc = np.asarray(acc, np.uint64)
    col = np.ascontiguousarray(col, f32)
    hit = acc != 0
    if solid is not None:
        hit &= np.asarray(solid) == 0
    A = amount(acc)
    dt = f32(dt)
    g = f32(f32(t["rate"]) * dt)
    out = col.copy()
    for ch in range(4):
        v = fma(A, f32(f32(t["tint"][ch]) * g), col[..., ch])
        if half:
            with np.errstate(over="ignore"):
                v = v.astype(np.float16).astype(f32)
        out[..., ch] = np.where(hit, v, col[..., ch])
    tout = None
    if temp is not None:
        temp = np.ascontiguousarray(temp, f32)
        tout = temp.copy()
        if f32(t["heat"]) != 0:
            tout = np.where(hit, fma(A, f32(f32(t["heat"]) * dt), temp), temp).astype(f32)
    return out, tout


# ---- the same in plain loops, on Python integers ---------------------------------------------------------------------------------------------
def density_loops(rec, dims):
    X, Y, Z = dims
    acc = [0] * (X * Y * Z)
    for x, y, z, age in np.ascontiguousarray(rec, f32).reshape(-1, 4):
        if not age >= 0:
            continue
        taps = []
        for a, (v, n) in enumerate(((x, X), (y, Y), (z, Z))):
            if a == 2 and Z == 1:                                     # a 2-D grid does not look at z
                taps.append(((0, 256),))
                continue
            t = f32(pr._c(v) * f32(n)) - f32(0.5)
            fl = np.floor(t)
            q = int(np.rint(f32(f32(t - fl) * f32(256))))
            i0 = int(fl)
            taps.append(((min(max(i0, 0), n - 1), 256 - q), (min(max(i0 + 1, 0), n - 1), q)))
        for cz, wz in taps[2]:
            for cy, wy in taps[1]:
                for cx, wx in taps[0]:
                    acc[(cz * Y + cy) * X + cx] += wx * wy * wz
    return np.array(acc, np.uint64).reshape(Z, Y, X)


def to_f32_rne(v):
    """a non-negative Python integer rounded to float32, to nearest, ties to even, in integer arithmetic"""
    v = int(v)
    n = v.bit_length()
    if n <= 24:
        return f32(v)
    sh = n - 24
    m, rest, half_ = v >> sh, v & ((1 << sh) - 1), 1 << (sh - 1)
    if rest > half_ or (rest == half_ and (m & 1)):
        m += 1
    return f32(np.ldexp(np.float64(m), sh))                       # (m <= 2^24: exact in float64 and in float32)


def apply_loops(acc, col, dt, t, temp=None, solid=None, half=False):
    acc = np.asarray(acc, np.uint64)
    out = np.ascontiguousarray(col, f32).copy()
    tout = None if temp is None else np.ascontiguousarray(temp, f32).copy()
    dt = f32(dt)
    g = f32(f32(t["rate"]) * dt)
    for idx in np.ndindex(acc.shape):
        if acc[idx] == 0 or (solid is not None and solid[idx]):
            continue
        A = f32(to_f32_rne(acc[idx]) * f32(2.0 ** -24))
        for ch in range(4):
            v = fma(A, f32(f32(t["tint"][ch]) * g), out[idx + (ch,)])
            out[idx + (ch,)] = f32(np.float16(v)) if half else v
        if tout is not None and f32(t["heat"]) != 0:
            tout[idx] = fma(A, f32(f32(t["heat"]) * dt), tout[idx])
    return out, tout


# ---- the sets the tests scatter ------------------------------------------------------------------------------------------------------------
ARRANGEMENTS = ("random", "sorted", "one_point", "one_cell", "two_cells", "dead5", "edges")


def in_cell(dims, cell, frac):
    """positions whose base cell (the (int)fl triple) is `cell`: t = cell + frac per axis, frac in (0, 1)"""
    return np.stack([((cell[a] + 0.5 + frac[:, a]) / dims[a]).astype(f32) for a in range(3)], axis=1)


def arrangement(name, dims, n, seed=0):
    """n records of the arrangement `name` (float32 (n, 4))"""
    rng = np.random.default_rng(4200 + seed)
    rec = np.empty((n, 4), f32)
    rec[:, :3] = rng.random((n, 3)).astype(f32)
    rec[:, 3] = rng.random(n).astype(f32)
    frac = (0.02 + 0.96 * rng.random((n, 3)))
    mid = [max(d // 2 - 1, 0) for d in dims]
    if name == "random":
        return rec
    if name == "sorted":                                                 # the same set in cell order: long runs
        return ps.sort(rec, dims)[0].copy()
    if name == "one_point":                                              # a nozzle: every adder on the same eight words
        rec[:, :3] = rec[0, :3]
    elif name == "one_cell":                                             # one base cell, random fractions: one run per wave, 64-bit sums
        rec[:, :3] = in_cell(dims, mid, frac)
    elif name == "two_cells":                                            # two base cells alternating: every run has length 1
        other = [min(m + 2, d - 1) for m, d in zip(mid, dims)]
        rec[:, :3] = np.where((np.arange(n) % 2 == 0)[:, None], in_cell(dims, mid, frac), in_cell(dims, other, frac))
    elif name == "dead5":                                                # every fifth record dead, by a negative age and a NaN one in turn
        rec = pr.records(dims, n, 4300 + seed)
    elif name == "edges":                                                # the edge positions, live (-0.0 among the ages), as often as they fit
        e = pr.edge_points(dims)
        rec[:, :3] = e[np.arange(n) % len(e)]
        rec[::7, 3] = f32(-0.0)
    else:
        raise ValueError(name)
    return rec


def fields(dims, seed, half=False):
    """a random colour and temperature with -0 in every other cell of the colour's alpha and of the temperature"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    temp = (rng.standard_normal((Z, Y, X)) * 3).astype(f32)
    odd = (np.add.outer(np.add.outer(np.arange(Z), np.arange(Y)), np.arange(X)) % 2) == 1
    col[odd, 3] = f32(-0.0)
    temp[odd] = f32(-0.0)
    if half:
        col = col.astype(np.float16).astype(f32)
    return col, temp
