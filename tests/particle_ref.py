"""numpy model of the tracer particles and the point query (include/fluidx_hip.h fx_set_particles / fx_sample_velocity,
fluidx12_amd/csrc/fx_particles.hip: k_move_particles, k_sample_velocity).

The rule in fp32, operation by operation, as the header states it; it has no transcendental, so the GPU tests compare bit for bit, every
record.  (A fused multiply-add is fmaf's, correctly rounded: tests/fma_ref.py; the sampler is buoyancy_ref's lerp over clamped taps.)
`sample` / `move` are vectorised over the records, `sample_loops` / `move_loops` are their plain-loop twins (tests/test_particle_ref.py
holds the one against the other).

Layouts as Fluid.upload / download: velocity float32[3][Z][Y][X], masks [Z][Y][X]; records float32[n][4] = (x, y, z, age), points [n][3 or 4].
fp16 storage: the model takes the velocity as stored (fp16-representable values); nothing else of the rule depends on the storage."""
import numpy as np

import buoyancy_ref as br
from fma_ref import fma

f32 = np.float32
EULER, MIDPOINT = 0, 1
X_LO, X_HI, Y_LO, Y_HI, Z_LO, Z_HI = 1, 2, 4, 8, 16, 32          # FX_WALL_*

DEFAULTS = dict(scheme=MIDPOINT, drift=(0.0, 0.0, 0.0), lifetime=0.0)

# the grids and counts of the GPU tests: rows that are no multiple of a wave, thin z, 2-D, a wide row; a single record, one past a
# workgroup, a ragged tail
SHAPES = [(20, 20, 12), (70, 70, 5), (36, 36, 1), (256, 256, 6)]
COUNTS = [1, 257, 4099]


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def c01(v):
    """c(v) = fminf(fmaxf(v, 0), 1): a NaN becomes 0, -0 becomes +0"""
    with np.errstate(invalid="ignore"):
        return (np.fmin(np.fmax(np.asarray(v, f32), f32(0)), f32(1)) + f32(0)).astype(f32)


def edge_values(n):
    """the coordinates every test plants on an axis of n cells: the walls, -0, the first and last cell centres, a cell centre and a cell
    face inside, places beyond both walls, and what no caller should write but may"""
    return np.array([0.0, 1.0, -0.0, 0.5 / n, 1 - 0.5 / n, (n // 2 + 0.5) / n, (n // 2) / n, -0.3, 1.7, np.inf, -np.inf, np.nan, 1e30], f32)


def edge_points(dims):
    """every edge value on every axis, the other two axes at edge values picked in turn: a few dozen points"""
    ev = [edge_values(n) for n in dims]
    pts = []
    for a in range(3):
        for k, v in enumerate(ev[a]):
            p = [ev[b][(k + 1 + b) % len(ev[b])] for b in range(3)]
            p[a] = v
            pts.append(p)
    return np.array(pts, f32)


def points(dims, n, seed):
    """n points: the edge set first (as much of it as fits), random ones in [0,1]^3 behind it"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)).astype(f32)
    e = edge_points(dims)[:n]
    p[:len(e)] = e
    return p


def time_step(dims):
    return f32((2.0 if dims[2] > 1 else 1.0) / dims[1])       # Fluid.default_time_step


def velocity(dims, seed, cells=1.5, dt=None, half=False):
    """a random velocity that carries a particle about `cells` cells (standard deviation) per step along every axis"""
    rng = np.random.default_rng(seed)
    dt = float(time_step(dims) if dt is None else dt)
    v = rng.standard_normal((3, dims[2], dims[1], dims[0]))
    for a, n in enumerate(dims):
        v[a] *= cells / (dt * n)
    v = v.astype(f32)
    return v.astype(np.float16).astype(f32) if half else v


def records(dims, n, seed, dead_every=5):
    """n records: the positions of `points`, ages in [0, 1), every fifth one dead on entry -- by a negative age and by a NaN one in turn"""
    rng = np.random.default_rng(seed + 1)
    rec = np.empty((n, 4), f32)
    rec[:, :3] = points(dims, n, seed)
    rec[:, 3] = rng.random(n).astype(f32)
    dead = np.arange(n) % dead_every == dead_every - 1
    rec[dead, 3] = np.where(np.arange(dead.sum()) % 2 == 0, f32(-1), f32(np.nan))
    return rec


def box_mask(dims):
    """a solid box about the centre, at least one cell thick"""
    X, Y, Z = dims
    m = np.zeros((Z, Y, X), np.uint8)
    m[Z // 4:max(3 * Z // 4, Z // 4 + 1), Y // 3:2 * Y // 3, X // 3:2 * X // 3] = 1
    return m


def axis_taps(pa, n):
    with np.errstate(invalid="ignore", over="ignore"):
        s = c01(pa)
        t = (s * f32(n) - f32(0.5)).astype(f32)
        fl = np.floor(t)
        f = (t - fl).astype(f32)
    i0 = fl.astype(np.int64)
    return f, br.addr_tap(i0, n, "clamp"), br.addr_tap(i0 + 1, n, "clamp")


def sample(vel, pts):
    """U(p) for every row of pts (columns beyond the third are ignored) -> float32 (n, 3)"""
    _, Z, Y, X = vel.shape
    pts = np.asarray(pts, f32)
    fx_, x0, x1 = axis_taps(pts[:, 0], X)
    fy_, y0, y1 = axis_taps(pts[:, 1], Y)
    fz_, z0, z1 = axis_taps(pts[:, 2], Z)
    out = np.empty((pts.shape[0], 3), f32)
    for a in range(3):
        T = vel[a].astype(f32)

        def plane(zi):
            return br.lerp(br.lerp(T[zi, y0, x0], T[zi, y0, x1], fx_), br.lerp(T[zi, y1, x0], T[zi, y1, x1], fx_), fy_)
        out[:, a] = br.lerp(plane(z0), plane(z1), fz_)            # (a 2-D grid: z0 = z1 = 0, the z lerp runs on equal operands)
    return out


def move(rec, vel, dt, prm=None, faces=0, solid=None):
    """one step of every live record -> the records behind it"""
    prm = params() if prm is None else prm
    _, Z, Y, X = vel.shape
    N = (X, Y, Z)
    axes = 3 if Z > 1 else 2                                       # a 2-D grid leaves z alone altogether
    rec = np.ascontiguousarray(rec, f32)
    out = rec.copy()
    with np.errstate(invalid="ignore"):
        live = rec[:, 3] >= 0
    if not live.any():
        return out
    dt = f32(dt)
    drift = np.array(prm["drift"], f32)
    lifetime = f32(prm["lifetime"])
    p, age = rec[live, :3], rec[live, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        k = (sample(vel, p) + drift).astype(f32)
        if prm["scheme"] == MIDPOINT:
            m = c01(fma(k, f32(0.5) * dt, p))
            k = (sample(vel, m) + drift).astype(f32)
        q = np.array(fma(k, dt, p), f32)
        q[:, axes:] = p[:, axes:]
        dead = np.zeros(len(q), bool)
        for a in range(axes):
            dead |= (q[:, a] < 0) & bool(faces & (1 << (2 * a)))
            dead |= (q[:, a] > 1) & bool(faces & (2 << (2 * a)))
        q[:, :axes] = c01(q[:, :axes])
        if solid is not None:
            cell = [np.minimum((q[:, a] * f32(N[a])).astype(f32).astype(np.int64), N[a] - 1) if a < axes else np.zeros(len(q), np.int64) for a in range(3)]
            hit = np.asarray(solid)[cell[2], cell[1], cell[0]] != 0
            q[hit] = p[hit]
        age1 = (age + dt).astype(f32)
        if lifetime > 0:
            dead |= age1 >= lifetime
    out[live, :3] = q
    out[live, 3] = np.where(dead, f32(-1), age1)
    return out


# ---- the same in plain loops ---------------------------------------------------------------------------------------------------------------
def _c(v):
    v = f32(v)
    if v != v or v <= 0:               # NaN, negative, either zero: +0
        return f32(0)
    return f32(1) if v > 1 else v


def sample_loops(vel, pts):
    _, Z, Y, X = vel.shape
    N = (X, Y, Z)
    out = np.empty((len(pts), 3), f32)

    def lp(a, b, f):
        with np.errstate(invalid="ignore"):
            return fma(f, f32(b) - f32(a), a)
    for n, pt in enumerate(np.asarray(pts, f32)):
        i0, i1, fr = [], [], []
        for a in range(3):
            t = f32(_c(pt[a]) * f32(N[a])) - f32(0.5)
            fl = np.floor(t)
            fr.append(f32(t - fl))
            i0.append(min(max(int(fl), 0), N[a] - 1))
            i1.append(min(max(int(fl) + 1, 0), N[a] - 1))
        for a in range(3):
            T = vel[a]
            c = []
            for zi in (i0[2], i1[2]):
                lo = lp(T[zi, i0[1], i0[0]], T[zi, i0[1], i1[0]], fr[0])
                hi = lp(T[zi, i1[1], i0[0]], T[zi, i1[1], i1[0]], fr[0])
                c.append(lp(lo, hi, fr[1]))
            out[n, a] = lp(c[0], c[1], fr[2])
    return out


def move_loops(rec, vel, dt, prm=None, faces=0, solid=None):
    prm = params() if prm is None else prm
    _, Z, Y, X = vel.shape
    N = (X, Y, Z)
    axes = 3 if Z > 1 else 2
    dt = f32(dt)
    drift = [f32(v) for v in prm["drift"]]
    lifetime = f32(prm["lifetime"])
    out = np.ascontiguousarray(rec, f32).copy()
    for n in range(len(out)):
        p, age = out[n, :3].copy(), out[n, 3]
        if not age >= 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            u = sample_loops(vel, p[None])[0]
            k = [f32(u[a] + drift[a]) for a in range(3)]
            if prm["scheme"] == MIDPOINT:
                h = f32(f32(0.5) * dt)
                m = np.array([_c(fma(k[a], h, p[a])) for a in range(3)], f32)
                u = sample_loops(vel, m[None])[0]
                k = [f32(u[a] + drift[a]) for a in range(3)]
            q = [f32(fma(k[a], dt, p[a])) if a < axes else p[a] for a in range(3)]
            dead = False
            for a in range(axes):
                if (q[a] < 0 and faces & (1 << (2 * a))) or (q[a] > 1 and faces & (2 << (2 * a))):
                    dead = True
                q[a] = _c(q[a])
            if solid is not None:
                cell = [min(int(f32(q[a] * f32(N[a]))), N[a] - 1) if a < axes else 0 for a in range(3)]
                if solid[cell[2], cell[1], cell[0]]:
                    q = list(p)
            age1 = f32(age + dt)
        if lifetime > 0 and age1 >= lifetime:
            dead = True
        out[n, 0], out[n, 1], out[n, 2] = q
        out[n, 3] = f32(-1) if dead else age1
    return out


# ---- the property the midpoint scheme is there for ---------------------------------------------------------------------------------------
def rotation_field(dims, omega):
    """a rigid rotation about the box's centre in texture space, sampled at the cell centres: u = omega x (p - c) about the z axis"""
    X, Y, Z = dims
    px, py, _ = br.cell_centres(dims)
    vel = np.zeros((3, Z, Y, X), f32)
    vel[0] = (-f32(omega) * (py - f32(0.5))).astype(f32)
    vel[1] = (f32(omega) * (px - f32(0.5))).astype(f32)
    return vel


def radius_error(scheme, dims=(32, 32, 1), omega_dt=0.1, dt=1 / 64, count=64, steps=50, radius=0.25):
    """the largest relative radius error of `count` particles on a circle about the centre behind `steps` steps of the rotation"""
    vel = rotation_field(dims, omega_dt / dt)
    ang = np.arange(count) * (2 * np.pi / count)
    rec = np.zeros((count, 4), f32)
    rec[:, 0], rec[:, 1], rec[:, 2] = 0.5 + radius * np.cos(ang), 0.5 + radius * np.sin(ang), 0.5
    for _ in range(steps):
        rec = move(rec, vel, dt, params(scheme=scheme))
    r = np.hypot(rec[:, 0].astype(np.float64) - 0.5, rec[:, 1].astype(np.float64) - 0.5)
    return float(np.abs(r / radius - 1).max())
