"""numpy model of the particle spawners (include/fluidx_hip.h fx_set_particle_spawners, fluidx12_amd/csrc/fx_particle_spawn.hip: k_spawn_count,
the scan, k_spawn_tick, k_spawn_place).

The rule as the header states it: unsigned integers that wrap, fp32 with every operation rounded as written (a fused multiply-add is fmaf's:
tests/fma_ref.py).  It has no transcendental and no atomic that decides a position, so the GPU tests compare bit for bit: every record and the
whole of fx_particle_spawn_info.

Records float32[n][4] = (x, y, z, age), masks [Z][Y][X] as Fluid.upload has them; a spawner is a dict with the keys of SPAWNER."""
import numpy as np

from fma_ref import fma

f32, u32, u64 = np.float32, np.uint32, np.uint64
BOX, BALL = 0, 1
MAX_SPAWNERS = 16
BALL_TRIES = 8
AGE_WORD = 24                                   # word(24): the age; words 0 .. 23 are the eight tries of a ball (a box takes 0 .. 2)
RATE_CAP = f32(67108864.0)                      # 2^26 births per spawner and step at the most

SPAWNER = dict(shape=BOX, seed=0, center=(0.5, 0.5, 0.5), half_extent=(0.1, 0.1, 0.1), rate=0.0, age_spread=0.0)


def spawner(base=None, **kw):
    """a spawner: the defaults, or `base`, with the given members replaced"""
    s = dict(SPAWNER if base is None else base)
    s.update(kw)
    return s


def mix(x):
    """the 32-bit finaliser of the rule, on uint32 arrays (or anything that becomes one)"""
    x = np.array(x, dtype=u32, ndmin=1, copy=True)
    x ^= x >> u32(16)
    x *= u32(0x7feb352d)
    x ^= x >> u32(15)
    x *= u32(0x846ca68b)
    x ^= x >> u32(16)
    return x


def word(seed, s, k, d):
    """word(d) of birth k (uint64, array or scalar) of spawner s -> uint32 array of k's shape (at least 1-D)"""
    k = np.array(k, dtype=u64, ndmin=1)
    h0 = mix(u32((int(seed) + 0x9e3779b9 * (int(s) + 1)) & 0xFFFFFFFF))
    h1 = mix(h0 ^ (k & u64(0xFFFFFFFF)).astype(u32))
    h2 = mix(h1 ^ (k >> u64(32)).astype(u32))
    return mix(h2 + u32((0x85ebca6b * (int(d) + 1)) & 0xFFFFFFFF))


def unit(seed, s, k, d):
    """u(d) in [0, 1): the word's upper 24 bits, exact in fp32"""
    return ((word(seed, s, k, d) >> u32(8)).astype(f32) * f32(2.0 ** -24)).astype(f32)


def sym(seed, s, k, d):
    """a(d) = fmaf(2, u(d), -1) in [-1, 1), exact"""
    return np.asarray(fma(f32(2), unit(seed, s, k, d), f32(-1)), f32)


def c01(v):
    with np.errstate(invalid="ignore"):
        return (np.fmin(np.fmax(np.asarray(v, f32), f32(0)), f32(1)) + f32(0)).astype(f32)


def draw(sp, s, k, is3d=True):
    """the offsets (a_x, a_y, a_z) of births k of spawner s, before the scale: float32 (n, 3), and which of them fell back to (0, 0, 0)"""
    k = np.array(k, dtype=u64, ndmin=1)
    n = len(k)
    seed = sp["seed"]
    fell = np.zeros(n, bool)
    if sp["shape"] == BOX:
        a = np.stack([sym(seed, s, k, d) for d in range(3)], axis=1)
        if not is3d:
            a[:, 2] = 0
        return a, fell
    a = np.zeros((n, 3), f32)
    todo = np.ones(n, bool)
    for t in range(BALL_TRIES):
        ax, ay, az = (sym(seed, s, k, 3 * t + d) for d in range(3))
        if not is3d:
            az = np.zeros(n, f32)
        r2 = np.asarray(fma(az, az, fma(ay, ay, (ax * ax).astype(f32))), f32)
        take = todo & (r2 <= f32(1))
        a[take] = np.stack([ax, ay, az], axis=1)[take]
        todo &= ~take
    return a, todo


def records_of(sp, s, k, is3d=True):
    """the records births k of spawner s would store: float32 (n, 4)"""
    a, _ = draw(sp, s, k, is3d)
    k = np.array(k, dtype=u64, ndmin=1)
    out = np.empty((len(k), 4), f32)
    for d in range(3):
        out[:, d] = c01(fma(a[:, d], f32(sp["half_extent"][d]), f32(sp["center"][d])))
    out[:, 3] = (unit(sp["seed"], s, k, AGE_WORD) * f32(sp["age_spread"])).astype(f32)
    return out


def cell_of(p, dims):
    """cell_axis per axis (fx_particle_cell.h), the z cell of a 2-D grid 0 -> (cx, cy, cz) int64 arrays"""
    out = []
    for a in range(3):
        if a == 2 and dims[2] == 1:
            out.append(np.zeros(len(p), np.int64))
        else:
            out.append(np.minimum((p[:, a] * f32(dims[a])).astype(f32).astype(np.int64), dims[a] - 1))
    return out


def new_state(n_spawners):
    """what fx_set_particle_spawners leaves: fractions, serials and the three counters at zero"""
    return dict(acc=[0] * n_spawners, serial=[0] * n_spawners, born=0, dropped=0, blocked=0)


def births(sp, acc, dt):
    """one tick of a spawner's accumulator -> (n_s, the accumulator behind it)"""
    with np.errstate(over="ignore"):
        w = np.fmin(f32(sp["rate"]) * f32(dt), RATE_CAP)
        inc = int(np.rint(f32(w * f32(65536.0))))
    acc = (acc + inc) & 0xFFFFFFFFFFFFFFFF
    return acc >> 16, acc & 0xFFFF


def step(rec, spawners, st, dt, dims, solid=None):
    """one run of the stage: the records behind it (a copy); `st` (new_state) is advanced in place"""
    rec = np.ascontiguousarray(rec, f32)
    out = rec.copy()
    is3d = dims[2] > 1
    with np.errstate(invalid="ignore"):
        dead = np.flatnonzero(~(rec[:, 3] >= 0))
    D = len(dead)
    j0 = 0
    for s, sp in enumerate(spawners):
        n_s, st["acc"][s] = births(sp, st["acc"][s], dt)
        base = st["serial"][s]
        st["serial"][s] = (base + n_s) & 0xFFFFFFFFFFFFFFFF
        lo, hi = min(j0, D), min(j0 + n_s, D)                  # the births of this spawner that find a slot: j in [lo, hi)
        st["dropped"] += n_s - (hi - lo)
        j0 += n_s
        if hi == lo:
            continue
        k = (np.arange(lo - (j0 - n_s), hi - (j0 - n_s), dtype=u64) + u64(base & 0xFFFFFFFFFFFFFFFF))
        r = records_of(sp, s, k, is3d)
        slots = dead[lo:hi]
        if solid is not None:
            cx, cy, cz = cell_of(r, dims)
            hit = np.asarray(solid)[cz, cy, cx] != 0
            st["blocked"] += int(hit.sum())
            slots, r = slots[~hit], r[~hit]
        st["born"] += len(slots)
        out[slots] = r
    return out


def info(st):
    """the state as ParticleSpawnInfo reports it"""
    serial = list(st["serial"]) + [0] * (MAX_SPAWNERS - len(st["serial"]))
    return dict(born=st["born"], dropped=st["dropped"], blocked=st["blocked"], serial=serial)
