"""Input recipes of tests/test_gpu_store_edges.py: the states that drive the optional stages of the step (vorticity confinement, emitters,
buoyancy, obstacles, open walls, MacCormack advection, the multigrid solver -- the kernels behind csrc/fx_store.h) to the edges of their
number formats, with the models' outputs for them.

  part 1  fp16 storage: stores into the binary16 subnormal range, across the overflow boundary (65504 | 65520 -> inf) and of -0
  part 2  fp32 storage: fields of fp32 subnormals

Every recipe follows tests/test_gpu_stage_matrix.py::half_range_state -- magnitudes log-uniform over the binary16 range, clipped to the largest
binary16, random signs, a lattice of +0 and of -0 cells, pressure log-uniform in 2^-30 .. 2^15 -- and returns a Case: the inputs, the model's
output and the cells the stage stores.  tests/test_store_edges.py holds every Case to its conditions on the models alone (no GPU); the GPU
tests assert the same conditions again and then compare bit for bit.  Cases are cached and read-only: the CPU and the GPU tests share them.

Shapes: (70, 70, 5) and (36, 36, 1) are the smallest with an interior, both x edges, a ragged second 64-wide tile and fewer planes than a tile
column, 3-D and 2-D; the kernel families that split by row length add (68, 68, 5) (k_jacobi_bnd_v4: 3-D, X % 4 == 0) and (64, 64, 4)
(k_mg_smooth_v4); (70, 70, 4) is two multigrid levels on the scalar sweep, (20, 20, 8) reaches k_mg_tail, (70, 70, 5) is one level."""
import functools
import types

import numpy as np

import buoyancy_ref as br
import emitter_ref as er
import maccormack_ref as mr
import multigrid_ref as mg
import open_ref as orf
import test_obstacle_ref as ob
import vorticity_ref as vr
from test_gpu_stage_matrix import half_bits, half_classes, log_uniform, subnormal_share

f32 = np.float32
TILE_SHAPES = [(70, 70, 5), (36, 36, 1)]
BND_SHAPES = TILE_SHAPES + [(68, 68, 5)]
MG_SHAPES = [(36, 36, 1), (64, 64, 4), (70, 70, 4), (20, 20, 8), (70, 70, 5)]
BIG = f32(65504.0)                                           # the largest binary16
TINY = 2.0 ** -128                                           # standard_normal * 2^-128: below the smallest normal (2^-126) up to four sigma


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


def time_step(dims):
    return f32((2.0 if dims[2] > 1 else 1.0) / dims[1])       # Fluid.default_time_step


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def to_half(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


def case(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)                          # shared among tests: nobody changes a reference
    return types.SimpleNamespace(**kw)


def seed_of(dims, k):
    return 7000 + 97 * k + dims[0] + 7 * dims[2]


# ---- the states ---------------------------------------------------------------------------------------------------------------------------
def half_field(rng, shape, lo=-27, hi=16, ends=0.0):
    """binary16 values as float32: magnitudes log-uniform in 2^lo .. 2^hi clipped to 65504, random signs.  `ends`: that share of the cells
    is drawn from the two ends of the range instead -- half of it from 2^-27 .. 2^-14 (the subnormals and what rounds to +-0), half from
    2^14 .. 2^16 (within a factor of four of the overflow boundary)"""
    v = log_uniform(rng, shape, lo, hi)
    if ends:
        pick = rng.random(shape)
        v = np.where(pick < ends / 2, log_uniform(rng, shape, -27, -14), np.where(pick < ends, log_uniform(rng, shape, 14, 16), v))
    return to_half(np.clip(v, -BIG, BIG))


def zero_lattice(a, negative=True):
    """a lattice of +0 cells and, on the odd planes / rows, of -0 cells (half_range_state's, on any leading layout [.., Z, Y, X])"""
    a[..., ::2, ::3, ::5] = 0.0
    if negative:
        if a.shape[-3] > 1:
            a[..., 1::2, ::3, ::5] = -0.0
        else:
            a[..., :, 1::3, ::5] = -0.0
    return a


def half_state(dims, k, vel=(-27, 16), ends=0.0, colour_negzero=True):
    """(velocity [3][Z][Y][X], colour [Z][Y][X][4], pressure [Z][Y][X]): velocity and colour hold binary16 values over the whole range with
    the zero lattices, the pressure is fp32, log-uniform in 2^-30 .. 2^15"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed_of(dims, k))
    v = zero_lattice(half_field(rng, (3, Z, Y, X), vel[0], vel[1], ends))
    c = np.moveaxis(zero_lattice(half_field(rng, (4, Z, Y, X), -27, 16, ends), colour_negzero), 0, -1).copy()
    if not colour_negzero:
        c[c == 0] = 0.0                                      # (the magnitudes below 2^-25 round to a zero of either sign)
    p = log_uniform(rng, (Z, Y, X), -30, 15)
    return v, c, p


def crossing_velocity(dims, k, cells=1.2, half=False):
    """a tracing velocity whose back-traces move `cells` cells (standard deviation) along every axis: some leave the box by less than a
    cell, some by more (tests/test_gpu_open_walls.py trace_state)"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed_of(dims, k))
    dt = time_step(dims)
    v = rng.standard_normal((3, Z, Y, X))
    for a, n in enumerate(dims):
        v[a] *= cells / (float(dt) * n)
    v = v.astype(f32)
    return to_half(v) if half else v


def subnormal_field(dims, k, lead=(), scale=TINY):
    X, Y, Z = dims
    return (np.random.default_rng(seed_of(dims, k)).standard_normal(tuple(lead) + (Z, Y, X)) * scale).astype(f32)


def mask_of(dims):
    return ob.random_mask(dims, seed=31, p=0.25)


def shares(h):
    """(subnormal, inf, -0, NaN) shares of binary16 bit patterns, as floats"""
    return tuple(float(v) for v in half_classes(np.asarray(h)))


def edge_conditions(what, h, overflow, subnormal=True, negzero=True):
    """the conditions of tests/test_gpu_stage_matrix.py::assert_the_edges_are_reached, with its bounds, on binary16 bit patterns of a MODEL's
    output, as (what, value, relation, bound): subnormal share >= 0.02, -0 share >= 2e-4, no NaN, inf share >= 2e-4 where the stage can
    overflow and exactly 0 where it cannot.  subnormal / negzero = False: this case is not the one that has to reach that range"""
    sub, inf, nz, nan = shares(h)
    out = [(what + ": NaN share", nan, "==", 0.0)]
    if subnormal:
        out.append((what + ": subnormal share", sub, ">=", 0.02))
    if negzero:
        out.append((what + ": -0 share", nz, ">=", 2e-4))
    out.append((what + ": inf share", inf, ">=", 2e-4) if overflow else (what + ": inf share", inf, "==", 0.0))
    return out


def assert_conditions(c):
    """conditions on the reference, not measurements of the kernels: if a recipe misses them, the recipe is wrong"""
    for what, value, rel, bound in c.conditions:
        print("%s %.5g (%s %g)" % (what, value, rel, bound))
    for what, value, rel, bound in c.conditions:
        assert {">=": value >= bound, ">": value > bound, "==": value == bound}[rel], (what, value, rel, bound)


def stored_bits(c):
    """the binary16 bit patterns of the values a part-1 case's stage stores, of the model (c.want) -- and of `got`, the same selection"""
    return half_bits(c.want[c.stored])


# ---- part 1: binary16 edges ---------------------------------------------------------------------------------------------------------------
VORTICITY_HALF = [(1e-3, False), (8.0, True)]                # (epsilon, can overflow): the first reaches the subnormals and -0, the second inf
VORT_ENDS = {1e-3: 0.0, 8.0: 0.5}


@functools.lru_cache(maxsize=None)
def vorticity_half(dims, eps):
    vel, _, _ = half_state(dims, 1, ends=VORT_ENDS[eps])
    vel[:, :, 8:13, 8:13] = -0.0                             # a patch at rest: w = g = 0 inside, the force is +0 - +0 = +0 and every -0 comes back +0
    dt = time_step(dims)
    want = vr.confine_stored(vel, eps, dt, True)
    stored = np.ones(vel.shape, bool)
    if dims[2] == 1:
        stored[2] = False                                    # 2-D: uz is copied
    first = eps == VORTICITY_HALF[0][0]
    cond = edge_conditions("vorticity %s eps %g" % (dims, eps), half_bits(want[stored]), dict(VORTICITY_HALF)[eps], subnormal=first, negzero=first)
    flipped = stored & (bits(vel) == 0x80000000) & (bits(want) == 0)
    cond.append(("vorticity %s eps %g: -0 inputs that a force of +0 turns into +0" % (dims, eps), float(flipped.sum()), ">=", 18.0))
    return case(vel=vel, dt=dt, eps=eps, want=want, stored=stored, conditions=cond)


def emitters_exact(dims):
    """two overlapping balls whose stored bits do not depend on the last bits of exp2: force = 0 and swirl != 0 make the force dz * -swirl
    and dx * swirl exactly (fma(basis, 0, x) = x), every colour rate is 0 or 1e9 (the colour keeps its value or saturates to exactly 1)"""
    return [er.emitter((0.45, 0.5, 0.5), 0.3, color_rate=(0.0, 1e9, 0.0, 0.0), force=(0.0, 0.0, 0.0), swirl=1e-4),
            er.emitter((0.6, 0.55, 0.5), 0.3, color_rate=(0.0, 0.0, 1e9, 0.0), force=(0.0, 0.0, 0.0), swirl=3e6)]


@functools.lru_cache(maxsize=None)
def emit_half(dims):
    vel, col, _ = half_state(dims, 2, colour_negzero=False)
    dt = time_step(dims)
    ems = emitters_exact(dims)
    wv, wc, m = er.apply(vel, col, ems, dt, half=True)
    is3d = dims[2] > 1
    # a 2-D grid's force is (basis * fx, basis * fy, 0) = 0 here -- no swirl term: fma(0, dt, u) = u, but for a -0, which comes back +0;
    # the stores of the 2-D case are the subnormals (and everything else) passed through
    cond = edge_conditions("emit %s velocity" % (dims,), half_bits(wv[:3 if is3d else 2][:, m]), overflow=is3d, negzero=is3d)
    cond += edge_conditions("emit %s colour" % (dims,), half_bits(wc[m]), overflow=False, negzero=False)      # saturated, and no -0 among the inputs
    cond.append(("emit %s: cells within 1e-5 of the threshold" % (dims,), float(er.near_threshold(dims, ems)), "==", 0.0))
    cond.append(("emit %s: cells inside a support" % (dims,), float(m.sum()), ">=", 400.0))
    return case(vel=vel, col=col, dt=dt, emitters=ems, want_vel=wv, want_col=wc, touched=m, conditions=cond)


def perturbed_basis_changes_nothing(dims, rel=3e-7):
    """the emitter case again with every basis scaled by 1 +- rel (an ulp or two of exp2): True if no output bit and no support cell changes"""
    c = emit_half(dims)
    out = [er.apply(c.vel, c.col, c.emitters, c.dt, half=True, basis_scale=s) for s in (1.0 - rel, 1.0 + rel)]
    return all(same_bits(v, c.want_vel) and same_bits(k, c.want_col) and np.array_equal(m, c.touched) for v, k, m in out)


HEAT_HALF = br.params(ambient=0.0, density_weight=0.5, lift=32.0, cooling=0.3, up=(0.3, 1.0, -0.2))


@functools.lru_cache(maxsize=None)
def heat_half(dims, address="clamp"):
    """no sources: no transcendental, the whole pass is exact.  The force fma(lift, T1, -(weight * rho)) * up * dt has to be far below 2^-24
    for a subnormal velocity to stay one and around 10^4 for a large one to overflow, so the grid has a quiet half (y < Y / 2: temperature
    2^-50 .. 2^-30, smoke 2^-27 .. 2^-22) and a loud one (temperature -- fp32 in every context -- 2^-27 .. 2^16, a third of it within 2^12 ..
    2^16; smoke over the whole binary16 range); VELOCITY1 has extra mass at both ends of the range everywhere"""
    X, Y, Z = dims
    vel1, col, _ = half_state(dims, 3, ends=0.4)
    vel0 = crossing_velocity(dims, 4, half=True)
    rng = np.random.default_rng(seed_of(dims, 5))
    T = log_uniform(rng, (Z, Y, X), -27, 16)
    T = np.where(rng.random((Z, Y, X)) < 1 / 3, log_uniform(rng, (Z, Y, X), 12, 16), T)
    quiet = np.arange(Y) < Y // 2
    T = np.where(quiet[None, :, None], log_uniform(rng, (Z, Y, X), -50, -30), T).astype(f32)
    col = col.copy()
    col[..., 3] = np.where(quiet[None, :, None], to_half(log_uniform(rng, (Z, Y, X), -27, -22)), col[..., 3])
    zero_lattice(T)
    dt = time_step(dims)
    wT, wv = br.apply(T, vel0, vel1, col, HEAT_HALF, [], dt, address, half=True)
    stored = np.zeros(vel1.shape, bool)
    stored[br.axes(dims, HEAT_HALF["up"])] = True
    cond = edge_conditions("heat %s %s VELOCITY1" % (dims, address), half_bits(wv[stored]), overflow=True)
    return case(T=T, vel0=vel0, vel1=vel1, col=col, dt=dt, prm=HEAT_HALF, address=address, want_T=wT, want=wv, stored=stored, conditions=cond)


@functools.lru_cache(maxsize=None)
def inflow_half(dims):
    """every legal face open; the pass stores the cells whose weight is not 1"""
    _, col, _ = half_state(dims, 6)
    vel0 = crossing_velocity(dims, 7, half=True)
    dt = time_step(dims)
    faces = orf.legal_faces(dims)
    w = orf.inflow_weights(vel0, dt, faces)
    want = orf.ref_inflow(col, vel0, dt, faces, half=True)
    stored = np.broadcast_to((w != 1)[..., None], col.shape).copy()
    cond = edge_conditions("inflow %s" % (dims,), half_bits(want[stored]), overflow=False)      # a blend towards clear air
    cond.append(("inflow %s: share of cells the pass stores" % (dims,), float((w != 1).mean()), ">=", 0.05))
    return case(vel0=vel0, col=col, dt=dt, faces=faces, w=w, want=want, stored=stored, conditions=cond)


@functools.lru_cache(maxsize=None)
def enforce_half(dims):
    """solid cells that hold -0, subnormals and +-65504 come back as +0 bits; no other cell changes a bit"""
    vel, col, _ = half_state(dims, 8)
    vel, col = vel.copy(), col.copy()
    vel[:, :, 1::4, 2::7] = BIG
    vel[:, :, 3::4, 2::7] = -BIG
    col[:, 2::4, 3::7, :] = BIG
    m = mask_of(dims)
    wv, wc = ob.ref_enforce(vel, col, m)
    s = m != 0
    # on the INPUT of the solid cells: the -0, the subnormals and the +-65504 that have to come back as +0
    cond = []
    for what, h in (("velocity", half_bits(vel[:, s])), ("colour", half_bits(col[s]))):
        sub, _, nz, nan = shares(h)
        cond += [("enforce %s solid %s in: subnormal share" % (dims, what), sub, ">=", 0.02), ("enforce %s solid %s in: -0 share" % (dims, what), nz, ">=", 2e-4),
                 ("enforce %s solid %s in: NaN share" % (dims, what), nan, "==", 0.0),
                 ("enforce %s solid %s in: +-65504 share" % (dims, what), float(((h & 0x7FFF) == 0x7BFF).mean()), ">=", 2e-4)]
    cond.append(("enforce %s: solid cells of the output that are not +0 bits" % (dims,), float(bits(wv)[:, s].any() or bits(wc)[s].any()), "==", 0.0))
    cond.append(("enforce %s: fluid cells the model changes" % (dims,), float((bits(wv) != bits(vel))[:, ~s].sum() + (bits(wc) != bits(col))[~s].sum()), "==", 0.0))
    return case(vel=vel, col=col, mask=m, want_vel=wv, want_col=wc, conditions=cond)


PROJECT_SETTINGS = ["obstacles", "open walls", "both"]


def setting(dims, name):
    """(mask or None, faces) of the three settings of the boundary-aware kernels"""
    return (mask_of(dims) if name != "open walls" else None, orf.legal_faces(dims) if name != "obstacles" else 0)


@functools.lru_cache(maxsize=None)
def project_half(dims, name):
    vel, _, p = half_state(dims, 9, ends=0.5)
    m, faces = setting(dims, name)
    want = orf.ref_project(vel, p, m, faces, half=True)
    fluid = np.ones(p.shape, bool) if m is None else m == 0
    stored = np.broadcast_to(fluid, vel.shape).copy()
    if dims[2] == 1:
        stored[2] = False                                    # 2-D: uz never changes
    cond = edge_conditions("project %s %s" % (dims, name), half_bits(want[stored]), overflow=True)
    return case(vel=vel, p=p, mask=m, faces=faces, want=want, stored=stored, conditions=cond)


@functools.lru_cache(maxsize=None)
def maccormack_half(dims, address):
    """the impulse off: bit for bit everywhere.  The tracing velocity (itself advected) is 2^-27 .. 2^7, the colour the whole range"""
    vel0, col, _ = half_state(dims, 10, vel=(-27, 7))
    dt = time_step(dims)
    wv, wc = mr.step(vel0, col, dt, address, impulse=False, half=True)
    # no store can overflow: the result is limited to storable taps and then multiplied by an attenuation below 1
    cond = edge_conditions("maccormack %s %s velocity" % (dims, address), half_bits(wv[:3 if dims[2] > 1 else 2]), overflow=False)
    cond += edge_conditions("maccormack %s %s colour" % (dims, address), half_bits(wc), overflow=False)
    return case(vel0=vel0, col=col, dt=dt, address=address, want_vel=wv, want_col=wc, conditions=cond)


# ---- part 2: fp32 subnormals --------------------------------------------------------------------------------------------------------------
VORTICITY_EPS = 8.0


@functools.lru_cache(maxsize=None)
def vorticity_subnormal(dims, kind):
    """kind "log": magnitudes log-uniform in 2^-140 .. 2^-60 -- the squares under the pass's sqrtf are subnormal in almost half of the cells
    and the pass still changes a good share of them.  kind "all": standard_normal * 2^-128, every input subnormal; the model changes nothing"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed_of(dims, 11))
    vel = log_uniform(rng, (3, Z, Y, X), -140, -60) if kind == "log" else subnormal_field(dims, 12, (3,))
    if Z == 1:
        vel[2] = 0
    dt = time_step(dims)
    want = vr.confine(vel, VORTICITY_EPS, dt)
    with np.errstate(all="ignore"):
        wz = vr._diff(vel[1], 2, f32) - vr._diff(vel[0], 1, f32)
        sq = wz * wz
    changed = float((bits(want) != bits(vel)).any(axis=0).mean())
    what = "vorticity fp32 %s %s: " % (dims, kind)
    cond = [(what + "NaN count", float(np.isnan(want).sum()), "==", 0.0)]
    if kind == "log":
        cond += [(what + "cells whose wz * wz is subnormal and non-zero", subnormal_share(sq), ">=", 0.3), (what + "cells the pass changes", changed, ">=", 0.15)]
    else:
        planes = vel if Z > 1 else vel[:2]
        cond += [(what + "inputs that are subnormal and non-zero", subnormal_share(planes), ">", 0.99), (what + "cells the pass changes", changed, "==", 0.0)]
    return case(vel=vel, dt=dt, eps=VORTICITY_EPS, want=want, conditions=cond)


SWEEPS = 5


def not_forced_to_zero(mask, shape3):
    """[3][Z][Y][X]: velocity components the boundary-aware projection does not set to +0 by rule -- cells that are not solid and, along the
    component's own axis, have no solid neighbour (free slip)"""
    Z, Y, X = shape3
    free = np.ones((3, Z, Y, X), bool)
    if mask is not None:
        s = mask != 0
        for a, axis in enumerate((2, 1, 0)):
            free[a] = ~s & ~orf._shift(s, axis, -1) & ~orf._shift(s, axis, 1)
    if Z == 1:
        free[2] = False
    return free


@functools.lru_cache(maxsize=None)
def pressure_subnormal(dims, name):
    """boundary-aware divergence, SWEEPS sweeps and projection of standard_normal * 2^-128 fields (tests/test_gpu_stage_matrix.py
    test_fp32_subnormal_fields_bit_exact's): (b, q, w) of the model and the share of each that is subnormal and non-zero, counted over the
    cells that are not solid -- for a velocity component also not next to a solid cell along its axis, where free slip stores +0"""
    vel, p = subnormal_field(dims, 13, (3,)), subnormal_field(dims, 14)
    if dims[2] == 1:
        vel[2] = 0
    m, faces = setting(dims, name)
    wv = ob.ref_enforce(vel, np.zeros(p.shape + (4,), f32), m)[0] if m is not None else vel
    b = ob.ref_divergence(wv, m if m is not None else np.zeros(p.shape, np.uint8))
    q = orf.ref_jacobi(p, b, m, faces, SWEEPS)
    w = orf.ref_project(wv, q, m, faces)
    fluid = np.ones(p.shape, bool) if m is None else m == 0
    sh = (subnormal_share(b[fluid]), subnormal_share(q[fluid]), subnormal_share(w[not_forced_to_zero(m, p.shape)]))
    cond = [("pressure fp32 %s %s: subnormal and non-zero share of the %s" % (dims, name, what), v, ">", 0.99) for what, v in zip(("divergence", "pressure", "velocity"), sh)]
    return case(vel=vel, p=p, mask=m, faces=faces, b=b, q=q, w=w, conditions=cond)


MG_TINY = 2.0 ** -131


@functools.lru_cache(maxsize=None)
def multigrid_subnormal(dims):
    p, b = subnormal_field(dims, 15, scale=MG_TINY), subnormal_field(dims, 16, scale=MG_TINY)
    prm = mg.defaults(dims)
    want = mg.solve(p, b, prm)
    cond = [("multigrid fp32 %s: subnormal and non-zero share of the pressure" % (dims,), subnormal_share(want[0]), ">", 0.99)]
    cond += [("multigrid fp32 %s: subnormal and non-zero share of level %d's %s" % (dims, l, what), subnormal_share(a), ">", 0.99)
             for l in range(1, len(want[1])) for what, a in zip(("correction", "right-hand side"), want[1][l])]
    return case(p=p, b=b, prm=prm, want=want, conditions=cond)


FIELD_INPUTS = ["colour", "temperature"]
HEAT_SUB = {"colour": br.params(ambient=0.25, density_weight=0.7, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2)),
            "temperature": br.params(ambient=0.0, density_weight=0.0, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2))}


@functools.lru_cache(maxsize=None)
def field_subnormal(dims, which):
    """the two inputs of the field passes: "colour" -- a subnormal colour, the temperature at its ambient value everywhere (so that the
    force is -(weight * rho), subnormal, alone); "temperature" -- a subnormal temperature with ambient = 0 under an ordinary colour and no
    density weight.  VELOCITY1 is subnormal in both, so that the force shows; the tracing velocity is an ordinary one that crosses cells"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed_of(dims, 17))
    vel0 = crossing_velocity(dims, 18)
    vel1 = subnormal_field(dims, 19, (3,))
    if which == "colour":
        col = np.moveaxis(subnormal_field(dims, 20, (4,)), 0, -1).copy()
        T = np.full((Z, Y, X), f32(HEAT_SUB[which]["ambient"]))
    else:
        col = rng.random((Z, Y, X, 4)).astype(f32)
        T = subnormal_field(dims, 21)
    dt = time_step(dims)
    prm = HEAT_SUB[which]
    faces = orf.legal_faces(dims)
    mv, mc = mr.step(vel0, col, dt, "clamp", impulse=False)
    hT, hv = br.apply(T, vel0, vel1, col, prm, [], dt, "clamp")
    w = orf.inflow_weights(vel0, dt, faces)
    inflow = orf.ref_inflow(col, vel0, dt, faces)
    what = "fields fp32 %s subnormal %s: " % (dims, which)
    blended = (w > 0) & (w < 1)
    cond = [(what + "subnormal and non-zero share of the force's VELOCITY1", subnormal_share(hv[br.axes(dims, prm["up"])]), ">", 0.99),
            (what + "VELOCITY1 values the force changes", float((bits(hv) != bits(vel1))[br.axes(dims, prm["up"])].mean()), ">=", 0.5),
            (what + "cells the inflow blends (0 < w < 1)", float(blended.mean()), ">=", 0.02)]
    if which == "colour":
        cond += [(what + "subnormal and non-zero share of the MacCormack colour", subnormal_share(mc), ">", 0.99),
                 (what + "subnormal and non-zero share of the blended inflow colour", subnormal_share(inflow[blended]), ">", 0.99)]
    else:
        cond += [(what + "subnormal and non-zero share of the temperature", subnormal_share(hT), ">", 0.99)]
    return case(vel0=vel0, vel1=vel1, col=col, T=T, dt=dt, prm=prm, faces=faces, mc_vel=mv, mc_col=mc, heat_T=hT, heat_vel=hv, w=w, inflow=inflow,
                conditions=cond)
