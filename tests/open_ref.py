"""numpy model of the open walls (include/fluidx_hip.h fx_set_open_walls, fluidx12_amd/csrc/fx_open.hip): the four rules in fp32, every
operation rounded as written.

  ref_jacobi      relaxation: a neighbour beyond an open face reads +0, otherwise a solid one p(c), otherwise p(n)
  ref_project     projection: the same q in the gradient, the free-slip rule of the obstacles, no wall damping towards an open face
  inflow_weights  w = (w_x * w_y) * w_z of the back-trace (2-D: w_x * w_y); ref_inflow: COLOR * w
  heat_apply      tests/buoyancy_ref.py's `apply` with Ts = fma(w, Ts - Ta, Ta) between its steps 1 and 2

"Beyond an open face" = a stencil neighbour whose unclamped index is -1 or N on an axis whose face there is open.  With faces = 0 the first two
are tests/obstacle_ref/ bit for bit and heat_apply is buoyancy_ref.apply (tests/test_open_ref.py holds them to that).

The fused multiply-adds are fmaf's, correctly rounded (tests/fma_ref.py, the one every model uses: the float64 sum is rounded to odd before it
is rounded to float32, so the two roundings cannot disagree with the one of fmaf).

Layouts as Fluid.upload / download: velocity float32[3][Z][Y][X], colour float32[Z][Y][X][4], pressure, divergence and masks [Z][Y][X]."""
import numpy as np

import buoyancy_ref as br
from fma_ref import fma

f32, f64 = np.float32, np.float64

X_LO, X_HI, Y_LO, Y_HI, Z_LO, Z_HI = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
ALL_3D, ALL_2D = 0x3F, 0x0F
INV6 = np.array([0x3e2aaaab], np.uint32).view(f32)[0]
KD3 = np.array([0x3f855556], np.uint32).view(f32)[0]           # 0.5f / 0.48f
# (numpy axis of [Z][Y][X], step, face bit) of the six neighbours in the sum's order: x-1, x+1, y-1, y+1, z-1, z+1
NEIGHBOURS = [(2, -1, X_LO), (2, 1, X_HI), (1, -1, Y_LO), (1, 1, Y_HI), (0, -1, Z_LO), (0, 1, Z_HI)]


def legal_faces(dims):
    return ALL_3D if dims[2] > 1 else ALL_2D


def face_sets(dims):
    """what the GPU tests run: each single face, Y_HI | X_LO, all legal faces"""
    singles = [X_LO, X_HI, Y_LO, Y_HI] + ([Z_LO, Z_HI] if dims[2] > 1 else [])
    return singles + [Y_HI | X_LO, legal_faces(dims)]


def _shift(a, axis, d):
    """a at index clamp(i + d) along axis"""
    n = a.shape[axis]
    return np.take(a, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def _on_face(shape, axis, d):
    """cells whose neighbour at step d along axis has the unclamped index -1 or N"""
    n = shape[axis]
    idx = np.arange(n)
    m = (idx == 0) if d < 0 else (idx == n - 1)
    sh = [1, 1, 1]
    sh[axis] = n
    return np.broadcast_to(m.reshape(sh), shape)


def _rule(shape, solid, faces, axis, d, bit):
    """(cells whose neighbour lies beyond an open face or None, cells whose clamped neighbour is solid or None)"""
    return (_on_face(shape, axis, d) if (faces & bit) else None, _shift(solid, axis, d) if solid.any() else None)


def _read(p, rule, axis, d):
    """the neighbour of every cell as the relaxation and the projection read it: beyond an open face ? +0 : S(n) ? p(c) : p(n)"""
    beyond, solid_n = rule
    q = _shift(p, axis, d)
    if solid_n is not None:
        q = np.where(solid_n, p, q)
    if beyond is not None:
        q = np.where(beyond, f32(0.0), q)
    return q.astype(f32, copy=False)


def _q(p, solid, faces, axis, d, bit):
    return _read(p, _rule(p.shape, solid, faces, axis, d, bit), axis, d)


def _solid(mask, shape):
    if mask is None:
        return np.zeros(shape, bool)
    return np.asarray(mask).reshape(shape) != 0


def ref_jacobi(p, b, mask, faces, n):
    p, b = np.array(p, f32), np.asarray(b, f32)
    solid = _solid(mask, p.shape)
    is3d = p.shape[0] > 1
    assert is3d or not (faces & (Z_LO | Z_HI))
    inv = INV6 if is3d else f32(0.25)
    nbs = NEIGHBOURS if is3d else NEIGHBOURS[:4]
    rules = [_rule(p.shape, solid, faces, ax, d, bit) for ax, d, bit in nbs]
    any_solid = solid.any()
    for _ in range(int(n)):
        s = _read(p, rules[0], nbs[0][0], nbs[0][1]) - b
        for rule, (ax, d, _) in zip(rules[1:], nbs[1:]):
            s = _read(p, rule, ax, d) + s
        p = s * inv
        if any_solid:
            p = np.where(solid, f32(0.0), p)
    return p.astype(f32, copy=False)


def ref_project(vel, p, mask, faces, half=False):
    vel, p = np.asarray(vel, f32), np.asarray(p, f32)
    Z, Y, X = p.shape
    solid = _solid(mask, p.shape)
    is3d = Z > 1
    assert is3d or not (faces & (Z_LO | Z_HI))
    kd = KD3 if is3d else f32(0.5)
    u = [vel[a].copy() for a in range(3)]
    for a in range(3 if is3d else 2):
        (ax, dm, bm), (_, dp, bp) = NEIGHBOURS[2 * a], NEIGHBOURS[2 * a + 1]
        grad = -_q(p, solid, faces, ax, dm, bm) + _q(p, solid, faces, ax, dp, bp)
        u[a] = fma(-grad, kd, u[a])
        u[a] = np.where(_shift(solid, ax, dm) | _shift(solid, ax, dp), f32(0.0), u[a]).astype(f32)       # free slip (2-D grids: no z neighbours)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    out = np.empty_like(vel)
    for a, (cell, n) in enumerate(((x, X), (y, Y), (z, Z))):
        pos = (cell.astype(f32) + f32(0.5)) / f32(n)
        if is3d or a < 2:
            pos = fma(pos, f32(2.0), f32(-1.0))
        f = (-np.abs(pos) + f32(0.970000029)) * f32(33.3333359)
        f = np.minimum(np.maximum(f, f32(-1.0)), f32(1.0))
        opened = ((pos < 0) & bool(faces & (1 << (2 * a)))) | ((pos > 0) & bool(faces & (2 << (2 * a))))
        w = np.where((f32(0.0) < u[a] * pos) & ~opened, f, f32(1.0)).astype(f32)
        r = np.where(solid, f32(0.0), u[a] * w).astype(f32)
        out[a] = r.astype(np.float16).astype(f32) if half else r
    return out


def trace(u0, dt, dims):
    """per axis (floor(t), t - floor(t)) of every cell's back-trace, t as buoyancy_ref.sample forms it"""
    X, Y, Z = dims
    dt = f32(dt)
    p = br.cell_centres(dims)
    out = []
    for a, n in enumerate(dims):
        t = br.fma(-np.asarray(u0[a], f32), dt, p[a]) * f32(n) - f32(0.5)
        fl = np.floor(t).astype(f32)
        out.append((fl, (t - fl).astype(f32)))
    return out


def axis_weight(fl, f, n, lo_open, hi_open):
    w = np.ones(fl.shape, f32)
    if lo_open:
        w = np.where(fl < 0, np.where(fl == -1, f, f32(0.0)), w)
    if hi_open:
        w = np.where(fl >= n - 1, np.where(fl == n - 1, f32(1.0) - f, f32(0.0)), w)
    return w.astype(f32)


def inflow_weights(vel0, dt, faces):
    _, Z, Y, X = np.shape(vel0)
    dims = (X, Y, Z)
    assert Z > 1 or not (faces & (Z_LO | Z_HI))
    tr = trace(vel0, dt, dims)
    wa = [axis_weight(tr[a][0], tr[a][1], dims[a], bool(faces & (1 << (2 * a))), bool(faces & (2 << (2 * a)))) for a in range(3)]
    w = wa[0] * wa[1]
    if Z > 1:
        w = w * wa[2]
    return w.astype(f32)


def ref_inflow(col, vel0, dt, faces, half=False):
    """COLOR * w, all four channels; half: the colour holds fp16-representable values and every product is rounded once (RNE)"""
    w = inflow_weights(vel0, dt, faces)
    out = (np.asarray(col, f32) * w[..., None]).astype(f32)
    return out.astype(np.float16).astype(f32) if half else out


def heat_apply(T, vel0, vel1, col, prm, sources, dt, address="clamp", half=False, solid=None, faces=0):
    """buoyancy_ref.apply with the open-wall rule between its steps 1 and 2 (restated from it, operation for operation)"""
    er = br.er
    Z, Y, X = T.shape
    dims = (X, Y, Z)
    dt = f32(dt)
    Ta, weight, lift, cooling = f32(prm["ambient"]), f32(prm["density_weight"]), f32(prm["lift"]), f32(prm["cooling"])
    Ts = br.sample(T.astype(f32), vel0, dt, address)
    if faces:
        Ts = br.fma(inflow_weights(vel0, dt, faces), Ts - Ta, Ta)
    keep = np.maximum(br.fma(-dt, cooling, f32(1.0)), f32(0.0))
    T1 = br.fma(Ts - Ta, keep, Ta)
    for s in sources:
        ex = er.exponent(dims, br.as_emitter(s))[0]
        with np.errstate(over="ignore", invalid="ignore"):
            basis = np.exp2(ex.astype(f64)).astype(f32)
            m = basis >= er.THRESHOLD
        T1 = np.where(m, br.fma(np.where(m, basis, f32(0)) * dt, f32(s["rate"]), T1), T1)
    if solid is None:
        solid = np.zeros((Z, Y, X), bool)
    solid = np.asarray(solid) != 0
    T1 = np.where(solid, Ta, T1).astype(f32)
    rho = col[..., 3].astype(f32)
    sc = br.fma(lift, T1 - Ta, -(weight * rho))
    out = vel1.astype(f32).copy()
    for a in br.axes(dims, prm["up"]):
        new = br.fma(f32(prm["up"][a]) * sc, dt, vel1[a].astype(f32))
        if half:
            new = new.astype(np.float16).astype(f32)
        out[a] = np.where(solid, vel1[a], new)
    return T1, out
