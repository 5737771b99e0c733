"""numpy model of the emitter pass (include/fluidx_hip.h fx_set_emitters, fluidx12_amd/csrc/fx_emit.hip: k_emit).

The pass in fp32, operation by operation, with one liberty: exp2 is evaluated in float64 and rounded once, which differs from the device by
an ulp here and there.  (A fused multiply-add is fmaf's, correctly rounded: tests/fma_ref.py.)  So the tests compare
  * outside every emitter's support: bit for bit (the cell is unchanged), and
  * inside: rel-L2 < 1e-6, the figure tests/test_gpu_sim.py::test_advect_matches_oracle uses for the built-in ball,
and they assert first (near_threshold) that no cell's basis sits so close to the threshold e^-4 that an ulp of exp2 decides its side.

Layouts as Fluid.upload / download: velocity float32[3][Z][Y][X], colour float32[Z][Y][X][4]."""
import numpy as np

from fma_ref import fma

f32, f64 = np.float32, np.float64
THRESHOLD = f32(0.0183156393)        # e^-4 as the kernels spell it
LOG2E = f32(1.44269502)

# the reference's built-in impulse as an emitter (Impulse.hlsli, CSAdvect.hlsl:59-68)
BUILTIN_3D = dict(center=(0.5, f32(0.1), 0.5), radius=1.0 / 16, color_rate=(8.0, 16.0, 40.0, 40.0), force=(0.0, 192.0, 0.0), swirl=200.0)
BUILTIN_2D = dict(center=(0.5, f32(0.1), 0.5), radius=1.0 / 32, color_rate=(8.0, 16.0, 40.0, 40.0), force=(0.0, 48.0, 0.0), swirl=0.0)


def emitter(center, radius, color_rate=(8.0, 16.0, 40.0, 40.0), force=(0.0, 192.0, 0.0), swirl=200.0):
    return dict(center=tuple(center), radius=radius, color_rate=tuple(color_rate), force=tuple(force), swirl=swirl)


def exponent(dims, e):
    """(ex, dx, dz) of every cell for emitter e: float32[Z][Y][X] each"""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    px = (x.astype(f32) + f32(0.5)) / f32(X)
    py = (y.astype(f32) + f32(0.5)) / f32(Y)
    pz = (z.astype(f32) + f32(0.5)) / f32(Z)
    cx, cy, cz = (f32(v) for v in e["center"])
    dx, dy = px - cx, py - cy
    dz = pz - cz if Z > 1 else np.zeros_like(px)
    d2 = fma(dz, dz, fma(dy, dy, dx * dx))
    r = f32(e["radius"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ex = ((d2 * f32(-4.0)) / (r * r)) * LOG2E
    return ex, dx, dz


def basis64(dims, e):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp2(exponent(dims, e)[0].astype(f64))


def near_threshold(dims, emitters, rel=1e-5):
    """cells whose float64 basis lies within relative `rel` of the threshold, summed over the emitters"""
    t = f64(THRESHOLD)
    return int(sum((np.abs(basis64(dims, e) - t) <= rel * t).sum() for e in emitters))


def support(dims, e):
    with np.errstate(invalid="ignore"):
        return basis64(dims, e).astype(f32) >= THRESHOLD


def apply(vel, col, emitters, dt, half=False, basis_scale=1.0):
    """the pass: (velocity, colour, mask of the cells inside at least one support).  half: the fields are fp16-stored -- vel / col must hold
    fp16-representable values; every changed cell is rounded once (RNE) behind the last emitter.  basis_scale: every basis times this factor
    before it is rounded to float32 -- a stand-in for another exp2's last bits (tests/store_edges.py shows with it that a case does not
    depend on them)"""
    _, Z, Y, X = vel.shape
    dims = (X, Y, Z)
    dt = f32(dt)
    u = [vel[a].astype(f32).copy() for a in range(3)]
    c = [col[..., i].astype(f32).copy() for i in range(4)]
    touched = np.zeros((Z, Y, X), bool)
    for e in emitters:
        ex, dx, dz = exponent(dims, e)
        with np.errstate(over="ignore", invalid="ignore"):
            basis = (np.exp2(ex.astype(f64)) * f64(basis_scale)).astype(f32)
            m = basis >= THRESHOLD
        if not m.any():
            continue
        fx_, fy_, fz_ = (f32(v) for v in e["force"])
        sw = f32(e["swirl"])
        b = np.where(m, basis, f32(0))
        if Z > 1:
            F = [fma(b, fx_, dz * -sw), fma(b, fy_, f32(0)), fma(b, fz_, dx * sw)]
        else:
            F = [b * fx_, b * fy_, np.zeros_like(b)]
        bdt = b * dt
        for a in range(3):
            u[a] = np.where(m, fma(F[a], dt, u[a]), u[a])
        for i in range(4):
            c[i] = np.where(m, np.clip(fma(bdt, f32(e["color_rate"][i]), c[i]), f32(0), f32(1)), c[i])
        touched |= m
    vo, co = np.stack(u), np.stack(c, axis=-1)
    if half:
        vo = np.where(touched[None], vo.astype(np.float16).astype(f32), vel)
        co = np.where(touched[..., None], co.astype(np.float16).astype(f32), col)
    return vo, co, touched


def apply_loops(vel, col, emitters, dt):
    """the same, cell by cell in plain loops (fp32 storage): what tests/test_emitter_ref.py holds `apply` against"""
    _, Z, Y, X = vel.shape
    dt = f32(dt)
    vo, co = vel.copy(), col.copy()
    touched = np.zeros((Z, Y, X), bool)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                px, py, pz = (f32(x) + f32(0.5)) / f32(X), (f32(y) + f32(0.5)) / f32(Y), (f32(z) + f32(0.5)) / f32(Z)
                for e in emitters:
                    dx, dy = px - f32(e["center"][0]), py - f32(e["center"][1])
                    dz = pz - f32(e["center"][2]) if Z > 1 else f32(0)
                    d2 = fma(dz, dz, fma(dy, dy, dx * dx))
                    r = f32(e["radius"])
                    basis = f32(2.0 ** float(((d2 * f32(-4.0)) / (r * r)) * LOG2E))
                    if not basis >= THRESHOLD:
                        continue
                    sw = f32(e["swirl"])
                    if Z > 1:
                        F = (fma(basis, f32(e["force"][0]), dz * -sw), fma(basis, f32(e["force"][1]), f32(0)), fma(basis, f32(e["force"][2]), dx * sw))
                    else:
                        F = (basis * f32(e["force"][0]), basis * f32(e["force"][1]), f32(0))
                    for a in range(3):
                        vo[a, z, y, x] = fma(F[a], dt, vo[a, z, y, x])
                    bdt = basis * dt
                    for i in range(4):
                        co[z, y, x, i] = min(max(fma(bdt, f32(e["color_rate"][i]), co[z, y, x, i]), f32(0)), f32(1))
                    touched[z, y, x] = True
    return vo, co, touched
