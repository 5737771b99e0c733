"""CPU model of the vorticity confinement pass (include/fluidx_hip.h fx_set_vorticity_confinement, csrc/fx_vorticity.hip).

numpy, float32 throughout, every operation rounded on its own and in the association the header states, so that the HIP kernel
(no fmaf, correctly rounded sqrtf and /) reproduces it bit for bit; dtype=np.float64 runs the same formulas in double for error estimates.

    D_a f = 0.5 * (f[upper clamped neighbour along a] - f[lower clamped neighbour along a])        (xl = max(x,1)-1, xr = min(x+1,X-1))
    w  = (Dy(uz) - Dz(uy), Dz(ux) - Dx(uz), Dx(uy) - Dy(ux))     m = sqrt((wx*wx + wy*wy) + wz*wz)
    g  = (Dx(m), Dy(m), Dz(m))                                   l = sqrt((gx*gx + gy*gy) + gz*gz)
    s  = (eps * dt) / (l + 1e-6)                                 u' = u + (g x w) * s
    2-D (Z == 1): every z difference is 0 -- wx = wy = gz = 0, m = |wz| -- and uz comes back unchanged.

Not under oracle/: nothing here restates the reference (it has no such pass).
"""
import numpy as np


def _diff(f, axis, dtype):
    """D along `axis` of an array [Z][Y][X] with clamped neighbour indices"""
    n = f.shape[axis]
    i = np.arange(n)
    lo, hi = np.maximum(i, 1) - 1, np.minimum(i + 1, n - 1)
    return dtype(0.5) * (np.take(f, hi, axis=axis) - np.take(f, lo, axis=axis))


def confine(u, eps, dt, dtype=np.float32):
    """u: array [3][Z][Y][X] (ux, uy, uz; the fx_download layout of VELOCITY1) -> the confined field, same layout and `dtype`"""
    u = np.asarray(u, dtype)
    assert u.ndim == 4 and u.shape[0] == 3
    ux, uy, uz = u[0], u[1], u[2]
    Z = ux.shape[0]
    AZ, AY, AX = 0, 1, 2
    zero = np.zeros_like(ux)
    with np.errstate(all="ignore"):
        wz = _diff(uy, AX, dtype) - _diff(ux, AY, dtype)
        if Z > 1:
            wx = _diff(uz, AY, dtype) - _diff(uy, AZ, dtype)
            wy = _diff(ux, AZ, dtype) - _diff(uz, AX, dtype)
            m = np.sqrt((wx * wx + wy * wy) + wz * wz)
            gz = _diff(m, AZ, dtype)
        else:
            wx, wy = zero, zero
            m = np.abs(wz)
            gz = zero
        gx, gy = _diff(m, AX, dtype), _diff(m, AY, dtype)
        l = np.sqrt((gx * gx + gy * gy) + gz * gz)
        s = (dtype(eps) * dtype(dt)) / (l + dtype(1e-6))
        Fx = gy * wz - gz * wy
        Fy = gz * wx - gx * wz
        Fz = gx * wy - gy * wx
        out = np.empty_like(u)
        out[0] = ux + Fx * s
        out[1] = uy + Fy * s
        out[2] = uz + Fz * s if Z > 1 else uz
    assert out.dtype == dtype
    return out


def confine_stored(u, eps, dt, half):
    """the pass as a context with fp16 (half=True) or fp32 storage runs it: the input as stored, the result rounded to storage (RNE), as float32"""
    if not half:
        return confine(u, eps, dt)
    u16 = np.asarray(u, np.float32).astype(np.float16).astype(np.float32)
    return confine(u16, eps, dt).astype(np.float16).astype(np.float32)
