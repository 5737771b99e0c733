"""CPU checks of the open walls (fx_set_open_walls): the C ABI surface without a device, the numpy model tests/open_ref.py anchored to the
obstacle reference (faces = 0 changes no bit) and to buoyancy_ref, its rules by hand, and the plume that the feature is for: with the top
of the box open the smoke leaves, with the box closed it piles up under the lid.  tests/test_gpu_open_walls.py holds the kernels against
this model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import buoyancy_ref as br
import np_ref
import open_ref as orf
import test_obstacle_ref as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_with_the_open_wall_calls(tmp_path):
    src = tmp_path / "open_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'static int (*set_)(fx_ctx*, uint32_t) = fx_set_open_walls;\n'
                   'static int (*get_)(fx_ctx*, uint32_t*) = fx_get_open_walls;\n'
                   'static int (*inflow_)(fx_ctx*, void*) = fx_open_inflow;\n'
                   'int main(void) { (void)set_; (void)get_; (void)inflow_; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        val = tmp_path / "open_values.c"                                 # the constants, evaluated (the calls above need the library to link)
        val.write_text('#include "fluidx_hip.h"\nint main(void) { return FX_WALL_X_LO == 0x01u && FX_WALL_X_HI == 0x02u && FX_WALL_Y_LO == 0x04u && '
                       'FX_WALL_Y_HI == 0x08u && FX_WALL_Z_LO == 0x10u && FX_WALL_Z_HI == 0x20u && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(val), "-o", str(tmp_path / "values")], check=True)
        assert subprocess.run([str(tmp_path / "values")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_mirrors_carry_the_three_calls():
    from fluidx12_amd import capi, build
    import fluidx12_amd as fx
    for name in ("fx_set_open_walls", "fx_get_open_walls", "fx_open_inflow"):
        assert name in capi.SYMBOLS
    assert capi.SYMBOLS["fx_set_open_walls"][1][1:] == [C.c_uint32] and capi.ABI_VERSION == 7
    assert (capi.WALL_X_LO, capi.WALL_X_HI, capi.WALL_Y_LO, capi.WALL_Y_HI, capi.WALL_Z_LO, capi.WALL_Z_HI) == (1, 2, 4, 8, 16, 32)
    assert (orf.X_LO, orf.X_HI, orf.Y_LO, orf.Y_HI, orf.Z_LO, orf.Z_HI) == (1, 2, 4, 8, 16, 32)
    for name in ("SetOpenWalls", "GetOpenWalls", "OpenInflow"):
        assert callable(getattr(fx.Fluid, name))
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetOpenWalls", "GetOpenWalls", "OpenInflow", "fx_set_open_walls", "fx_get_open_walls", "fx_open_inflow"):
        assert name in hpp, name
    assert "-openWalls" in open(os.path.join(ROOT, "examples", "fluidx_demo.cpp")).read()
    assert "fx_open.hip" in build.SOURCES


def test_a_null_context_is_refused():
    from fluidx12_amd import capi
    lib = capi.load()
    faces = C.c_uint32(77)
    assert lib.fx_set_open_walls(None, 0) == capi.FX_E_INVALID and lib.fx_set_open_walls(None, capi.WALL_Y_HI) == capi.FX_E_INVALID
    assert lib.fx_get_open_walls(None, C.byref(faces)) == capi.FX_E_INVALID and faces.value == 77
    assert lib.fx_open_inflow(None, None) == capi.FX_E_INVALID


# ---- the anchor: faces = 0 is the obstacle reference, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(20, 20, 5), (36, 36, 1)])
def test_closed_walls_are_the_obstacle_reference(dims):
    X, Y, Z = dims
    rng = np.random.default_rng(401)
    vel = rng.standard_normal((3, Z, Y, X)).astype(f32)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    b = rng.standard_normal((Z, Y, X)).astype(f32)
    for m in (ob.random_mask(dims), np.zeros((Z, Y, X), np.uint8)):
        assert same_bits(orf.ref_jacobi(p, b, m, 0, 5), ob.ref_jacobi(p, b, m, 5))
        for half in (False, True):
            v = vel.astype(np.float16).astype(f32) if half else vel
            assert same_bits(orf.ref_project(v, p, m, 0, half), ob.ref_project(v, p, m, half))
    assert same_bits(orf.ref_jacobi(p, b, None, 0, 3), ob.ref_jacobi(p, b, np.zeros((Z, Y, X), np.uint8), 3))


def test_the_exact_fma_is_fmaf():
    """against the double rounding it is there to avoid: a product that lies a hair beside a float32 tie"""
    a, b = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12)                     # a * b = 1 + 2^-11 + 2^-24: exactly half an ulp above 1 + 2^-11 ...
    c = f32(2.0 ** -60)                                                  # ... and a hair more: fmaf rounds up, the float64 sum rounds to the tie first
    want = f32(1 + 2.0 ** -11 + 2.0 ** -23)
    twice = (np.float64(a) * np.float64(b) + np.float64(c)).astype(f32)    # the float64 sum rounded to float64, then to float32
    assert orf.fma(a, b, c) == want and twice != want
    assert orf.fma(a, b, -c) == f32(1 + 2.0 ** -11)
    import emitter_ref as er
    import fma_ref
    import maccormack_ref as mr
    import multigrid_ref as mg
    assert all(m.fma is fma_ref.fma for m in (orf, br, er, mr, mg))         # one fma for every model (tests/test_fma_ref.py: == libm's fmaf)


@pytest.mark.parametrize("dims", [(20, 20, 5), (36, 36, 1)])
def test_closed_walls_leave_the_heat_pass_alone(dims):
    X, Y, Z = dims
    rng = np.random.default_rng(409)
    T = rng.random((Z, Y, X)).astype(f32)
    v0 = (rng.standard_normal((3, Z, Y, X)) * 0.4).astype(f32)
    v1 = rng.standard_normal((3, Z, Y, X)).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    prm = br.params(ambient=0.25, density_weight=0.5, lift=2.0, cooling=0.3, up=(0.2, 1.0, -0.1))
    solid = ob.random_mask(dims, seed=5, p=0.1)
    for address in ("clamp", "mirror"):
        got = orf.heat_apply(T, v0, v1, col, prm, br.list_a(), 1 / 16, address, solid=solid, faces=0)
        want = br.apply(T, v0, v1, col, prm, br.list_a(), 1 / 16, address, solid=solid)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    some = orf.heat_apply(T, v0, v1, col, prm, [], 1 / 16, faces=orf.legal_faces(dims))
    none = br.apply(T, v0, v1, col, prm, [], 1 / 16)
    assert not same_bits(some[0], none[0])


# ---- the rules by hand --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(7, 6, 5), (7, 6, 1)])
def test_a_sweep_of_ones_counts_the_open_faces(dims):
    X, Y, Z = dims
    is3d = Z > 1
    n, inv = (6, orf.INV6) if is3d else (4, f32(0.25))
    p = np.ones((Z, Y, X), f32)
    for faces in orf.face_sets(dims) + [0]:
        q = orf.ref_jacobi(p, np.zeros_like(p), None, faces, 1)
        z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        k = ((x == 0) & bool(faces & 1)).astype(int) + ((x == X - 1) & bool(faces & 2)) + ((y == 0) & bool(faces & 4)) + ((y == Y - 1) & bool(faces & 8))
        if is3d:
            k = k + ((z == 0) & bool(faces & 16)) + ((z == Z - 1) & bool(faces & 32))
        want = (n - k).astype(f32) * inv                                  # the sum of n - k ones is exact in any order
        assert same_bits(q, want)
        assert q[Z // 2, Y // 2, X // 2] == f32(n) * inv
        if faces == orf.legal_faces(dims):
            assert k.max() == (3 if is3d else 2) and q[0, 0, 0] == f32(n - k.max()) * inv
    # a solid cell stays 0, and a solid neighbour still reads as the cell itself
    m = np.zeros((Z, Y, X), np.uint8)
    m[0, 2, 0] = 1
    q = orf.ref_jacobi(p, np.zeros_like(p), m, orf.X_LO, 1)
    assert q[0, 2, 0] == 0 and q[0, 1, 0] == f32(n - 1) * inv and q[0, 2, 1] == f32(n) * inv


def test_the_inflow_weights_by_hand():
    X, Y, Z = dims = (8, 6, 4)
    dt = f32(1 / 16)
    rng = np.random.default_rng(419)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    zero = np.zeros((3, Z, Y, X), f32)
    for faces in (orf.X_LO, orf.ALL_3D):
        assert (orf.inflow_weights(zero, dt, faces) == 1).all() and same_bits(orf.ref_inflow(col, zero, dt, faces), col)
    # u0_x * dt * X = 0.25: every trace moves a quarter cell towards x-; layer 0 samples 0.25 of the ghost
    vel = zero.copy()
    vel[0] = f32(0.25) / (dt * f32(X))
    w = orf.inflow_weights(vel, dt, orf.X_LO)
    fl, f = orf.trace(vel, dt, dims)[0]
    assert (fl[:, :, 0] == -1).all() and (w[:, :, 0] == f[:, :, 0]).all() and abs(float(w[0, 0, 0]) - 0.75) < 1e-6
    assert (w[:, :, 1:] == 1).all()
    assert (orf.inflow_weights(vel, dt, orf.ALL_3D & ~orf.X_LO) == 1).all()           # the other five faces: nothing
    out = orf.ref_inflow(col, vel, dt, orf.X_LO)
    assert same_bits(out[:, :, 1:], col[:, :, 1:]) and same_bits(out[:, :, 0], col[:, :, 0] * w[:, :, 0, None])
    assert (orf.inflow_weights(-vel, dt, orf.X_LO) == 1).all()                         # moving away from the face: nothing changes
    wh = orf.inflow_weights(-vel, dt, orf.X_HI)                                        # ... but x+ sees the same quarter
    assert (wh[:, :, :-1] == 1).all() and abs(float(wh[0, 0, -1]) - 0.75) < 1e-6
    # a trace two cells out and more samples the ghost alone (2.5 cells: t = y + 2.5)
    far = zero.copy()
    far[1] = f32(-2.5) / (dt * f32(Y))
    w = orf.inflow_weights(far, dt, orf.Y_HI)
    assert (w[:, -1] == 0).all() and (w[:, -2] == 0).all() and (w[:, -3] > 0).all() and (w[:, :-3] == 1).all()
    assert same_bits(orf.ref_inflow(col, far, dt, orf.Y_HI)[:, -1], np.zeros((Z, X, 4), f32))


def test_no_damping_towards_an_open_face():
    X, Y, Z = 8, 40, 4
    vel = np.zeros((3, Z, Y, X), f32)
    vel[1] = 1.0
    p = np.zeros((Z, Y, X), f32)
    y = Y - 1
    assert (y + 0.5) / Y * 2 - 1 > 0.94
    closed = orf.ref_project(vel, p, None, 0)
    opened = orf.ref_project(vel, p, None, orf.Y_HI)
    assert closed[1, 1, y, 3] < 1 and opened[1, 1, y, 3] == 1
    assert same_bits(orf.ref_project(vel, p, None, orf.Y_LO | orf.X_LO | orf.X_HI | orf.Z_LO | orf.Z_HI), closed)      # only the face it runs towards
    assert same_bits(orf.ref_project(-vel, p, None, orf.Y_HI), orf.ref_project(-vel, p, None, 0))      # moving down is damped at the floor as ever
    assert orf.ref_project(-vel, p, None, orf.Y_LO)[1, 1, 0, 3] == -1
    # the pressure ghost: p = 1 everywhere pushes the fluid out through an open face, and nowhere else
    out = orf.ref_project(np.zeros_like(vel), np.ones_like(p), None, orf.Y_HI)
    assert out[1, 1, y, 3] == orf.KD3 and not out[1, :, :y].any() and not out[0].any() and not out[2].any()


# ---- the plume ---------------------------------------------------------------------------------------------------------------------------
PLUME_DIMS, PLUME_DT, PLUME_ITERS, PLUME_ON, PLUME_STEPS = (32, 32, 32), 1 / 60, 40, 120, 240


def advect_without_impulse(vel, col, dt):
    """np_ref.advect minus its impulse: the trace, the sampler and the attenuation"""
    _, Z, Y, X = vel.shape
    dt = f32(dt)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    ax = ((x + 0.5) / X).astype(f32) - vel[0] * dt
    ay = ((y + 0.5) / Y).astype(f32) - vel[1] * dt
    az = ((z + 0.5) / Z).astype(f32) - vel[2] * dt
    u = np.stack([np_ref.trilinear(vel[a], ax, ay, az) for a in range(3)])
    c = np_ref.trilinear(col, ax, ay, az)
    atten = max(f32(1.0) - f32(0.2) * dt, f32(0.0))
    return (u * atten).astype(f32), (c * atten).astype(f32)


def plume_model(faces):
    """Sigma alpha behind steps PLUME_ON and PLUME_STEPS: np_ref's advection, then the inflow, the divergence, the sweeps and the projection"""
    X, Y, Z = PLUME_DIMS
    vel, col, p = np.zeros((3, Z, Y, X), f32), np.zeros((Z, Y, X, 4), f32), np.zeros((Z, Y, X), f32)
    sums = []
    for k in range(PLUME_STEPS):
        v1, c1 = np_ref.advect(vel, col, PLUME_DT) if k < PLUME_ON else advect_without_impulse(vel, col, PLUME_DT)
        if faces:
            c1 = orf.ref_inflow(c1, vel, PLUME_DT, faces)
        p = orf.ref_jacobi(p, np_ref.divergence(v1), None, faces, PLUME_ITERS)
        vel, col = orf.ref_project(v1, p, None, faces), c1
        if k + 1 in (PLUME_ON, PLUME_STEPS):
            sums.append(float(col[..., 3].astype(np.float64).sum()))
    return sums


def test_the_smoke_leaves_through_an_open_lid():
    o120, o240 = plume_model(orf.Y_HI)
    c120, c240 = plume_model(0)
    print("sum alpha  open: step 120 %.3f  step 240 %.3f   closed: step 120 %.3f  step 240 %.3f" % (o120, o240, c120, c240))
    assert o240 < 0.25 * o120
    assert c240 > 10 * o240
