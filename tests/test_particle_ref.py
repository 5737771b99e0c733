"""CPU checks of the tracer particles (fx_set_particles, fx_sample_velocity): the C ABI surface without a device, the numpy model
tests/particle_ref.py against its plain-loop twin, its rules by hand, and the property the midpoint scheme is there for: particles in a
rigid rotation stay on their circle.  tests/test_gpu_particles.py holds the kernels against this model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import buoyancy_ref as br
import particle_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CALLS = ("fx_set_particles", "fx_get_particles", "fx_particles_device", "fx_set_particle_params", "fx_get_particle_params", "fx_move_particles",
         "fx_sample_velocity")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx_with_the_particle_calls(tmp_path):
    src = tmp_path / "particle_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'typedef char size_is_28[sizeof(fx_particle_params) == 28 ? 1 : -1];\n'
                   'static int (*set_)(fx_ctx*, void*, const float*, uint32_t, uint32_t) = fx_set_particles;\n'
                   'static int (*get_)(fx_ctx*, float*, uint32_t, uint32_t*) = fx_get_particles;\n'
                   'static int (*dev_)(fx_ctx*, void**, uint32_t*) = fx_particles_device;\n'
                   'static int (*setp_)(fx_ctx*, const fx_particle_params*) = fx_set_particle_params;\n'
                   'static int (*getp_)(fx_ctx*, fx_particle_params*) = fx_get_particle_params;\n'
                   'static int (*move_)(fx_ctx*, void*) = fx_move_particles;\n'
                   'static int (*samp_)(fx_ctx*, void*, const float*, uint32_t, float*, uint32_t) = fx_sample_velocity;\n'
                   'int main(void) { (void)set_; (void)get_; (void)dev_; (void)setp_; (void)getp_; (void)move_; (void)samp_; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        val = tmp_path / "particle_values.c"                             # the constants, evaluated (the calls above need the library to link)
        val.write_text('#include "fluidx_hip.h"\nint main(void) { return sizeof(fx_particle_params) == 28 && FX_MAX_PARTICLES == (1u << 26) && '
                       'FX_PARTICLES_DEVICE == 0x1u && FX_PARTICLE_EULER == 0u && FX_PARTICLE_MIDPOINT == 1u && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(val), "-o", str(tmp_path / "values")], check=True)
        assert subprocess.run([str(tmp_path / "values")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_symbols_are_exported_and_mirrored():
    from fluidx12_amd import capi, build
    import fluidx12_amd as fx
    lib = capi.load()
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    for name in CALLS:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert capi.SYMBOLS["fx_set_particles"] == (C.c_int, [vp, vp, fp, C.c_uint32, C.c_uint32])
    assert capi.SYMBOLS["fx_sample_velocity"] == (C.c_int, [vp, vp, fp, C.c_uint32, fp, C.c_uint32])
    assert capi.SYMBOLS["fx_set_particle_params"][1][1:] == [C.POINTER(capi.ParticleParams)]
    assert C.sizeof(capi.ParticleParams) == 28 and capi.ABI_VERSION == 7
    assert (capi.MAX_PARTICLES, capi.PARTICLES_DEVICE, capi.PARTICLE_EULER, capi.PARTICLE_MIDPOINT) == (1 << 26, 1, 0, 1)
    assert (pr.EULER, pr.MIDPOINT) == (capi.PARTICLE_EULER, capi.PARTICLE_MIDPOINT)
    assert (pr.X_LO, pr.X_HI, pr.Y_LO, pr.Y_HI, pr.Z_LO, pr.Z_HI) == (capi.WALL_X_LO, capi.WALL_X_HI, capi.WALL_Y_LO, capi.WALL_Y_HI, capi.WALL_Z_LO, capi.WALL_Z_HI)
    members = ("SetParticles", "GetParticles", "ParticlesDevice", "SetParticleParams", "GetParticleParams", "MoveParticles", "SampleVelocity")
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in members:
        assert callable(getattr(fx.Fluid, name)) and name in hpp, name
    for name in CALLS:
        assert name in hpp, name
    assert "fx_particles.hip" in build.SOURCES


def test_a_null_context_is_refused():
    from fluidx12_amd import capi
    lib = capi.load()
    n, p = C.c_uint32(77), C.c_void_p(5)
    rec = (C.c_float * 4)(0.5, 0.5, 0.5, 0.0)
    prm = capi.ParticleParams()
    assert lib.fx_set_particles(None, None, rec, 1, 0) == capi.FX_E_INVALID and lib.fx_set_particles(None, None, None, 0, 0) == capi.FX_E_INVALID
    assert lib.fx_get_particles(None, rec, 1, C.byref(n)) == capi.FX_E_INVALID and n.value == 77
    assert lib.fx_particles_device(None, C.byref(p), C.byref(n)) == capi.FX_E_INVALID and (p.value, n.value) == (5, 77)
    assert lib.fx_set_particle_params(None, C.byref(prm)) == capi.FX_E_INVALID and lib.fx_get_particle_params(None, C.byref(prm)) == capi.FX_E_INVALID
    assert lib.fx_move_particles(None, None) == capi.FX_E_INVALID
    assert lib.fx_sample_velocity(None, None, rec, 1, rec, 0) == capi.FX_E_INVALID and lib.fx_sample_velocity(None, None, None, 0, None, 0) == capi.FX_E_INVALID


# ---- the model against its twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(7, 7, 5), (9, 9, 1)])
def test_the_vectorised_model_is_the_loop_model(dims):
    dt = 1 / 16
    vel = pr.velocity(dims, 3, dt=dt)
    pts = pr.points(dims, 120, 5)
    assert same_bits(pr.sample(vel, pts), pr.sample_loops(vel, pts))
    rec = pr.records(dims, 120, 7)
    faces_all = 0x3F if dims[2] > 1 else 0x0F
    for scheme in (pr.EULER, pr.MIDPOINT):
        prm = pr.params(scheme=scheme, drift=(0.01, -0.3, 0.02), lifetime=0.55)
        for faces, solid in ((0, None), (pr.X_HI | pr.Y_LO, None), (faces_all, pr.box_mask(dims)), (0, pr.box_mask(dims))):
            a, b = pr.move(rec, vel, dt, prm, faces, solid), pr.move_loops(rec, vel, dt, prm, faces, solid)
            assert same_bits(a, b), (scheme, faces)
            dead_in = ~(rec[:, 3] >= 0)
            assert dead_in.any() and same_bits(a[dead_in], rec[dead_in])            # a dead record keeps every bit, NaN ages included
            assert (a[~dead_in, 3] == -1).any() and (a[~dead_in, 3] > 0).any()     # the lifetime kills some and not others


# ---- the rules by hand ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(8, 8, 4), (16, 16, 1)])
def test_a_linear_field_comes_back_exactly_at_cell_centres(dims):
    """(extents that are powers of two: the centres, the field's values there and every product below are then exact in fp32)"""
    X, Y, Z = dims
    px, py, pz = br.cell_centres(dims)

    def lin(x, y, z):
        return np.stack([(2 * x + 0.25 * y - z).astype(f32), (y * 4).astype(f32), (x - y).astype(f32)])
    vel = lin(px, py, pz)
    pts = np.stack([px.ravel(), py.ravel(), pz.ravel()], axis=1)
    assert same_bits(pr.sample(vel, pts), vel.reshape(3, -1).T)
    # ... and half-way between two centres along x (a cell face) it is the linear function there
    face = pts[pts[:, 0] > 1 / X].copy()
    face[:, 0] -= f32(0.5 / X)
    assert same_bits(pr.sample(vel, face), lin(face[:, 0], face[:, 1], face[:, 2]).T)


def test_the_clamp_by_hand():
    assert same_bits(pr.c01(np.array([np.nan, -np.inf, -0.3, -0.0, 0.0, 0.25, 1.0, 1.7, 1e30, np.inf], f32)),
                     np.array([0, 0, 0, 0, 0, 0.25, 1, 1, 1, 1], f32))
    vel = pr.velocity((5, 5, 3), 11)
    wild = np.array([[np.nan, -np.inf, 1e30], [np.inf, np.nan, -5.0]], f32)
    tame = np.array([[0, 0, 1], [1, 0, 0]], f32)
    assert same_bits(pr.sample(vel, wild), pr.sample(vel, tame))
    assert same_bits(pr.sample(vel, tame)[0], vel[:, 2, 0, 0])                      # a corner of the box reads the corner cell


def test_walls_obstacles_and_age_by_hand():
    dims, dt = (8, 8, 4), f32(0.25)
    vel = np.zeros((3, 4, 8, 8), f32)
    vel[0] = 1.0                                                                     # a quarter of the box per step towards x+
    rec = np.array([[0.5, 0.5, 0.5, 0.0], [0.9, 0.5, 0.5, 1.0], [0.9, 0.5, 0.5, -2.0]], f32)
    for scheme in (pr.EULER, pr.MIDPOINT):
        out = pr.move(rec, vel, dt, pr.params(scheme=scheme))
        assert same_bits(out, np.array([[0.75, 0.5, 0.5, 0.25], [1.0, 0.5, 0.5, 1.25], [0.9, 0.5, 0.5, -2.0]], f32))   # the closed wall holds it
    out = pr.move(rec, vel, dt, faces=pr.X_HI)
    assert same_bits(out[1], np.array([1.0, 0.5, 0.5, -1.0], f32)) and out[0, 3] == 0.25                              # the open one lets it go
    assert same_bits(pr.move(rec, vel, dt, faces=0x3F & ~pr.X_HI), pr.move(rec, vel, dt))                             # ... and only that one
    solid = np.zeros((4, 8, 8), np.uint8)
    solid[2, 4, 6] = 1                                                               # the cell of (0.75, 0.5, 0.5)
    out = pr.move(rec, vel, dt, solid=solid)
    assert same_bits(out[0], np.array([0.5, 0.5, 0.5, 0.25], f32)) and out[1, 0] == 1.0                               # stays put, still ages
    out = pr.move(rec, vel, dt, pr.params(lifetime=1.25))
    assert out[0, 3] == 0.25 and same_bits(out[1], np.array([1.0, 0.5, 0.5, -1.0], f32))                              # age1 >= lifetime
    out = pr.move(rec, vel, dt, pr.params(drift=(-1.0, 0.0, 0.5)))
    assert same_bits(out[0], np.array([0.5, 0.5, 0.625, 0.25], f32))
    flat = pr.move(np.array([[0.5, 0.5, 7.0, 0.0], [0.5, 0.5, np.nan, 0.0]], f32), vel[:, :1] + 1, dt, pr.params(drift=(0, 0, 3.0)))
    assert same_bits(flat[:, 2], np.array([7.0, np.nan], f32)) and (flat[:, 0] == 1.0).all()                          # a 2-D grid leaves z alone


# ---- what the midpoint scheme is for -------------------------------------------------------------------------------------------------------
def test_midpoint_keeps_a_rigid_rotation_on_its_circle():
    """64 particles on the circle of radius 0.25 in a rigid rotation on 32 x 32 x 1, omega dt = 0.1, 50 steps.  Euler's radius grows by
    sqrt(1 + (omega dt)^2) per step, the midpoint scheme's by sqrt(1 + (omega dt)^4 / 4): the ratio of the errors is (omega dt)^2 / 4 =
    0.0025, held here to 1 / 100.  Measured on this model: Euler 0.28, midpoint 6.3e-4."""
    e, m = pr.radius_error(pr.EULER), pr.radius_error(pr.MIDPOINT)
    print("largest relative radius error behind 50 steps: Euler %.3g, midpoint %.3g, ratio %.3g" % (e, m, m / e))
    assert 0.2 < e < 0.35
    assert m <= e / 100
