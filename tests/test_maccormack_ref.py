"""CPU checks of the MacCormack advection (fx_set_advection_scheme): the numpy model tests/maccormack_ref.py against plain per-cell loops and
against its own limits (a constant field, a fluid at rest), what the scheme is for (a carried blob keeps its peak, the limiter keeps a step edge
inside its bounds), the C ABI surface without a device, and the register budget of the two kernels.  tests/test_gpu_maccormack.py holds the
kernels against this model."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import maccormack_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def small_state(dims, seed, cells=1.5):
    """velocities that carry a trace `cells` cells per axis (standard deviation): some leave the box on every side; a colour with -0 and 0 entries"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    dt = f32(0.05)
    vel = rng.standard_normal((3, Z, Y, X))
    for a, n in enumerate(dims):
        vel[a] *= cells / (float(dt) * n)
    col = (rng.random((Z, Y, X, 4)) * 2 - 0.5).astype(f32)
    col[0, 0, :2] = f32(-0.0)
    col[0, 1, :2] = f32(0.0)
    return vel.astype(f32), col, dt


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 8, 1)])
def test_model_equals_plain_loops(dims, address):
    vel, col, dt = small_state(dims, 701)
    for limit in (True, False):
        gv, gc = mr.step(vel, col, dt, address, impulse=False, limit=limit)
        wv, wc = mr.step_loops(vel, col, dt, address, limit=limit)
        assert same_bits(gv, wv) and same_bits(gc, wc), limit
    lim, unl = mr.step(vel, col, dt, address, impulse=False), mr.step(vel, col, dt, address, impulse=False, limit=False)
    assert not same_bits(lim[1], unl[1])                              # the limiter acts on this state
    assert not same_bits(lim[1], mr.step(vel, col, dt, address, impulse=False, scheme="semi-lagrangian")[1])


@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 8, 1)])
def test_a_constant_field_stays_itself(dims, address):
    vel, _, dt = small_state(dims, 709)
    X, Y, Z = dims
    for value in (f32(0.625), f32(-3.0), f32(0.0), f32(0.1)):         # (not -0: lerp(-0, -0, f) = fma(f, +0, -0) is +0 in either scheme)
        q = np.full((Z, Y, X), value, f32)
        for limit in (True, False):
            assert same_bits(mr.advect_field(q, vel, dt, address, limit), q), (value, limit)


@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("dims", [(8, 4, 4), (16, 8, 1)])
def test_a_fluid_at_rest_is_advected_as_by_the_semi_lagrangian_step(dims, address):
    """u0 = 0: both traces end on the cell itself, hat = bar = q and the correction vanishes.  (Power-of-two extents: ((x + .5) / N) * N - .5 is
    then x exactly; on other extents the trace of a cell at rest may land an ulp beside its centre, in both schemes.)"""
    _, col, dt = small_state(dims, 719)
    X, Y, Z = dims
    rest = np.zeros((3, Z, Y, X), f32)
    for impulse in (False, True):
        mc = mr.step(rest, col, dt, address, impulse=impulse)
        sl = mr.step(rest, col, dt, address, impulse=impulse, scheme="semi-lagrangian")
        assert same_bits(mc[0], sl[0]) and same_bits(mc[1], sl[1])


# ---- what the scheme is for -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", mr.CARRY_DIMS)
def test_a_carried_blob_keeps_its_peak(dims):
    """the issue's table: 32 x 32 x 8 0.997 -> 0.367 semi-Lagrangian against 0.799 MacCormack, 48 x 48 x 1 0.999 -> 0.489 against 0.900
    (this blob: 0.984 -> 0.366 / 0.812 and 0.993 -> 0.487 / 0.908)"""
    q = mr.blob(dims)
    sl, mc = mr.carry(q, dims, "semi-lagrangian"), mr.carry(q, dims, "maccormack")
    print("%s: peak %.3f -> semi-Lagrangian %.3f, MacCormack %.3f (ratio %.2f), minimum %.3g; without the limiter minimum %.3f"
          % (dims, q.max(), sl.max(), mc.max(), mc.max() / sl.max(), mc.min(), mr.carry(q, dims, "maccormack", limit=False).min()))
    assert mc.max() >= 1.5 * sl.max()
    assert mc.min() >= 0
    assert mc.max() <= q.max()                                        # the limiter: never above the data


@pytest.mark.parametrize("dims", mr.CARRY_DIMS)
def test_the_limiter_keeps_a_step_edge_within_its_bounds(dims):
    q = mr.edge(dims)
    assert q.min() == 0 and q.max() == 1
    mc, un = mr.carry(q, dims, "maccormack"), mr.carry(q, dims, "maccormack", limit=False)
    print("%s: limited [%.3g, %.3g], unlimited [%.3g, %.3g]" % (dims, mc.min(), mc.max(), un.min(), un.max()))
    assert mc.min() >= 0 and mc.max() <= 1
    assert un.max() > 1                                               # the limiter does something


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_with_the_scheme_calls(tmp_path):
    src = tmp_path / "scheme_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'static int (*set_)(fx_ctx*, uint32_t) = fx_set_advection_scheme;\n'
                   'static int (*get_)(fx_ctx*, uint32_t*) = fx_get_advection_scheme;\n'
                   'int main(void) { (void)set_; (void)get_; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        val = tmp_path / "scheme_values.c"                               # the constants, evaluated (the calls above need the library to link)
        val.write_text('#include "fluidx_hip.h"\nint main(void) { return FX_ADVECT_SEMI_LAGRANGIAN == 0u && FX_ADVECT_MACCORMACK == 1u && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(val), "-o", str(tmp_path / "values")], check=True)
        assert subprocess.run([str(tmp_path / "values")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_the_symbols_are_exported_and_mirrored():
    from fluidx12_amd import capi, build
    import fluidx12_amd as fx
    syms = subprocess.run(["nm", "-D", "--defined-only", build.ensure_built()], capture_output=True, text=True, check=True).stdout
    for name in ("fx_set_advection_scheme", "fx_get_advection_scheme"):
        assert re.search(r"\bT %s$" % name, syms, re.M), name
        assert name in capi.SYMBOLS
    assert capi.SYMBOLS["fx_set_advection_scheme"] == (C.c_int, [C.c_void_p, C.c_uint32])
    assert capi.SYMBOLS["fx_get_advection_scheme"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)])
    assert (capi.ADVECT_SEMI_LAGRANGIAN, capi.ADVECT_MACCORMACK) == (0, 1) and capi.ABI_VERSION == 7
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetAdvectionScheme", "GetAdvectionScheme"):
        assert callable(getattr(fx.Fluid, name))
        assert name in hpp, name
    assert "fx_set_advection_scheme" in hpp and "fx_get_advection_scheme" in hpp
    assert "-advection" in open(os.path.join(ROOT, "examples", "fluidx_demo.cpp")).read()
    assert "fx_maccormack.hip" in build.SOURCES


def test_a_null_context_is_refused():
    from fluidx12_amd import capi
    lib = capi.load()
    scheme = C.c_uint32(77)
    assert lib.fx_set_advection_scheme(None, 1) == capi.FX_E_INVALID and lib.fx_set_advection_scheme(None, 0) == capi.FX_E_INVALID
    assert lib.fx_get_advection_scheme(None, C.byref(scheme)) == capi.FX_E_INVALID and scheme.value == 77
    assert lib.fx_get_advection_scheme(None, None) == capi.FX_E_INVALID


# ---- the kernels' register budget -------------------------------------------------------------------------------------------------------------
def test_neither_kernel_spills(tmp_path):
    """fx_maccormack.hip compiled for gfx950 with the library's flags: every k_mc_* instantiation has a private segment of 0 bytes"""
    from fluidx12_amd import build as b
    source = "fx_maccormack.hip"
    out = tmp_path / (source + ".s")
    subprocess.check_call([b.hipcc()] + b.FLAGS + b.EXTRA_FLAGS.get(source, []) + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(b.CSRC, source), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        if "k_mc_" in m.group(1):
            found[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
    assert len(found) == 8 and sum("k_mc_predict" in k for k in found) == 4 and sum("k_mc_correct" in k for k in found) == 4, sorted(found)
    assert all(v == 0 for v in found.values()), found
