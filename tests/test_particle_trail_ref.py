"""CPU checks of the particle trail (fx_set_particle_trail, fx_deposit_particles, fx_particle_density): the numpy model
tests/particle_trail_ref.py against its plain-loop twin, the rule by hand, the C ABI surface without a device, and the kernels' register budget.
tests/test_gpu_particle_trails.py holds the kernels against the model."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import particle_ref as pr
import particle_trail_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CALLS = ("fx_set_particle_trail", "fx_get_particle_trail", "fx_deposit_particles", "fx_particle_density")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def live_count(rec):
    return int(tr.live_of(rec).sum())


# ---- the model against its twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 4, 1), (5, 3, 2), (1, 1, 1)])
def test_the_vectorised_scatter_is_the_loop_scatter(dims):
    for name in tr.ARRANGEMENTS:
        for n in (1, 2, 97):
            rec = tr.arrangement(name, dims, n, seed=n)
            a, b = tr.density(rec, dims), tr.density_loops(rec, dims)
            assert a.dtype == np.uint64 and a.shape == dims[::-1] and np.array_equal(a, b), (name, n)
            assert int(a.sum()) == live_count(rec) << 24, (name, n)


@pytest.mark.parametrize("dims", [(20, 20, 12), (36, 36, 1), (3, 3, 2)])
def test_every_live_record_adds_exactly_two_to_the_24(dims):
    e = pr.edge_points(dims)
    rec = np.zeros((len(e), 4), f32)
    rec[:, :3] = e
    assert int(tr.density(rec, dims).sum()) == len(e) << 24
    for k in range(len(e)):                                                # ... each one of them on its own, 0, 1, -0, -0.3, 1.7, +-inf, NaN, 1e30 included
        assert int(tr.density(rec[k:k + 1], dims).sum()) == 1 << 24, e[k]
    for name in tr.ARRANGEMENTS:
        rec = tr.arrangement(name, dims, 4099, seed=3)
        assert int(tr.density(rec, dims).sum()) == live_count(rec) << 24, name
    dead = tr.arrangement("dead5", dims, 100, seed=1)
    assert live_count(dead) == 80


def test_the_scatter_by_hand():
    dims = (8, 4, 2)
    X, Y, Z = dims

    def one(x, y, z, age=0.0):
        return tr.density(np.array([[x, y, z, age]], f32), dims)
    # a cell centre: 2^24 into that cell alone
    a = one(4.5 / X, 2.5 / Y, 1.5 / Z)
    assert a[1, 2, 4] == 1 << 24 and np.count_nonzero(a) == 1
    # a face centre between cells 3 and 4 along x: 2^23 into each
    a = one(4.0 / X, 2.5 / Y, 0.5 / Z)
    assert a[0, 2, 3] == 1 << 23 and a[0, 2, 4] == 1 << 23 and np.count_nonzero(a) == 2
    # position 0: both taps of every axis clamp onto cell 0
    a = one(0.0, 0.0, 0.0)
    assert a[0, 0, 0] == 1 << 24 and np.count_nonzero(a) == 1
    a = one(1.0, np.inf, 1e30)
    assert a[Z - 1, Y - 1, X - 1] == 1 << 24 and np.count_nonzero(a) == 1
    a = one(np.nan, -np.inf, -0.0)
    assert a[0, 0, 0] == 1 << 24 and np.count_nonzero(a) == 1
    # a quarter of a cell beyond a centre: 192 : 64
    a = one(4.75 / X, 2.5 / Y, 1.5 / Z)
    assert a[1, 2, 4] == 192 << 16 and a[1, 2, 5] == 64 << 16 and np.count_nonzero(a) == 2
    # -0.0 is live; a negative or NaN age adds nothing
    assert int(one(0.3, 0.3, 0.3, -0.0).sum()) == 1 << 24
    for age in (-1.0, -1e-45, np.nan, -np.inf):
        assert not one(0.3, 0.3, 0.3, age).any()
    # a 2-D grid does not look at z
    flat = (8, 4, 1)
    a = tr.density(np.array([[4.5 / 8, 2.5 / 4, 0.9, 0.0], [4.5 / 8, 2.5 / 4, np.nan, 0.0]], f32), flat)
    assert a[0, 2, 4] == 2 << 24 and np.count_nonzero(a) == 1
    # 64-bit words: 4099 records in one cell pass 2^32
    dims = (20, 20, 12)
    a = tr.density(tr.arrangement("one_cell", dims, 4099, seed=1), dims)
    assert int(a.max()) > 1 << 32 and int(a.max()) & 0xFFFF and np.count_nonzero(a) == 8
    assert len(np.unique(tr.base_cell(tr.arrangement("one_cell", dims, 4099, seed=1), dims), axis=0)) == 1
    two = tr.base_cell(tr.arrangement("two_cells", dims, 257, seed=1), dims)
    assert (two[1:] != two[:-1]).any(axis=1).all()                         # every run has length 1


# ---- the apply rule ------------------------------------------------------------------------------------------------------------------------
def test_the_integer_conversion_rounds_to_nearest_even():
    cases = [0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, (1 << 32) + (1 << 7), (1 << 32) + (1 << 8),
             (1 << 32) + (1 << 8) + 1, (1 << 33) + (3 << 8), 8683970560 + 12345, (1 << 50) - 1, (1 << 50) + (1 << 26) + 1, (1 << 64) - 1]
    got = tr.amount(np.array(cases, np.uint64))
    want = np.array([tr.to_f32_rne(v) * f32(2.0 ** -24) for v in cases], f32)
    assert same_bits(got, want)
    assert tr.to_f32_rne((1 << 24) + 1) == f32(1 << 24) and tr.to_f32_rne((1 << 24) + 3) == f32((1 << 24) + 4)      # ties to even, both ways
    assert tr.amount(np.array([1 << 24], np.uint64))[0] == 1.0


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 4, 1)])
def test_the_vectorised_apply_is_the_loop_apply(dims, half):
    rec = np.concatenate([tr.arrangement("random", dims, 5, seed=2), tr.arrangement("one_cell", dims, 3000, seed=2)])
    acc = tr.density(rec, dims)
    col, temp = tr.fields(dims, 11, half)
    solid = pr.box_mask(dims)
    t = tr.trail(rate=3.0, tint=(0.25, -0.5, 0.125, 0.7), heat=-2.5)
    dt = pr.time_step(dims)
    for kw in (dict(), dict(temp=temp), dict(temp=temp, solid=solid)):
        a, b = tr.apply(acc, col, dt, t, half=half, **kw), tr.apply_loops(acc, col, dt, t, half=half, **kw)
        assert same_bits(a[0], b[0]) and (a[1] is None) == (b[1] is None) == ("temp" not in kw)
        if a[1] is not None:
            assert same_bits(a[1], b[1]) and not same_bits(a[1], temp)
        out = a[0]
        untouched = acc == 0
        assert untouched.any() and same_bits(out[untouched], col[untouched])                   # -0 included: the bits stay
        assert (np.signbit(col[untouched][:, 3]) & (col[untouched][:, 3] == 0)).any()
        hit = ~untouched if "solid" not in kw else ~untouched & (solid == 0)
        assert (out[hit] != col[hit]).any(axis=-1).all()
        if "solid" in kw:
            inside = (solid != 0) & ~untouched
            assert inside.any() and same_bits(out[inside], col[inside]) and same_bits(a[1][inside], temp[inside])
        if half:                                                                                 # rounded once: the stored values are binary16's
            assert same_bits(out, out.astype(np.float16).astype(f32))
            exact = tr.apply(acc, col, dt, t, half=False, **kw)[0]
            assert same_bits(out, exact.astype(np.float16).astype(f32)) and not same_bits(out, exact)
    # heat = 0 leaves the temperature alone
    assert same_bits(tr.apply(acc, col, dt, tr.trail(rate=3.0, tint=(1, 1, 1, 1)), temp=temp)[1], temp)


def test_the_alpha_sum_is_the_amount_deposited():
    dims = (20, 20, 12)
    rec = tr.arrangement("dead5", dims, 4099, seed=5)
    t = tr.trail(rate=2.0, tint=(0.0, 0.0, 0.0, 0.75))
    dt = pr.time_step(dims)
    out, _ = tr.apply(tr.density(rec, dims), np.zeros(dims[::-1] + (4,), f32), dt, t)
    want = live_count(rec) * (float(f32(2.0) * dt) * 0.75)
    assert abs(out[..., 3].astype(np.float64).sum() / want - 1) < 1e-6


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx_with_the_trail_calls(tmp_path):
    src = tmp_path / "trail_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'typedef char trail_is_32[sizeof(fx_particle_trail) == 32 ? 1 : -1];\n'
                   'static int (*set_)(fx_ctx*, const fx_particle_trail*) = fx_set_particle_trail;\n'
                   'static int (*get_)(fx_ctx*, fx_particle_trail*) = fx_get_particle_trail;\n'
                   'static int (*dep_)(fx_ctx*, void*) = fx_deposit_particles;\n'
                   'static int (*den_)(fx_ctx*, void*, uint64_t*, size_t) = fx_particle_density;\n'
                   'int main(void) { (void)set_; (void)get_; (void)dep_; (void)den_; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        val = tmp_path / "trail_values.c"
        val.write_text('#include "fluidx_hip.h"\nint main(void) { return sizeof(fx_particle_trail) == 32 && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(val), "-o", str(tmp_path / "values")], check=True)
        assert subprocess.run([str(tmp_path / "values")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_symbols_are_exported_and_mirrored():
    from fluidx12_amd import capi, build
    import fluidx12_amd as fx
    lib = capi.load()
    vp = C.c_void_p
    for name in CALLS:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert capi.SYMBOLS["fx_set_particle_trail"] == (C.c_int, [vp, C.POINTER(capi.ParticleTrail)])
    assert capi.SYMBOLS["fx_get_particle_trail"] == (C.c_int, [vp, C.POINTER(capi.ParticleTrail)])
    assert capi.SYMBOLS["fx_deposit_particles"] == (C.c_int, [vp, vp])
    assert capi.SYMBOLS["fx_particle_density"] == (C.c_int, [vp, vp, C.POINTER(C.c_uint64), C.c_size_t])
    assert C.sizeof(capi.ParticleTrail) == 32 and capi.ABI_VERSION == 7
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetParticleTrail", "GetParticleTrail", "DepositParticles", "ParticleDensity"):
        assert callable(getattr(fx.Fluid, name)) and name in hpp, name
    for name in CALLS:
        assert name in hpp, name
    assert "fx_particle_trail.hip" in build.SOURCES
    assert "TRAIL_MERGE" in capi.LAB_KNOBS and "TRAIL_MERGE" not in capi.knob_names()          # the shipped switch list does not grow


def test_a_null_context_is_refused():
    from fluidx12_amd import capi
    lib = capi.load()
    t = capi.ParticleTrail(32, 0, 1.5, (C.c_float * 4)(1, 2, 3, 4), 5.0)
    word = (C.c_uint64 * 1)(77)
    assert lib.fx_set_particle_trail(None, C.byref(t)) == capi.FX_E_INVALID and lib.fx_set_particle_trail(None, None) == capi.FX_E_INVALID
    assert lib.fx_get_particle_trail(None, C.byref(t)) == capi.FX_E_INVALID and (t.rate, tuple(t.tint), t.heat) == (1.5, (1, 2, 3, 4), 5.0)
    assert lib.fx_get_particle_trail(None, None) == capi.FX_E_INVALID
    assert lib.fx_deposit_particles(None, None) == capi.FX_E_INVALID
    assert lib.fx_particle_density(None, None, word, 8) == capi.FX_E_INVALID and word[0] == 77
    assert lib.fx_particle_density(None, None, None, 0) == capi.FX_E_INVALID


# ---- the kernels' register budget ------------------------------------------------------------------------------------------------------------
def test_no_trail_kernel_spills(tmp_path):
    """fx_particle_trail.hip compiled for gfx950 with the library's flags: every k_trail_* instantiation has a private segment of 0 bytes"""
    from fluidx12_amd import build as b
    source = "fx_particle_trail.hip"
    out = tmp_path / (source + ".s")
    subprocess.check_call([b.hipcc()] + b.FLAGS + b.EXTRA_FLAGS.get(source, []) + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(b.CSRC, source), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        if "k_trail_" in m.group(1):
            found[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
    # splat: IS3D x WIDE x MERGE; apply: HALF x WIDE
    assert len(found) == 12 and sum("k_trail_splat" in k for k in found) == 8 and sum("k_trail_apply" in k for k in found) == 4, sorted(found)
    assert all(v == 0 for v in found.values()), found
