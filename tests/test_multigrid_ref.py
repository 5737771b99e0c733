"""CPU checks of the multigrid pressure solver (fx_set_pressure_solver): the numpy model tests/multigrid_ref.py against plain per-cell loops
and against what it must reduce to (omega = 1 is the Jacobi sweep, a fixed point has no residual, a constant prolongs to itself), the level
planner of csrc/fx_multigrid_plan.cpp linked into a small program, the C ABI surface without a device, what the solver is for (one solve leaves
less than half of what 40 Jacobi sweeps leave) and the register budget of the kernels.  tests/test_gpu_multigrid.py holds the kernels against
this model."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import multigrid_ref as mg
import open_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(bits(a), bits(b))


def fields(dims, seed):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    b = rng.standard_normal((Z, Y, X)).astype(f32)
    p[0, 0, :2] = f32(-0.0)
    b[0, 1, :2] = f32(0.0)
    return p, b


# ---- the model against plain loops --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(8, 6, 4), (6, 4, 5), (10, 8, 1)])
def test_smooth_and_residual_equal_plain_loops(dims):
    p, b = fields(dims, 811)
    for omega in (f32(6.0 / 7.0), f32(1.0), f32(0.8)):
        assert same_bits(mg.smooth(p, b, omega), mg.smooth_loops(p, b, omega)), omega
    assert same_bits(mg.residual(p, b), mg.residual_loops(p, b))
    assert same_bits(mg.smooth(np.zeros_like(p), b, f32(0.8)), mg.smooth_loops(np.zeros_like(p), b, f32(0.8)))


@pytest.mark.parametrize("dims", [(8, 6, 4), (12, 4, 8), (10, 8, 1)])
def test_restrict_and_prolong_equal_plain_loops(dims):
    X, Y, Z = dims
    r, _ = fields(dims, 821)
    c = mg.restrict(r)
    assert c.shape == (Z // 2 if Z > 1 else 1, Y // 2, X // 2)
    assert same_bits(c, mg.restrict_loops(r))
    assert same_bits(mg.prolong(c, r.shape), mg.prolong_loops(c, r.shape))


# ---- what the rules must reduce to --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(9, 7, 5), (11, 6, 1)])
def test_omega_one_is_the_jacobi_sweep(dims):
    """p' = fma(1, J - p, p) is J bit for bit wherever J - p is exact (Sterbenz: p / 2 <= J <= 2 p): pressures in [1, 2) and a small
    right-hand side keep every J in [1 - 1/64, 2).  (Outside that regime J - p rounds on its own and the damped form differs in the last bit.)"""
    X, Y, Z = dims
    rng = np.random.default_rng(823)
    p = (1.0 + rng.random((Z, Y, X))).astype(f32)
    b = ((rng.random((Z, Y, X)) - 0.5) / 16).astype(f32)
    for n in (1, 3):
        assert same_bits(mg.smooth(p, b, f32(1.0), n), open_ref.ref_jacobi(p, b, None, 0, n)), n


@pytest.mark.parametrize("dims", [(8, 6, 4), (10, 8, 1)])
def test_an_exact_fixed_point_has_no_residual(dims):
    X, Y, Z = dims
    p = np.random.default_rng(827).integers(-9, 10, (Z, Y, X)).astype(f32)
    zero = np.zeros_like(p)
    b = -mg.residual(p, zero)                                         # S - 6 p: small integers, exact
    assert same_bits(mg.residual(p, b), zero)
    assert same_bits(mg.restrict(mg.residual(p, b)), np.zeros(mg.restrict(zero).shape, f32))


@pytest.mark.parametrize("dims", [(8, 6, 4), (12, 4, 8), (10, 8, 1)])
def test_a_constant_correction_prolongs_to_itself(dims):
    X, Y, Z = dims
    for value in (f32(0.625), f32(-3.0), f32(0.1), f32(0.0)):
        c = np.full((Z // 2 if Z > 1 else 1, Y // 2, X // 2), value, f32)
        assert same_bits(mg.prolong(c, (Z, Y, X)), np.full((Z, Y, X), value, f32)), value


def test_one_level_is_damped_sweeps():
    dims = (37, 53, 1)
    p, b = fields(dims, 829)
    prm = mg.defaults(dims)
    got, levels = mg.solve(p, b)
    assert levels == [None]
    assert same_bits(got, mg.smooth(p, b, prm["omega"], prm["cycles"] * prm["coarse"]))


# ---- the level planner ----------------------------------------------------------------------------------------------------------------------------
PROBE = r'''
#include "fx_internal.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
	if (argc != 5) return 2;
	fx::Geom g = {};
	g.X = atoi(argv[1]); g.Y = atoi(argv[2]); g.Zg = g.nz = atoi(argv[3]);
	g.zhi = g.Zg - 1;
	fx::MgPlan p;
	const int n = fx::mg_plan(g, (unsigned)atoi(argv[4]), &p);
	std::printf("%d %d %d", n, p.tail, p.tail_floats);
	for (int l = 0; l < p.levels; ++l) std::printf(" %d %d %d", p.lv[l].X, p.lv[l].Y, p.lv[l].Z);
	std::printf("\n");
	return n == p.levels ? 0 : 1;
}
'''


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """fx_multigrid_plan.cpp linked into a small program, compiled as the library's sources are"""
    from fluidx12_amd import build
    d = tmp_path_factory.mktemp("mg_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run([build.hipcc()] + build.FLAGS + ["-I", build.CSRC, "-x", "hip", str(src), os.path.join(build.CSRC, "fx_multigrid_plan.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)

    def call(dims, cap=0):
        v = [int(t) for t in subprocess.run([str(exe)] + [str(n) for n in dims] + [str(cap)], check=True, capture_output=True, text=True).stdout.split()]
        return {"levels": [tuple(v[3 + 3 * l:6 + 3 * l]) for l in range(v[0])], "tail": v[1], "tail_floats": v[2]}
    return call


PLANS = {
    (256, 256, 256): [(256,) * 3, (128,) * 3, (64,) * 3, (32,) * 3, (16,) * 3, (8,) * 3, (4,) * 3, (2,) * 3],
    (150, 150, 150): [(150, 150, 150), (75, 75, 75)],
    (24, 40, 72): [(24, 40, 72), (12, 20, 36), (6, 10, 18), (3, 5, 9)],
    (64, 64, 4): [(64, 64, 4), (32, 32, 2)],
    (16, 16, 2): [(16, 16, 2)],
    (37, 53, 1): [(37, 53, 1)],
    (36, 36, 1): [(36, 36, 1), (18, 18, 1), (9, 9, 1)],
}


@pytest.mark.parametrize("dims", sorted(PLANS))
def test_the_planner_halves_even_extents_of_at_least_four(planner, dims):
    """written out by hand from the rule: a level is halved while every extent that would be halved is even and >= 4 (256^3 therefore ends at
    2^3, 150^3 at 75^3; 64 x 64 x 4 stops at Z = 2, 16 x 16 x 2 is not coarsened at all; a 2-D grid keeps Z = 1)"""
    got = planner(dims)
    assert got["levels"] == PLANS[dims]
    assert mg.plan(dims) == PLANS[dims]
    for cap in (1, 2):
        assert planner(dims, cap)["levels"] == PLANS[dims][:cap] == mg.plan(dims, cap)
    assert got["tail"] == mg.tail_level(PLANS[dims])


def test_the_tail_starts_at_the_first_level_of_at_most_4096_cells(planner):
    assert planner((256, 256, 256))["tail"] == 4                      # 16^3
    assert planner((32, 32, 32))["tail"] == 1                         # 16^3
    assert planner((32, 32, 32))["tail_floats"] == 4096 + 2 * (4096 + 512 + 64 + 8)
    assert planner((128, 128, 1))["tail"] == 1                        # 64^2 = 4096 exactly
    assert planner((256, 256, 1))["tail"] == 2
    assert planner((150, 150, 150))["tail"] == 0                      # 75^3 is the last level and too large
    assert planner((32, 32, 32), 1)["tail"] == 0
    assert planner((20, 12, 8))["tail"] == 1


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_with_the_solver_calls(tmp_path):
    src = tmp_path / "solver_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'static int (*set_)(fx_ctx*, const fx_pressure_solver*) = fx_set_pressure_solver;\n'
                   'static int (*get_)(fx_ctx*, fx_pressure_solver*) = fx_get_pressure_solver;\n'
                   'static int (*solve_)(fx_ctx*, void*) = fx_pressure_solve;\n'
                   'static int (*level_)(fx_ctx*, uint32_t, int, void*, size_t) = fx_download_pressure_level;\n'
                   'int main(void) { (void)set_; (void)get_; (void)solve_; (void)level_; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") or shutil.which("g++")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        val = tmp_path / "solver_values.c"
        val.write_text('#include "fluidx_hip.h"\n#include <stddef.h>\nint main(void) { return sizeof(fx_pressure_solver) == 32 && offsetof(fx_pressure_solver, omega) == 28 '
                       '&& FX_PRESSURE_JACOBI == 0u && FX_PRESSURE_MULTIGRID == 1u && FX_MG_NO_TAIL == 0x1u && FX_MG_MAX_LEVELS == 12u && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(val), "-o", str(tmp_path / "values")], check=True)
        assert subprocess.run([str(tmp_path / "values")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_the_symbols_are_exported_and_mirrored():
    from fluidx12_amd import capi, build
    import fluidx12_amd as fx
    syms = subprocess.run(["nm", "-D", "--defined-only", build.ensure_built()], capture_output=True, text=True, check=True).stdout
    names = ("fx_set_pressure_solver", "fx_get_pressure_solver", "fx_pressure_solve", "fx_download_pressure_level")
    for name in names:
        assert re.search(r"\bT %s$" % name, syms, re.M), name
        assert name in capi.SYMBOLS
    ps = C.POINTER(capi.PressureSolver)
    assert capi.SYMBOLS["fx_set_pressure_solver"] == (C.c_int, [C.c_void_p, ps]) and capi.SYMBOLS["fx_get_pressure_solver"] == (C.c_int, [C.c_void_p, ps])
    assert capi.SYMBOLS["fx_pressure_solve"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert capi.SYMBOLS["fx_download_pressure_level"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t])
    assert C.sizeof(capi.PressureSolver) == 32 and capi.PressureSolver.omega.offset == 28
    assert (capi.PRESSURE_JACOBI, capi.PRESSURE_MULTIGRID, capi.MG_NO_TAIL, capi.MG_MAX_LEVELS) == (0, 1, 1, 12) and capi.ABI_VERSION == 7
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetPressureSolver", "GetPressureSolver", "PressureSolve", "DownloadPressureLevel"):
        assert callable(getattr(fx.Fluid, name))
        assert name in hpp, name
    for name in names:
        assert name in hpp, name
    assert "-multigrid" in open(os.path.join(ROOT, "examples", "fluidx_demo.cpp")).read()
    assert "fx_multigrid.hip" in build.SOURCES and "fx_multigrid_plan.cpp" in build.SOURCES


def test_a_null_context_is_refused():
    from fluidx12_amd import capi
    lib = capi.load()
    ps = capi.PressureSolver(capi.PRESSURE_MULTIGRID, 0, 2, 2, 2, 16, 0, 0.8)
    buf = (C.c_float * 4)()
    assert lib.fx_set_pressure_solver(None, C.byref(ps)) == capi.FX_E_INVALID and lib.fx_set_pressure_solver(None, None) == capi.FX_E_INVALID
    assert lib.fx_get_pressure_solver(None, C.byref(ps)) == capi.FX_E_INVALID and ps.cycles == 2
    assert lib.fx_pressure_solve(None, None) == capi.FX_E_INVALID
    assert lib.fx_download_pressure_level(None, 0, 0, buf, 16) == capi.FX_E_INVALID


# ---- what the solver is for ---------------------------------------------------------------------------------------------------------------------
CONVERGENCE_DIMS = [(32, 32, 32), (24, 40, 72), (20, 20, 20), (64, 64, 1)]
def solves(dims, count):
    X, Y, Z = dims
    b = mg.plume_rhs(dims)
    p = np.zeros((Z, Y, X), f32)
    r0 = mg.rms_residual(p, b)
    out = []
    for _ in range(count):
        p, _ = mg.solve(p, b)
        out.append((mg.rms_residual(p, b) / r0, mg.residual_error(p, b) / r0))
    return b, r0, out


@pytest.mark.parametrize("dims", CONVERGENCE_DIMS)
def test_one_solve_leaves_less_than_half_of_forty_jacobi_sweeps(dims):
    """rms of the mean-removed residual after one default solve from zero / after 40 Jacobi sweeps, as a share of the right-hand side's, in this
    fp32 model: 32^3 0.060 / 0.540, 24 x 40 x 72 0.065 / 0.614, 20^3 0.054 / 0.312, 64^2 0.029 / 0.800 (the float64 prototype of the issue, on
    its own right-hand side and with its own levels: 0.047 / 0.585, 0.16 / 0.675, 0.075 / 0.43, 0.026 / 0.79)"""
    X, Y, Z = dims
    b, r0, out = solves(dims, 1)
    jac = mg.rms_residual(open_ref.ref_jacobi(np.zeros((Z, Y, X), f32), b, None, 0, 40), b) / r0
    print("%s: multigrid %.4f, 40 Jacobi sweeps %.4f of the initial residual" % (dims, out[0][0], jac))
    assert out[0][0] <= 0.5 * jac


@pytest.mark.parametrize("dims", CONVERGENCE_DIMS + [(37, 53, 1)])
def test_the_residual_does_not_grow_over_six_solves(dims):
    """non-increasing, as far as the fp32 residual can tell: the rms measured for a pressure differs from the rms of its exact residual by at
    most the rms of the residual's own rounding error (the model against a float64 evaluation of the same arrays, 3e-6 to 3e-5 of the initial
    residual on these shapes), so a step up by less than the two errors involved is no growth.  In this model the residuals are, as shares of
    the initial one: 32^3 0.060, 0.0040, 2.7e-4, 2.1e-5, 1.1e-5, 1.1e-5 (error 7e-6); 24 x 40 x 72 0.065, 0.018, 0.0095, 0.0052, 0.0029,
    0.0016 (1.5e-5); 20^3 0.054, 0.0056, 8.2e-4, 1.3e-4, 2.1e-5, 5.4e-6 (3e-6); 64^2 0.029, 9.0e-4, 5.0e-5, 4.1e-5, 4.4e-5, 4.6e-5 (2.6e-5: the
    floor, where the only steps up occur, 3e-6 each); 37 x 53 0.76, 0.62, 0.54, 0.47, 0.43, 0.39"""
    _, _, out = solves(dims, 6)
    print("%s: %s (errors %s)" % (dims, " ".join("%.3g" % r for r, _ in out), " ".join("%.3g" % f for _, f in out)))
    for (r0, f0), (r1, f1) in zip(out, out[1:]):
        assert r1 <= r0 + (f0 + f1)
    assert out[-1][0] < out[0][0]


# ---- the kernels' register budget -----------------------------------------------------------------------------------------------------------------
def test_no_kernel_spills(tmp_path):
    """fx_multigrid.hip compiled for gfx950 with the library's flags: every k_mg_* instantiation has a private segment of 0 bytes"""
    from fluidx12_amd import build as b
    source = "fx_multigrid.hip"
    out = tmp_path / (source + ".s")
    subprocess.check_call([b.hipcc()] + b.FLAGS + b.EXTRA_FLAGS.get(source, []) + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(b.CSRC, source), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        if "k_mg_" in m.group(1):
            found[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
    count = {k: sum(k in name for name in found) for k in ("k_mg_smooth_v4", "k_mg_residual_restrict", "k_mg_prolong_correct", "k_mg_tail")}
    assert count == {"k_mg_smooth_v4": 4, "k_mg_residual_restrict": 2, "k_mg_prolong_correct": 2, "k_mg_tail": 1} and len(found) == 13, sorted(found)
    assert all(v == 0 for v in found.values()), found
