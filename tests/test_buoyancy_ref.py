"""CPU checks of the buoyancy pass (fx_set_buoyancy / fx_set_heat_sources / fx_heat): the new structs in the C header, the ctypes / Python /
C++ mirrors, the numpy model tests/buoyancy_ref.py against a plain-loop restatement and its invariants, and the launcher's host side
(fx::heat_plan of csrc/fx_heat_plan.cpp: the sources' boxes, the grid's tiles and the axes the force acts on), linked into a small
program -- no device is needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import buoyancy_ref as br
import emitter_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

SHAPES = br.SHAPES                                                  # the shapes and the sources of tests/test_gpu_buoyancy.py
six = br.list_b


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the header and its mirrors ---------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_with_the_buoyancy_structs(tmp_path):
    src = tmp_path / "buoyancy_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'int main(void) { fx_buoyancy b; fx_heat_source h[FX_MAX_HEAT_SOURCES]; b.struct_size = sizeof b; b.flags = 0;\n'
                   '  b.ambient = b.density_weight = b.lift = b.cooling = b.up[2] = 0.0f; h[0].struct_size = sizeof h[0]; h[0].flags = 0;\n'
                   '  h[0].center[2] = h[0].radius = h[0].rate = 0.0f;\n'
                   '  return sizeof(fx_buoyancy) == 36 && sizeof(fx_heat_source) == 28 && FX_MAX_HEAT_SOURCES == 16u && FX_ABI_VERSION == 7 &&\n'
                   '    FX_FIELD_TEMPERATURE == 11 && b.struct_size == 36 && h[0].struct_size == 28 ? 0 : 1; }\n')
    calls = tmp_path / "buoyancy_calls.c"
    calls.write_text('#include "fluidx_hip.h"\n'
                     'static int (*set_)(fx_ctx*, const fx_buoyancy*) = fx_set_buoyancy;\n'
                     'static int (*get_)(fx_ctx*, fx_buoyancy*, int*) = fx_get_buoyancy;\n'
                     'static int (*sets_)(fx_ctx*, const fx_heat_source*, uint32_t) = fx_set_heat_sources;\n'
                     'static int (*gets_)(fx_ctx*, fx_heat_source*, uint32_t, uint32_t*) = fx_get_heat_sources;\n'
                     'static int (*heat_)(fx_ctx*, void*) = fx_heat;\n'
                     'int use(void) { return set_ && get_ && sets_ && gets_ && heat_; }\n')
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") or shutil.which("g++")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "probe")], check=True)
        assert subprocess.run([str(tmp_path / "probe")]).returncode == 0
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(calls), "-o", str(tmp_path / "calls.o")], check=True)
    if shutil.which("g++"):
        for f in (src, calls):
            subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(f)], check=True)


def test_mirrors_carry_the_interface():
    from fluidx12_amd import build, capi
    import fluidx12_amd as fx
    assert C.sizeof(capi.Buoyancy) == 36 and C.sizeof(capi.HeatSource) == 28
    assert capi.MAX_HEAT_SOURCES == 16 and capi.FIELD_TEMPERATURE == 11 == fx.FIELD_TEMPERATURE and capi.ABI_VERSION == 7
    for name in ("fx_set_buoyancy", "fx_get_buoyancy", "fx_set_heat_sources", "fx_get_heat_sources", "fx_heat"):
        assert name in capi.SYMBOLS
    assert capi.SYMBOLS["fx_get_buoyancy"][1][1:] == [C.POINTER(capi.Buoyancy), C.POINTER(C.c_int)]
    for name in ("SetBuoyancy", "GetBuoyancy", "SetHeatSources", "GetHeatSources", "Heat"):
        assert callable(getattr(fx.Fluid, name))
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetBuoyancy", "GetBuoyancy", "SetHeatSources", "GetHeatSources", "Heat", "fx_set_buoyancy", "fx_get_buoyancy",
                 "fx_set_heat_sources", "fx_get_heat_sources", "fx_heat"):
        assert name in hpp, name
    assert "fx_heat.hip" in build.SOURCES and "fx_heat_plan.cpp" in build.SOURCES


def test_refusals_that_need_no_device():
    from fluidx12_amd import capi
    lib = capi.load()
    on = C.c_int(7)
    n = C.c_uint32(7)
    assert lib.fx_set_buoyancy(None, None) == capi.FX_E_INVALID and lib.fx_get_buoyancy(None, None, C.byref(on)) == capi.FX_E_INVALID and on.value == 7
    assert lib.fx_set_heat_sources(None, None, 0) == capi.FX_E_INVALID
    assert lib.fx_get_heat_sources(None, None, 0, C.byref(n)) == capi.FX_E_INVALID and n.value == 7
    assert lib.fx_heat(None, None) == capi.FX_E_INVALID


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def rand_state(dims, seed, scale=1.0):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vel0 = (rng.standard_normal((3, Z, Y, X)) * scale).astype(f32)
    vel1 = rng.standard_normal((3, Z, Y, X)).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    T = (rng.random((Z, Y, X)) * 4 - 1).astype(f32)
    return T, vel0, vel1, col


@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("dims", [(6, 5, 4), (7, 6, 1)])
def test_model_is_the_plain_loops(dims, address):
    T, vel0, vel1, col = rand_state(dims, 11, scale=2.0)             # dt * N * |u| of a few cells: traces leave the walls
    vel1[0, 0, 0, 0] = f32(-0.0)
    prm = br.params(ambient=0.25, density_weight=0.7, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2))
    src = [br.source((0.4, 0.5, 0.5), 0.3, 9.0), br.source((0.7, 0.3, 0.6), 0.25, -4.0)]
    solid = np.random.default_rng(12).random(T.shape) < 0.2
    dt = f32(0.3)
    for mask in (None, solid):
        t0, v0 = br.apply(T, vel0, vel1, col, prm, src, dt, address, solid=mask)
        t1, v1 = br.apply_loops(T, vel0, vel1, col, prm, src, dt, address, solid=mask)
        assert same_bits(t0, t1) and same_bits(v0, v1)
        assert not same_bits(t0, T) and not same_bits(v0, vel1)
        if dims[2] == 1:
            assert same_bits(v0[2], vel1[2])                         # a 2-D grid has no z component to push
    assert same_bits(t0[solid], np.full(int(solid.sum()), f32(0.25))) and same_bits(v0[:, solid], vel1[:, solid])
    assert br.supports(dims, src).any()


@pytest.mark.parametrize("address", ["clamp", "mirror"])
def test_uniform_ambient_stays_ambient_bit_for_bit(address):
    dims = (9, 8, 5)
    _, vel0, vel1, col = rand_state(dims, 13, scale=5.0)
    for Ta in (0.0, 1.7, -3.25, 293.15):
        T = np.full(dims[::-1], f32(Ta))
        t, _ = br.apply(T, vel0, vel1, col, br.params(ambient=Ta, cooling=0.37, lift=2.0, density_weight=0.5), [], f32(0.21), address)
        assert same_bits(t, T)


def test_zero_coefficients_leave_the_velocity_values():
    dims = (9, 8, 5)
    T, vel0, vel1, col = rand_state(dims, 17)
    t, v = br.apply(T, vel0, vel1, col, br.params(ambient=0.5, cooling=0.2, up=(0.3, 1.0, -0.2)), six()[:4], f32(0.1))
    assert np.array_equal(v, vel1) and not same_bits(t, T)


def test_full_cooling_returns_ambient_outside_the_supports():
    dims = (12, 10, 6)
    T, vel0, vel1, col = rand_state(dims, 19)
    src = six()[:4]
    for cooling, dt in ((4.0, 0.25), (10.0, 0.5)):                    # cooling * dt = 1 and 5
        t, _ = br.apply(T, vel0, vel1, col, br.params(ambient=0.75, cooling=cooling), src, f32(dt))
        m = br.supports(dims, src)
        assert m.any() and not m.all()
        assert same_bits(t[~m], np.full(int((~m).sum()), f32(0.75)))
        assert not np.any(t[m] == f32(0.75))


def test_model_fp16_rounds_the_pushed_components_only():
    dims = (10, 9, 4)
    T, vel0, vel1, col = rand_state(dims, 23)
    vel0, vel1, col = (a.astype(np.float16).astype(f32) for a in (vel0, vel1, col))
    t, v = br.apply(T, vel0, vel1, col, br.params(lift=1.0, density_weight=0.3), [], f32(0.1), half=True)
    assert same_bits(v[0], vel1[0]) and same_bits(v[2], vel1[2]) and not same_bits(v[1], vel1[1])
    assert np.array_equal(v[1], v[1].astype(np.float16).astype(f32))


@pytest.mark.parametrize("dims", SHAPES)
def test_the_test_sources_keep_clear_of_the_threshold(dims):
    """the precondition of the GPU comparison: no cell's basis within relative 1e-5 of e^-4 -- the cap on excluded cells is zero"""
    assert br.near_threshold(dims, six()) == 0


# ---- the launcher's host side ----------------------------------------------------------------------------------------------------------
PROBE = r"""
// heat_plan through its own declarations (fx_internal.h): X Y Z, upx upy upz, then cx cy cz r per source; source k carries rate k + 1
#include "fx_internal.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char** argv)
{
	if (argc < 7) return 2;
	fx::Geom g = {};
	g.X = atoi(argv[1]); g.Y = atoi(argv[2]); g.Zg = g.nz = atoi(argv[3]); g.zhi = g.Zg - 1;
	fx_buoyancy b = {};
	b.struct_size = sizeof b;
	b.ambient = 1.0f; b.density_weight = 2.0f; b.lift = 3.0f; b.cooling = 4.0f;
	for (int a = 0; a < 3; ++a) b.up[a] = (float)atof(argv[4 + a]);
	fx_heat_source list[FX_MAX_HEAT_SOURCES + 1];
	int n = 0;
	for (int i = 7; i + 3 < argc && n <= (int)FX_MAX_HEAT_SOURCES; i += 4, ++n) {
		fx_heat_source e = {};
		e.struct_size = sizeof e;
		for (int a = 0; a < 3; ++a) e.center[a] = (float)atof(argv[i + a]);
		e.radius = (float)atof(argv[i + 3]);
		e.rate = (float)(n + 1);
		list[n] = e;
	}
	fx::HeatArgs h;
	const int wgs = fx::heat_plan(g, b, list, n, &h);
	printf("%d %d %d %d %d %d %d %d %d %d %d\n", wgs, h.axes, h.n, h.tiles_x, h.tiles_y, (int)h.ambient, (int)h.weight, (int)h.lift, (int)h.cooling,
		h.up[0] == b.up[0] && h.up[1] == b.up[1] && h.up[2] == b.up[2], 0);
	for (int k = 0; k < h.n; ++k) {
		const fx::HeatBall& s = h.s[k];
		unsigned w[4];
		memcpy(w, s.c, 12); memcpy(w + 3, &s.rr, 4);
		printf("%d %u %u %u %u %d %d %d %d %d %d\n", (int)s.rate - 1, w[0], w[1], w[2], w[3], s.lo[0], s.lo[1], s.lo[2], s.hi[0], s.hi[1], s.hi[2]);
	}
	return 0;
}
"""


class Ball:
    pass


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """fx_heat_plan.cpp (and fx_emit_plan.cpp, which it takes the boxes from) linked into a small program, compiled as the library's sources are"""
    from fluidx12_amd import build
    d = tmp_path_factory.mktemp("heat_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run([build.hipcc()] + build.FLAGS + ["-I", build.CSRC, "-x", "hip", str(src), os.path.join(build.CSRC, "fx_heat_plan.cpp"),
                    os.path.join(build.CSRC, "fx_emit_plan.cpp"), "-o", str(exe)], check=True, capture_output=True)

    def call(dims, up, sources):
        argv = [str(exe)] + [str(v) for v in dims] + [repr(float(v)) for v in up]
        for s in sources:
            argv += [repr(float(v)) for v in s["center"]] + [repr(float(s["radius"]))]
        rows = [[int(v) for v in l.split()] for l in subprocess.run(argv, check=True, capture_output=True, text=True).stdout.splitlines()]
        head = dict(zip(("wgs", "axes", "n", "tiles_x", "tiles_y", "ambient", "weight", "lift", "cooling", "up_kept"), rows[0]))
        balls = []
        for r in rows[1:]:
            b = Ball()
            b.index = r[0]                                           # which source of the list this is
            b.c = tuple(np.array(r[1:4], np.uint32).view(f32))
            b.rr = np.array(r[4:5], np.uint32).view(f32)[0]
            b.lo, b.hi = tuple(r[5:8]), tuple(r[8:11])
            balls.append(b)
        assert len(balls) == head["n"]
        return head, balls
    return call


def bbox(mask):
    idx = np.argwhere(mask)
    return [(int(idx[:, 2 - a].min()), int(idx[:, 2 - a].max()) + 1) for a in range(3)]


@pytest.mark.parametrize("dims", SHAPES)
def test_plan_boxes_hold_every_support_and_the_tiles_cover_the_grid(plan, dims):
    src = six()
    head, balls = plan(dims, (0.0, 1.0, 0.0), src)
    X, Y, Z = dims
    assert (head["tiles_x"], head["tiles_y"]) == ((X + 63) // 64, (Y + 3) // 4) and head["wgs"] == head["tiles_x"] * head["tiles_y"] * Z
    assert (head["ambient"], head["weight"], head["lift"], head["cooling"], head["up_kept"]) == (1, 2, 3, 4, 1)
    sup = [er.support(dims, br.as_emitter(s)) for s in src]

    def near(k, ax):                                                 # the cells within the radius along one axis
        if Z == 1 and ax == 2:
            return np.array([0])
        return np.flatnonzero(np.abs((np.arange(dims[ax]) + 0.5) / dims[ax] - src[k]["center"][ax]) <= src[k]["radius"])
    kept = [k for k in range(len(src)) if all(len(near(k, ax)) for ax in range(3))]
    assert [b.index for b in balls] == kept and 5 not in kept        # list order kept; the sixth has no cell at any of these shapes
    assert all(k in kept for k in range(len(src)) if sup[k].any())
    for b in balls:
        k = b.index
        assert tuple(b.c) == tuple(f32(v) for v in src[k]["center"]) and b.rr == f32(src[k]["radius"]) * f32(src[k]["radius"])
        for ax in range(3):
            assert 0 <= b.lo[ax] < b.hi[ax] <= dims[ax], (k, ax)
            if sup[k].any():
                lo, hi = bbox(sup[k])[ax]
                assert b.lo[ax] <= lo and hi <= b.hi[ax], (k, ax)
            n = near(k, ax)                                          # ... and tight: a cell more at most
            assert 0 <= n[0] - b.lo[ax] <= 1 and 0 <= b.hi[ax] - (n[-1] + 1) <= 1, (k, ax)


def test_plan_picks_the_axes_of_up(plan):
    for up, want3, want2 in (((0.0, 1.0, 0.0), 2, 2), ((0.3, 1.0, -0.2), 7, 3), ((1.0, 0.0, 0.0), 1, 1), ((0.0, 0.0, -2.0), 4, 0)):
        assert plan((32, 32, 32), up, [])[0]["axes"] == want3, up
        assert plan((36, 36, 1), up, [])[0]["axes"] == want2, up      # a 2-D grid: never z
    head, balls = plan((32, 32, 32), (0.0, 1.0, 0.0), [])
    assert head["n"] == 0 and balls == [] and head["wgs"] == 1 * 8 * 32
    head, _ = plan((256, 256, 256), (0.0, 1.0, 0.0), six())
    assert head["wgs"] == 4 * 64 * 256 and head["n"] == 6            # at 256^3 the sixth source holds a cell
