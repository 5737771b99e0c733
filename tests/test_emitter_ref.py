"""CPU checks of the settable emitters (fx_set_emitters): the numpy model tests/emitter_ref.py against a plain-loop restatement, the
launcher's host side (fx::emit_plan of csrc/fx_emit_plan.cpp: bounding boxes, clipping, tiling), linked into a small program -- no
device is needed --, and the new struct in the C header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import emitter_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# (centre, radius): the built-in ball's place, one well inside, one clipped by two walls, one more, the whole grid, and one without a cell
SIX = [((0.5, 0.1, 0.5), 1 / 16), ((0.3, 0.6, 0.4), 0.11), ((0.02, 0.97, 0.5), 0.2), ((0.7, 0.3, 0.55), 0.13), ((0.5, 0.5, 0.5), 1.0),
       ((0.41, 0.37, 0.52), 0.004)]
SHAPES = [(32, 32, 32), (20, 20, 12), (70, 70, 5), (130, 130, 4), (256, 256, 6), (36, 36, 1), (64, 64, 1)]


def six():
    return [er.emitter(c, r, color_rate=(0.5 + k, 1.0 + 2 * k, 3.0, 2.0 + k), force=(10.0 * k - 20.0, 30.0 + 7 * k, 5.0 * k), swirl=40.0 * k - 60.0)
            for k, (c, r) in enumerate(SIX)]


@pytest.mark.parametrize("dims", [(8, 8, 8), (9, 9, 1)])
def test_model_is_the_plain_loops(dims):
    X, Y, Z = dims
    rng = np.random.default_rng(3)
    vel = rng.standard_normal((3, Z, Y, X)).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    ems = six() + [er.emitter((0.4, 0.4, 0.45), 0.3, color_rate=(90.0, 0.0, 5.0, 60.0))]      # saturates
    dt = f32(0.25)
    v0, c0, m0 = er.apply(vel, col, ems, dt)
    v1, c1, m1 = er.apply_loops(vel, col, ems, dt)
    assert np.array_equal(m0, m1) and m0.any()
    assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(c0.view(np.uint32), c1.view(np.uint32))
    assert c0.max() == 1.0                                            # the saturation took part
    # outside every support nothing moved
    assert np.array_equal(v0[:, ~m0].view(np.uint32), vel[:, ~m0].view(np.uint32)) and np.array_equal(c0[~m0].view(np.uint32), col[~m0].view(np.uint32))


@pytest.mark.parametrize("dims", SHAPES)
def test_the_test_emitters_keep_clear_of_the_threshold(dims):
    """the precondition of the GPU comparison: no cell's basis within relative 1e-5 of e^-4"""
    assert er.near_threshold(dims, six()) == 0


def test_model_fp16_rounds_changed_cells_only():
    dims = (20, 20, 12)
    X, Y, Z = dims
    rng = np.random.default_rng(5)
    vel = rng.standard_normal((3, Z, Y, X)).astype(np.float16).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(np.float16).astype(f32)
    v, c, m = er.apply(vel, col, six()[:4], f32(0.1), half=True)
    assert m.any() and not m.all()
    assert np.array_equal(v[:, ~m], vel[:, ~m]) and np.array_equal(c[~m], col[~m])
    assert np.array_equal(v, v.astype(np.float16).astype(f32)) and np.array_equal(c, c.astype(np.float16).astype(f32))


# ---- the launcher's host side -------------------------------------------------------------------------------------------------------

PROBE = r"""
// emit_plan through its own declarations (fx_internal.h): X Y Z, then cx cy cz r per emitter; emitter k carries swirl k + 1
#include "fx_internal.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char** argv)
{
	fx::Geom g = {};
	g.X = atoi(argv[1]); g.Y = atoi(argv[2]); g.Zg = g.nz = atoi(argv[3]); g.zhi = g.Zg - 1;
	fx_emitter list[FX_MAX_EMITTERS + 1];
	int n = 0;
	for (int i = 4; i + 3 < argc && n <= (int)FX_MAX_EMITTERS; i += 4, ++n) {
		fx_emitter e = {};
		e.struct_size = sizeof e;
		for (int a = 0; a < 3; ++a) e.center[a] = (float)atof(argv[i + a]);
		e.radius = (float)atof(argv[i + 3]);
		e.swirl = (float)(n + 1);
		list[n] = e;
	}
	fx::EmitArgs a;
	const int wgs = fx::emit_plan(g, list, n, &a);
	printf("%d %d %d %d %d %d %d %d\n", wgs, a.n, a.x0, a.y0, a.z0, a.tiles_x, a.tiles_y, a.tiles_z);
	for (int k = 0; k < a.n; ++k) {
		const fx::EmitBall& b = a.e[k];
		unsigned w[4];
		memcpy(w, b.c, 12); memcpy(w + 3, &b.rr, 4);
		printf("%d %u %u %u %u %d %d %d %d %d %d\n", (int)b.swirl - 1, w[0], w[1], w[2], w[3], b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]);
	}
	return 0;
}
"""


class Ball:
    pass


class Args:
    pass


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """fx_emit_plan.cpp linked into a small program of its own, compiled as the library's sources are: no device is needed to run it"""
    from fluidx12_amd import build
    d = tmp_path_factory.mktemp("emit_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run([build.hipcc()] + build.FLAGS + ["-I", build.CSRC, "-x", "hip", str(src), os.path.join(build.CSRC, "fx_emit_plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def call(dims, ems):
        argv = [str(exe)] + [str(v) for v in dims]
        for e in ems:
            argv += [repr(float(v)) for v in e["center"]] + [repr(float(e["radius"]))]
        rows = [[int(v) for v in l.split()] for l in subprocess.run(argv, check=True, capture_output=True, text=True).stdout.splitlines()]
        a = Args()
        wgs, a.n, a.x0, a.y0, a.z0, a.tiles_x, a.tiles_y, a.tiles_z = rows[0]
        a.e = []
        for r in rows[1:]:
            b = Ball()
            b.index = r[0]                                           # which emitter of the list this is
            b.c = tuple(np.array(r[1:4], np.uint32).view(f32))
            b.rr = np.array(r[4:5], np.uint32).view(f32)[0]
            b.lo, b.hi = tuple(r[5:8]), tuple(r[8:11])
            a.e.append(b)
        assert len(a.e) == a.n
        return wgs, a
    return call


def bbox(mask):
    """[lo, hi) per axis (x, y, z) of a mask[Z][Y][X]"""
    idx = np.argwhere(mask)
    return [(int(idx[:, 2 - a].min()), int(idx[:, 2 - a].max()) + 1) for a in range(3)]


@pytest.mark.parametrize("dims", SHAPES)
def test_plan_boxes_hold_every_support_and_tiles_cover_them(plan, dims):
    ems = six()
    wgs, a = plan(dims, ems)
    sup = [er.support(dims, e) for e in ems]

    def near(k, ax):                                                 # the cells within the radius along one axis
        if dims[2] == 1 and ax == 2:
            return np.array([0])
        return np.flatnonzero(np.abs((np.arange(dims[ax]) + 0.5) / dims[ax] - ems[k]["center"][ax]) <= ems[k]["radius"])
    kept = [k for k in range(len(ems)) if all(len(near(k, ax)) for ax in range(3))]
    assert a.n == len(kept) and 5 not in kept                        # the sixth has no cell at any of these shapes and is dropped
    assert all(k in kept for k in range(len(ems)) if sup[k].any())
    ulo, uhi = [10 ** 9] * 3, [0] * 3
    for j, k in enumerate(kept):
        b = a.e[j]
        assert tuple(b.c) == tuple(f32(v) for v in ems[k]["center"]) and b.index == k                          # list order kept
        assert b.rr == f32(ems[k]["radius"]) * f32(ems[k]["radius"])
        for ax in range(3):
            assert 0 <= b.lo[ax] < b.hi[ax] <= dims[ax], (k, ax)
            if sup[k].any():
                lo, hi = bbox(sup[k])[ax]
                assert b.lo[ax] <= lo and hi <= b.hi[ax], (k, ax)
            # ... and tight: the cells within the radius along this axis (clipped), a cell more at most -- the work follows the covered volume
            n = near(k, ax)
            assert 0 <= n[0] - b.lo[ax] <= 1 and 0 <= b.hi[ax] - (n[-1] + 1) <= 1, (k, ax)
            ulo[ax], uhi[ax] = min(ulo[ax], b.lo[ax]), max(uhi[ax], b.hi[ax])
    assert a.x0 % 64 == 0 and a.y0 % 4 == 0 and a.x0 <= ulo[0] and a.y0 <= ulo[1] and a.z0 == ulo[2]
    assert a.x0 + 64 * a.tiles_x >= uhi[0] > a.x0 + 64 * (a.tiles_x - 1)
    assert a.y0 + 4 * a.tiles_y >= uhi[1] > a.y0 + 4 * (a.tiles_y - 1)
    assert a.tiles_z == uhi[2] - ulo[2]
    assert wgs == a.tiles_x * a.tiles_y * a.tiles_z


def test_plan_follows_the_ball_not_the_grid(plan):
    dims = (256, 256, 256)
    wgs, a = plan(dims, [er.emitter(**er.BUILTIN_3D)])
    assert a.n == 1 and (a.x0, a.y0, a.z0) == (64, 8, 112)
    assert (a.tiles_x, a.tiles_y, a.tiles_z) == (2, 9, 32)          # x 112..143: the two 64-wide tiles from 64; y 10..41: rows 8..43 in fours; z 112..143
    assert wgs == 576                                                # of the grid's 4 * 64 * 256 = 65536 tiles
    assert tuple(a.e[0].lo) == (112, 10, 112) and tuple(a.e[0].hi) == (144, 42, 144)


def test_plan_launches_nothing_for_an_empty_union(plan):
    dims = (32, 32, 32)
    for ems in ([], [er.emitter((0.41, 0.37, 0.52), 0.004)], [er.emitter((3.0, 0.5, 0.5), 1.0)], [er.emitter((0.5, -2.0, 0.5), 1.5)],
                [er.emitter((0.41, 0.37, 0.52), 0.004), er.emitter((0.5, 0.5, 7.0), 2.0)],
                [er.emitter((0.515625, 0.515625, 0.515625), 1e-25)]):          # on a cell centre, but the radius squares to 0 in fp32: dropped
        wgs, a = plan(dims, ems)
        assert wgs == 0 and a.n == 0, ems
    # a 2-D grid ignores the z coordinate of the centre
    wgs, a = plan((64, 64, 1), [er.emitter((0.5, 0.5, 9.0), 0.1)])
    assert wgs > 0 and a.n == 1 and (a.e[0].lo[2], a.e[0].hi[2]) == (0, 1)


def test_header_compiles_as_c_with_the_emitter_struct(tmp_path):
    src = tmp_path / "emitter_probe.c"
    src.write_text('#include "fluidx_hip.h"\nint main(void) { fx_emitter e[FX_MAX_EMITTERS]; e[0].struct_size = sizeof e[0]; e[0].flags = 0;\n'
                   '  e[0].center[2] = e[0].radius = e[0].color_rate[3] = e[0].force[2] = e[0].swirl = 0.0f;\n'
                   '  return sizeof(fx_emitter) == 56 && FX_MAX_EMITTERS == 16u && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "probe")], check=True)
        assert subprocess.run([str(tmp_path / "probe")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_ctypes_struct_matches_the_header():
    import ctypes as C
    from fluidx12_amd import capi
    assert C.sizeof(capi.Emitter) == 56 and capi.MAX_EMITTERS == 16
