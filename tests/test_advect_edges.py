"""CPU checks of tests/advect_edges.py, the recipes of tests/test_gpu_advect_edges.py: every recipe reaches the edge it is for -- conditions on
the models' outputs, never on a kernel's --, the model and the oracle agree outside the impulse ball for every recipe, and the grids reach the
instantiations, tiles and chunks of the staged advection that advect_edges.PLAN says: fx::advect_lds_plan (csrc/fx_advect_plan.cpp), what
launch_advect_lds launches by, linked into a small program.  No device is needed."""
import os
import subprocess

import numpy as np
import pytest

import advect_edges as ae

ids = ae.ids


# ---- the recipes --------------------------------------------------------------------------------------------------------------------------
def hold(c):
    ae.assert_conditions(c)
    assert ae.agree_outside_the_ball(c), c.what
    assert c.far.mean() > 0.9 and not c.far.all()             # the oracle covers most of the field; the ball exists


@pytest.mark.parametrize("scale", ae.SCALES)
@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("storage", ae.STORAGES)
@pytest.mark.parametrize("dims", ae.SHAPES, ids=ids)
def test_geometry_cases(dims, storage, address, scale):
    c = ae.geometry(dims, storage, address, scale)
    hold(c)
    share = float(c.inwin.mean())
    print("%s: in-window share %.4f" % (c.what, share))
    # what the three scales are there for, from the normal distribution: P(|u| < 0.5) per axis in x and y (dt N = 2) is 0.988 / 0.13 / 0.03 for
    # the fast rows (sigma = scale) and 1 / 1 / 0.6 for the slow half (sigma = 0.05 scale).  So 0.2: nearly every wave inside the window;
    # 3: the slow half inside, the fast half outside; 12: the slow half mixed lane by lane (0.5 * 0.6^2 = 0.18 at most), the fast half outside
    assert share > 0.95 if scale == 0.2 else 0.45 < share < 0.6 if scale == 3.0 else 0.08 < share < 0.3


@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("dims", ae.RANGE_SHAPES, ids=ids)
def test_recipe_a_reaches_the_binary16_subnormals_and_negative_zero(dims, address):
    c = ae.half_edges(dims, address)
    hold(c)
    assert 0.1 <= c.inwin.mean() <= 0.9


@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("dims", ae.RANGE_SHAPES, ids=ids)
def test_recipe_b_is_subnormal_on_both_populations(dims, address):
    c = ae.subnormal(dims, address)
    hold(c)
    assert 0.3 <= c.inwin.mean() <= 0.7
    assert ae.subnormal_share(c.col) > 0.99 and ae.subnormal_share(c.vel[:, :, : dims[1] // 2]) > 0.99


@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("storage", ae.STORAGES)
@pytest.mark.parametrize("dims", ae.RANGE_SHAPES, ids=ids)
def test_recipe_c_plants_non_finite_values_everywhere(dims, storage, address):
    c = ae.nonfinite(dims, storage, address)
    hold(c)
    assert 0.3 <= c.inwin.mean() <= 0.8
    assert ae.same_bits(c.vel, ae.to_half(c.vel)) and ae.same_bits(c.col, ae.to_half(c.col))     # one state for both storages
    for plane in [c.vel[a] for a in range(3)] + [c.col[..., i] for i in range(4)]:
        for share in ((plane == np.inf).mean(), (plane == -np.inf).mean(), np.isnan(plane).mean()):
            assert 0.5 * ae.PLANT < share < 1.5 * ae.PLANT, share
    # a NaN of the model that no voxel's own velocity explains: the taps carry them too
    lost = ae.own_velocity_not_finite(c)
    assert (np.isnan(c.want_col[..., 3]) & ~lost).sum() > 100


def test_same_but_nan_tells_the_differences_apart():
    a = np.array([1.0, np.nan, -0.0, np.inf], np.float32)
    assert ae.same_but_nan(a, a)[0]
    b = a.copy(); b[1] = np.float32(np.nan); b.view(np.uint32)[1] ^= 1                      # another payload
    assert ae.same_but_nan(b, a)[0]
    for k, v in ((0, np.nan), (1, 1.0), (2, 0.0), (3, -np.inf)):
        b = a.copy(); b[k] = v
        assert not ae.same_but_nan(b, a)[0], k


# ---- the launcher's host side -------------------------------------------------------------------------------------------------------------
PROBE = r"""
// advect_lds_plan through its own declarations (fx_internal.h): X Y Z half force lend alpha defer [nz]; the scratch is what a context lends
#include "fx_internal.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
	if (argc < 9) return 2;
	fx::Geom g = {};
	g.X = atoi(argv[1]); g.Y = atoi(argv[2]); g.Zg = atoi(argv[3]);
	g.nz = argc > 9 ? atoi(argv[9]) : g.Zg; g.zlo = 0; g.zhi = g.Zg - 1;
	const int half = atoi(argv[4]), force = atoi(argv[5]), lend = atoi(argv[6]), alpha = atoi(argv[7]);
	fx::AdvectLdsKnobs k;
	k.defer = atoi(argv[8]);
	const size_t words = lend ? fx::advect_far_words(g, g.nz) : 0;
	const fx::AdvectLdsPlan p = fx::advect_lds_plan(g, half, 0, g.nz, force != 0, words != 0, words, alpha != 0, k);
	printf("%d %d %d %d %d %d %d %d %d %zu\n", (int)p.staged, (int)p.p2, p.tile_rows, p.tiles_x, p.tiles_y, p.zchunk, p.nchunks, (int)p.defer, (int)p.alpha, words);
	return 0;
}
"""
FIELDS = ("staged", "p2", "tile_rows", "tiles_x", "tiles_y", "zchunk", "nchunks", "defer", "alpha", "words")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """fx_advect_plan.cpp linked into a small program, compiled as the library's sources are"""
    from fluidx12_amd import build
    d = tmp_path_factory.mktemp("advect_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run([build.hipcc()] + build.FLAGS + ["-I", build.CSRC, "-x", "hip", str(src), os.path.join(build.CSRC, "fx_advect_plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def call(dims, half=0, force=1, lend=1, alpha=0, defer=1, nz=None):
        argv = [str(exe)] + [str(int(v)) for v in tuple(dims) + (half, force, lend, alpha, defer)] + ([str(nz)] if nz is not None else [])
        return dict(zip(FIELDS, (int(v) for v in subprocess.run(argv, check=True, capture_output=True, text=True).stdout.split())))
    return call


def chunk_lengths(p, nzp):
    return [min(p["zchunk"], nzp - k * p["zchunk"]) for k in range(p["nchunks"])]


def test_the_library_is_built_from_the_planner():
    from fluidx12_amd import build
    assert "fx_advect_plan.cpp" in build.SOURCES and "fx_advect_lds.hip" in build.SOURCES
    text = open(os.path.join(build.CSRC, "fx_advect_lds.hip")).read()
    assert "advect_lds_plan(" in text and "pow2" not in text and "min_voxels" not in text      # the launcher decides nothing itself


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("dims", ae.SHAPES, ids=ids)
def test_every_grid_reaches_what_the_table_says(plan, dims, half):
    want = ae.PLAN[dims]
    X, Y, Z = dims
    for defer in (1, 0):
        p = plan(dims, half=half, defer=defer)
        assert p["staged"] == 1 and p["p2"] == int(want["p2"]) and p["tile_rows"] == 8 and p["defer"] == defer and p["alpha"] == 0, p
        assert (p["tiles_x"], X - 64 * (p["tiles_x"] - 1)) == want["x"] and (p["tiles_y"], Y - 8 * (p["tiles_y"] - 1)) == want["y"], p
        # off the power-of-two grids the chunks do not depend on the deferral; on them 32 planes deferring, 16 inline -- both one chunk of 16 here
        assert chunk_lengths(p, Z) == want["chunks"], p
        assert sum(chunk_lengths(p, Z)) == Z and min(chunk_lengths(p, Z)) >= 1
    assert plan(dims, half=half, lend=0)["defer"] == 0                        # no scratch lent: gathers inside the kernel
    if dims in ae.ALPHA_SHAPES:
        # the alpha side volume rides along where the far voxels are deferred (tests/test_gpu_advect_edges.py part 3c), and only there
        assert plan(dims, half=half, alpha=1)["alpha"] == 1 and plan(dims, half=half, alpha=1, defer=0)["alpha"] == 0
        assert plan(dims, half=half, alpha=1, lend=0)["alpha"] == 0


def test_thresholds_of_the_staged_path(plan):
    assert plan((63, 64, 16))["staged"] == 0 and plan((64, 64, 16))["staged"] == 1           # X < 64
    assert plan((64, 7, 16))["staged"] == 0 and plan((64, 8, 16))["staged"] == 1             # fewer rows than a tile
    assert plan((64, 64, 11))["staged"] == 0 and plan((64, 64, 12))["staged"] == 1           # 11 planes
    assert plan((64, 64, 1))["staged"] == 0                                                  # 2-D
    # below 2^22 voxels per launch only when forced (ADVECT_LDS = 2)
    assert plan((128, 128, 255), force=0)["staged"] == 0 and plan((128, 128, 256), force=0)["staged"] == 1
    assert plan((128, 128, 255), force=1)["staged"] == 1
    for dims in ae.SHAPES:
        assert plan(dims, force=0)["staged"] == 0
    # a slab's launch: its own planes count, not the grid's (the cases test_gpu_slabs.py adds: 48 planes of 96 each)
    for dims in ((72, 72, 96), (64, 64, 96)):
        p = plan(dims, nz=48)
        assert p["staged"] == 1 and p["p2"] == 0 and p["defer"] == 1 and sum(chunk_lengths(p, 48)) == 48, p
    assert plan((64, 64, 96), nz=11)["staged"] == 0


def test_the_shipped_sizes_keep_their_plans(plan):
    """what the launcher chose before the planner was moved out of it: 256^3 (the benchmark) 32-plane chunks deferring and 16 inline, 150^3 as many
    chunks as keep every workgroup resident"""
    p = plan((256, 256, 256), force=0)
    assert (p["staged"], p["p2"], p["tiles_x"], p["tiles_y"], p["zchunk"], p["nchunks"], p["defer"]) == (1, 1, 4, 32, 32, 8, 1)
    p = plan((256, 256, 256), force=0, defer=0)
    assert (p["zchunk"], p["nchunks"], p["defer"]) == (16, 16, 0)
    p = plan((150, 150, 150), force=1)
    assert (p["p2"], p["tiles_x"], p["tiles_y"], p["zchunk"], p["nchunks"]) == (0, 3, 19, 19, 8)       # 57 tiles: 512 // 57 = 8 chunks of ceil(150 / 8)
