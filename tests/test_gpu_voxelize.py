"""The mesh voxeliser on the GPU (fx_set_obstacle_meshes, csrc/fx_voxelize.hip) against the numpy model tests/voxelize_ref.py: the mask
fx_get_obstacles returns and the report, exact equality everywhere (tests/test_voxelize_ref.py anchors the model).

Grids (X, Y, Z) -- the library's planes are square (fx_create refuses X != Y), so Y = X throughout: (20, 20, 10) a row shorter than a
word; (32, 32, 6) the virtual cell X falls in the second word; (72, 72, 20) three words, the fill's carry crosses lanes, 1440 columns: a
wall-sized triangle takes the patch kernel; (160, 160, 6) five words, 960 columns: the same triangle stays with its wave; (24, 24, 8) rows
that are no multiple of 16 bytes: the fill's byte path (X = 20 too)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import emitter_ref as er
import moving_obstacle_ref as mv
import voxelize_ref as vr

pytestmark = pytest.mark.gpu
f32 = np.float32

GRIDS = [(20, 20, 10), (32, 32, 6), (72, 72, 20), (160, 160, 6)]
MID = (72, 72, 20)
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status
    return f


@functools.lru_cache(maxsize=None)
def ctx(dims):
    """one context per grid for the whole file: every call replaces the mask, and the bitmap must come back clean each time"""
    return make(dims, jacobi_iters=4)


def check(dims, meshes, f=None):
    """the device against the model for one call -> (mask, report)"""
    f = f or ctx(dims)
    rep = f.SetObstacleMeshes(meshes)
    want, wrep = vr.voxelise(meshes, dims)
    got, cells = f.GetObstacles()
    print(dims, "device", rep, "model", wrep)
    assert rep == wrep and cells == wrep["solid_cells"]
    assert np.array_equal(got, want)
    return want, wrep


def box(dims):
    X, Y, Z = dims
    return vr.box_mesh(vr.cell_centre(dims, (X // 5, Y // 6, Z // 5)), vr.cell_centre(dims, (3 * X // 4, 4 * Y // 5, 3 * Z // 4)))


# ---- 1: closed meshes on every grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", GRIDS + [(24, 24, 8)])
def test_box_sphere_and_torus_match_the_model(dims):
    X, Y, Z = dims
    v, t = box(dims)
    m, rep = check(dims, [(v, t, None)])
    assert rep["open_columns"] == 0
    assert rep["solid_cells"] == (3 * X // 4 - X // 5) * (4 * Y // 5 - Y // 6) * (3 * Z // 4 - Z // 5)    # all ties
    m, rep = check(dims, [vr.uv_sphere((0.5, 0.5, 0.5), 0.3, 12, 24) + (None,)])
    assert rep["open_columns"] == 0 and rep["solid_cells"] > 0
    m, rep = check(dims, [vr.torus((0.5, 0.5, 0.5), 0.27, 0.12) + (None,)])                            # two crossings of a column and four
    assert rep["open_columns"] == 0 and rep["solid_cells"] > 0 and not m[Z // 2, Y // 2, X // 2]


@pytest.mark.parametrize("wall", range(6))
def test_a_sphere_across_each_wall_stays_closed(wall):
    c = [0.5, 0.5, 0.5]
    c[wall // 2] = (-0.05, 0.9)[wall % 2]
    m, rep = check(MID, [vr.uv_sphere(c, 0.3, 12, 24) + (None,)])
    assert rep["open_columns"] == 0 and rep["solid_cells"] > 0
    face = [slice(None)] * 3
    face[2 - wall // 2] = -1 if wall % 2 else 0
    assert m[tuple(face)].any()


# ---- 2: the scatter's paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [MID, (160, 160, 6)])
def test_triangles_far_larger_than_the_grid(dims):
    """the quantiser's clamp at +-2^18 and the box clipped to the grid; tilted, so that the crossing cell runs over the whole row and past
    both of its ends; on 72 x 72 x 20 the clipped box takes the patch kernel, on 160 x 160 x 6 the wave's own loop"""
    v = np.array([[0.2, -900.0, -700.0], [0.9, 800.0, -650.0], [0.4, 30.0, 990.0],
                  [-0.3, -3.0, -2.0], [1.4, 4.0, -1.5], [0.5, 0.5, 5.0]], f32)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.uint32)
    m, rep = check(dims, [(v, t, None)])
    assert rep["open_columns"] > 20 and 0 < rep["solid_cells"] < m.size            # open, and it crosses inside the grid
    q, _ = vr.quantise(v, dims)
    assert (np.abs(q[:3, 1:]) == 262144).any()                                                          # the clamp took part
    # a closed box that holds the whole grid: twelve wall-sized triangles, every cell solid
    b = vr.box_mesh((-0.5, -0.4, -0.3), (1.5, 1.6, 1.7))
    m, rep = check(dims, [b + (None,)])
    assert rep["open_columns"] == 0 and rep["solid_cells"] == m.size


def test_boxes_on_either_side_of_the_patch_kernel_s_threshold():
    """rectangles (two triangles each) in tilted planes whose clipped boxes hold 960 ... 1088 columns: the wave's loop up to 1024, the list
    and the patch kernel from 1025"""
    X, Y, Z = MID
    v, t = [], []
    for n, (ny, nz) in enumerate([(60, 16), (64, 16), (65, 16), (68, 16), (57, 18), (54, 19)]):
        y0, z0 = 2 + n % 2, 1
        x = 0.1 + 0.12 * n
        lo = ((y0 + 0.25) / Y, (z0 + 0.25) / Z)
        hi = ((y0 + ny - 0.25) / Y, (z0 + nz - 0.25) / Z)                                                 # centres y0 .. y0 + ny - 1 inside
        k = 4 * n
        v += [(x, lo[0], lo[1]), (x + 0.05, hi[0], lo[1]), (x + 0.1, hi[0], hi[1]), (x + 0.05, lo[0], hi[1])]
        t += [(k, k + 1, k + 2), (k, k + 2, k + 3)]
    m, rep = check(MID, [(np.array(v, f32), np.array(t, np.uint32), None)])
    assert rep["open_columns"] > 0


def test_two_thousand_quads_on_the_same_sixteen_columns():
    """atomic contention: 4000 triangles toggle bits of the same few words"""
    dims = (160, 160, 6)
    X, Y, Z = dims
    rng = np.random.default_rng(11)
    xs = rng.random(2000) * 1.2 - 0.1                                  # some beyond either wall
    lo, hi = (40.25 / Y, 1.25 / Z), (43.75 / Y, 4.75 / Z)              # the centres of columns 40..43 x 1..4
    v = np.empty((2000, 4, 3), f32)
    v[:, :, 0] = xs[:, None] + np.array([0.0, 0.004, 0.008, 0.004])[None, :]
    v[:, :, 1] = np.array([lo[0], hi[0], hi[0], lo[0]])[None, :]
    v[:, :, 2] = np.array([lo[1], lo[1], hi[1], hi[1]])[None, :]
    k = 4 * np.arange(2000)[:, None]
    t = np.concatenate([k + np.array([[0, 1, 2]]), k + np.array([[0, 2, 3]])], axis=0).astype(np.uint32)
    m, rep = check(dims, [(v.reshape(-1, 3), t, None)])
    assert rep["open_columns"] == 0 and m[1:5, 40:44, :].any() and not np.delete(m, np.s_[40:44], axis=1).any()   # an even count: closed


def test_degenerate_and_invalid_triangles():
    v, t = vr.uv_sphere((0.5, 0.5, 0.5), 0.3, 8, 12)
    n = len(v)
    bad_v = np.vstack([v, [[np.nan, 0.5, 0.5]], [[0.5, np.inf, 0.5]], [[3e38, 0.5, 0.5]]]).astype(f32)
    extra = np.array([[0, 1, n + 9], [0, 1, 0xFFFFFFFF], [0, n, 2], [n + 1, 1, 2],      # out of range twice, a NaN and an infinite vertex
                      [3, 3, 4], [5, 5, 5],                                              # a repeated index: no area
                      [0, n + 2, 0]], np.uint32)                                         # finite, clamped, no area
    flat = np.array([[0.3, 0.2, 0.5], [0.6, 0.8, 0.5], [0.9, 0.4, 0.5],                  # edge-on along z: zero projected area
                     [0.3, 0.5, 0.1], [0.6, 0.5, 0.8], [0.9, 0.5, 0.4]], f32)            # ... and along y
    allv = np.vstack([bad_v, flat])
    k = len(bad_v)
    allt = np.vstack([t, extra, [[k, k + 1, k + 2], [k + 3, k + 4, k + 5]]]).astype(np.uint32)
    m, rep = check(MID, [(allv, allt, None)])
    base, brep = vr.voxelise([(v, t, None)], MID)
    assert np.array_equal(m, base) and rep == dict(brep, skipped_triangles=4)
    # a transform that overflows: every triangle is skipped, nothing is solid
    big = np.array([3e38, 3e38, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f32)
    m, rep = check(MID, [(v, t, big)])
    assert rep["skipped_triangles"] > 0 and rep["solid_cells"] < brep["solid_cells"]


def test_no_triangles_give_an_all_zero_mask_that_stays_in_force():
    dims = (32, 32, 6)
    empty = (np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32), None)
    sphere = vr.uv_sphere((0.5, 0.5, 0.5), 0.3, 8, 12) + (None,)

    def run(setter):
        f = make(dims, jacobi_iters=6)
        setter(f)
        f.timing_enable(True)
        for k in range(2):
            f.UpdateFrame(f32(2.0 / 32), k)
            f.Simulate(k)
        f.Synchronize()
        t = f.timing_read()
        out = [f.digest(k) for k in ALL_FIELDS], (t.steps, t.jacobi_launches, t.jacobi_sweeps)
        f.Release()
        return out

    def by_meshes(f):
        check(dims, [sphere], f)                                       # a mask in force, then the empty call replaces it
        assert f.SetObstacleMeshes([empty]) == {"solid_cells": 0, "open_columns": 0, "skipped_triangles": 0}
        m, cells = f.GetObstacles()
        assert cells == 0 and not m.any()
        lib = capi.load()                                               # positions and indices may be NULL
        one = (capi.ObstacleMesh * 1)()
        one[0].struct_size = C.sizeof(capi.ObstacleMesh)
        assert lib.fx_set_obstacle_meshes(f._ctx, None, one, 1, None) == capi.FX_OK

    zeros = run(lambda f: f.SetObstacles(np.zeros((6, 32, 32), np.uint8)))
    assert run(by_meshes) == zeros
    assert zeros[1][1] == zeros[1][2] == 12                             # the obstacle kernels: one sweep per launch


# ---- 3: inputs -------------------------------------------------------------------------------------------------------------------------------
def test_device_meshes_give_the_bits_of_host_meshes():
    import torch
    a = vr.uv_sphere((0.4, 0.5, 0.45), 0.28, 12, 24)
    b = vr.torus((0.6, 0.5, 0.5), 0.2, 0.1)
    xf = vr.rotation_translation((1.0, 2.0, 3.0), 0.7, (0.5, 0.5, 0.5), (0.03, -0.02, 0.01))
    host = [a + (xf,), b + (None,)]
    want, wrep = check(MID, host)
    dev = [(torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda(), None if m is None else torch.from_numpy(m).cuda()) for v, t, m in host]
    f = ctx(MID)
    assert f.SetObstacleMeshes(dev) == wrep and np.array_equal(f.GetObstacles()[0], want)
    assert f.SetObstacleMeshes([dev[0], host[1]]) == wrep and np.array_equal(f.GetObstacles()[0], want)     # mixed in one call
    # a caller's stream
    s = torch.cuda.Stream()
    assert f.SetObstacleMeshes(dev, stream=s.cuda_stream) == wrep and np.array_equal(f.GetObstacles()[0], want)


@pytest.mark.parametrize("dims", [MID, (20, 20, 10)])
def test_a_rotation_and_translation_with_irrational_entries(dims):
    v, t = box(dims)
    xf = vr.rotation_translation((0.3, -1.0, 0.6), np.sqrt(2.0), (0.5, 0.5, 0.5), (np.pi / 100, -np.e / 100, np.sqrt(3.0) / 100))
    m, rep = check(dims, [(v, t, xf)])
    assert rep["open_columns"] == 0 and rep["solid_cells"] > 0
    assert not np.array_equal(m, vr.voxelise([(v, t, None)], dims)[0])
    s = vr.uv_sphere((0.5, 0.5, 0.5), (0.3, 0.2, 0.25), 10, 16)
    check(dims, [s + (xf,)])


def test_two_overlapping_spheres_are_their_union_and_the_bitmap_comes_back_clean():
    a = vr.uv_sphere((0.4, 0.5, 0.5), 0.25, 10, 16) + (None,)
    b = vr.uv_sphere((0.6, 0.5, 0.5), 0.25, 10, 16) + (None,)
    ma, mb = vr.voxelise([a], MID)[0], vr.voxelise([b], MID)[0]
    both, rep = check(MID, [a, b])
    assert (ma & mb).sum() > 50 and np.array_equal(both, ma | mb)
    again, _ = check(MID, [a, b])                                      # a second call: nothing of the first is left in the bitmap
    assert np.array_equal(again, both)
    check(MID, [b])
    sixteen = [vr.uv_sphere((0.1 + 0.05 * k, 0.3 + 0.03 * k, 0.5), 0.12, 6, 8) + (vr.translation((0.0, 0.0, 0.01 * k)),) for k in range(16)]
    check(MID, sixteen)


# ---- 4: refusals -----------------------------------------------------------------------------------------------------------------------------
def c_meshes(items):
    arr = (capi.ObstacleMesh * max(len(items), 1))()
    for k, (v, t, m) in enumerate(items):
        arr[k].struct_size, arr[k].flags = C.sizeof(capi.ObstacleMesh), 0
        arr[k].positions, arr[k].indices = v.ctypes.data, t.ctypes.data
        arr[k].vertex_count, arr[k].triangle_count = len(v), len(t)
        arr[k].transform = None if m is None else m.ctypes.data
    return arr


def test_every_refusal_leaves_the_previous_mask_in_force():
    lib = capi.load()
    dims = (32, 32, 6)
    v, t = vr.uv_sphere((0.5, 0.5, 0.5), 0.3, 8, 12)
    v, t = np.ascontiguousarray(v), np.ascontiguousarray(t)
    other = box(dims) + (None,)
    f = make(dims, jacobi_iters=4)
    before, _ = check(dims, [(v, t, None)], f)
    rep = capi.MeshReport(7, 7, 7)

    def refused(arr, count, status=capi.FX_E_INVALID, g=f, mask=before):
        ok = lib.fx_set_obstacle_meshes(g._ctx, None, arr, count, C.byref(rep)) == status
        got, cells = g.GetObstacles()
        return ok and np.array_equal(got, mask) and cells == int(mask.sum()) and (rep.solid_cells, rep.open_columns, rep.skipped_triangles) == (7, 7, 7)

    good = c_meshes([other])
    assert refused(good, 0) and refused(None, 1) and refused(None, 0)
    assert refused(c_meshes([other] * 17), 17)
    for size in (0, 36, 39, 44, 48):
        bad = c_meshes([other, other]); bad[1].struct_size = size
        assert refused(bad, 2), size
    for flags in (2, 3, 0x80000000):
        bad = c_meshes([other]); bad[0].flags = flags
        assert refused(bad, 1), flags
    bad = c_meshes([other]); bad[0].positions = None
    assert refused(bad, 1)
    bad = c_meshes([other]); bad[0].indices = None
    assert refused(bad, 1)
    assert lib.fx_set_obstacle_meshes(None, None, good, 1, None) == capi.FX_E_INVALID
    with pytest.raises(fx.FluidxError):
        f.SetObstacleMeshes([])
    with pytest.raises(fx.FluidxError):
        f.SetObstacleMeshes([other] * 17)
    assert np.array_equal(f.GetObstacles()[0], before)
    # ... and the mask is configuration like fx_set_obstacles': kept across UpdateFrame, detached by SetObstacles(None), replaced by either setter
    f.UpdateFrame(f32(0.05), 1)
    assert np.array_equal(f.GetObstacles()[0], before)
    f.SetObstacles(None)
    assert f.GetObstacles()[1] == 0
    done = capi.MeshReport()
    assert lib.fx_set_obstacle_meshes(f._ctx, None, good, 1, C.byref(done)) == capi.FX_OK and done.solid_cells == f.GetObstacles()[1] > 0
    f.SetObstacles(before)
    assert np.array_equal(f.GetObstacles()[0], before)

    # 2-D grids
    flat = make((32, 32, 1), jacobi_iters=4)
    m2 = np.zeros((1, 32, 32), np.uint8); m2[0, 4:9, 5:11] = 1
    flat.SetObstacles(m2)
    assert refused(good, 1, g=flat, mask=m2)
    # faithful contexts (no mask can be in force there)
    fa = make(dims, jacobi_iters=16, jacobi_mode="faithful")
    assert refused(good, 1, g=fa, mask=np.zeros_like(before))
    # the multigrid solver selected
    mg = make(dims, jacobi_iters=4)
    mg.SetPressureSolver("multigrid")
    assert refused(good, 1, status=capi.FX_E_STATE, g=mg, mask=np.zeros_like(before))
    mg.SetPressureSolver("jacobi")
    assert lib.fx_set_obstacle_meshes(mg._ctx, None, good, 1, None) == capi.FX_OK
    # slab ranks and render-only contexts
    r = fx.Fluid()
    assert r.Init(0, 0, (32, 32, 32), slab=(0, 12), halo_advect=6, halo_jacobi=2)
    assert lib.fx_set_obstacle_meshes(r._ctx, None, good, 1, C.byref(rep)) == capi.FX_E_INVALID and r.GetObstacles()[1] == 0
    ro = fx.Fluid()
    assert ro.Init(64, 64, dims, render_only=True)
    assert lib.fx_set_obstacle_meshes(ro._ctx, None, good, 1, C.byref(rep)) == capi.FX_E_STATE
    assert lib.fx_set_obstacle_meshes(ro._ctx, None, None, 0, C.byref(rep)) == capi.FX_E_STATE       # ... whatever else is wrong with the call
    assert (rep.solid_cells, rep.open_columns, rep.skipped_triangles) == (7, 7, 7)
    for o in (f, flat, fa, mg, r, ro):
        o.Release()


# ---- 5: the step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_three_steps_equal_those_of_a_context_given_the_model_s_mask(storage):
    dims = (64, 64, 8)
    X, Y, Z = dims
    c, r = (0.45, 0.5, 0.5), 0.2
    mesh = vr.uv_sphere(c, r, 10, 16) + (vr.translation((1.0 / X, 0.0, 0.0)),)
    want, wrep = vr.voxelise([mesh], dims)
    body = mv.body([x - r - 0.05 for x in c], [x + r + 0.05 for x in c], linear=(0.5, 0.0, 0.1), angular=(0.0, 0.0, 2.0))
    emitter = [er.emitter((0.4, 0.85, 0.5), 0.2, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, -40.0, 3.0), swirl=20.0)]

    def run(setter):
        f = make(dims, storage=storage, jacobi_iters=8)
        f.SetEmitters(emitter)
        f.SetObstacleBodies([body])
        setter(f)
        f.timing_enable(True)
        for k in range(3):
            f.UpdateFrame(f32(2.0 / Y), k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
        t = f.timing_read()
        out = [f.digest(k) for k in ALL_FIELDS], (t.steps, t.jacobi_launches, t.jacobi_sweeps, t.jacobi_main_launches, t.jacobi_main_sweeps)
        vel = f.download(fx.FIELD_VELOCITY)
        f.Release()
        return out, vel

    def by_meshes(f):
        assert f.SetObstacleMeshes([mesh]) == wrep

    a, vel = run(by_meshes)
    b, _ = run(lambda f: f.SetObstacles(want))
    assert a == b and wrep["solid_cells"] > 100
    assert vel[:, want.astype(bool)].any()                             # the body moved the voxelised cells


# ---- 6: the C++ wrapper -------------------------------------------------------------------------------------------------------------------
CXX = r'''
#include "Fluid.hpp"
#include <cstdio>
using namespace fluidx;
int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	const XMUINT3 grid = { 32, 32, 6 };
	Fluid::Options opt;
	opt.storage = FX_STORAGE_FP32; opt.jacobiIters = 4; opt.jacobiMode = FX_JACOBI_FIXED;
	Fluid fluid;
	if (!fluid.Init(nullptr, 0, 0, grid, opt)) return 3;
	const float lo[3] = { 0.25f, 0.125f, 0.25f }, hi[3] = { 0.75f, 0.5f, 0.75f };
	std::vector<float> pos;
	for (int k = 0; k < 8; ++k) { pos.push_back(k & 1 ? hi[0] : lo[0]); pos.push_back(k & 2 ? hi[1] : lo[1]); pos.push_back(k & 4 ? hi[2] : lo[2]); }
	const std::vector<uint32_t> idx = { 0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3, 1, 3, 7, 1, 7, 5, 0, 4, 6, 0, 6, 2 };
	const float shift[12] = { 1, 0, 0, 0.03125f, 0, 1, 0, 0.0625f, 0, 0, 1, 0 };
	fx_mesh_report rep = {};
	if (!fluid.SetObstacleMesh(pos, idx, shift, &rep)) return 4;
	std::vector<uint8_t> mask;
	uint64_t cells = 0;
	if (!fluid.GetObstacles(mask, &cells) || cells != rep.solid_cells || rep.open_columns || rep.skipped_triangles) return 5;
	fx_obstacle_mesh many[17] = {};
	if (fluid.SetObstacleMeshes(many, 17) || fluid.LastStatus() != FX_E_INVALID) return 6;             // the mask in force stays
	if (!fluid.GetObstacles(mask, &cells) || cells != rep.solid_cells) return 7;
	FILE* f = std::fopen(argv[1], "wb");
	if (!f || std::fwrite(mask.data(), 1, mask.size(), f) != mask.size()) return 8;
	return std::fclose(f) ? 9 : 0;
}
'''


def test_the_cxx_wrapper_hands_a_mesh_over(tmp_path):
    import os
    import shutil
    import subprocess
    from fluidx12_amd import build as fxbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cc)
    libdir = os.path.dirname(fxbuild.ensure_built())
    src, exe, out = tmp_path / "mesh.cpp", str(tmp_path / "mesh"), str(tmp_path / "mask.bin")
    src.write_text(CXX)
    subprocess.run([cc, "-std=c++17", "-O1", "-I", os.path.join(root, "fluidx12_amd", "csrc"), str(src), "-o", exe, "-L" + libdir, "-lfluidx_hip",
                    "-Wl,-rpath," + libdir], check=True, timeout=300)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)             # a fresh child process, under its own time limit
    assert r.returncode == 0, (r.returncode, r.stderr)
    dims = (32, 32, 6)
    v = np.array([[(0.75 if k & 1 else 0.25), (0.5 if k & 2 else 0.125), (0.75 if k & 4 else 0.25)] for k in range(8)], f32)
    t = np.array([0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3, 1, 3, 7, 1, 7, 5, 0, 4, 6, 0, 6, 2], np.uint32).reshape(-1, 3)
    want, rep = vr.voxelise([(v, t, vr.translation((0.03125, 0.0625, 0.0)))], dims)
    assert rep["open_columns"] == 0 and rep["solid_cells"] == 16 * 12 * 3
    assert np.array_equal(np.fromfile(out, np.uint8).reshape(want.shape), want)
