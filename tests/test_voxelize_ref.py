"""Anchors of the voxeliser's numpy model (tests/voxelize_ref.py), which tests/test_gpu_voxelize.py holds the device to bit for bit: known
cell counts, geometric bounds, closedness across the walls, the invariances the atomic scatter relies on, exact shifts; and the host-side
pieces of fx_set_obstacle_meshes that need no GPU (the header's declarations, the argument check)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import voxelize_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIMS = (40, 24, 20)


def centres(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid((np.arange(Z) + 0.5) / Z, (np.arange(Y) + 0.5) / Y, (np.arange(X) + 0.5) / X, indexing="ij")
    return x, y, z


def test_a_box_on_cell_centres_is_all_ties():
    v, t = vr.box_mesh(vr.cell_centre(DIMS, (8, 4, 4)), vr.cell_centre(DIMS, (30, 19, 15)))
    q, fin = vr.quantise(vr.transform(v, None), DIMS)
    assert fin.all() and ((q - 128) % 256 == 0).all()                 # every corner ON a centre: every face is a tie
    mask, rep = vr.voxelise([(v, t, None)], DIMS)
    assert rep == {"solid_cells": 22 * 15 * 11, "open_columns": 0, "skipped_triangles": 0}
    want = np.zeros_like(mask)
    # the sample sits at (-eps^2, +eps) off the centre in (y, z): the low z and the HIGH y face are in; along x the toggle is at the first
    # centre at or beyond the plane: the low x face is in, the high one out
    want[4:15, 5:20, 8:30] = 1
    assert np.array_equal(mask, want)


def test_a_uv_sphere_is_closed_and_lies_between_its_bounds():
    r = 0.3
    v, t = vr.uv_sphere((0.5, 0.5, 0.5), r, 12, 24)
    mask, rep = vr.voxelise([(v, t, None)], DIMS)
    x, y, z = centres(DIMS)
    d = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    assert mask[d <= 0.95 * r].all() and not mask[d > 1.001 * r].any()
    assert rep["open_columns"] == 0 and rep["skipped_triangles"] == 0
    assert rep["solid_cells"] == 2112


@pytest.mark.parametrize("cx", [0.9, -0.05])
def test_a_sphere_across_an_x_wall_stays_closed(cx):
    v, t = vr.uv_sphere((cx, 0.5, 0.5), 0.3, 12, 24)
    mask, rep = vr.voxelise([(v, t, None)], DIMS)
    assert rep["open_columns"] == 0 and rep["solid_cells"] > 0
    assert mask[:, :, -1].any() if cx > 0.5 else mask[:, :, 0].any()   # ... and it does reach the wall


def test_the_result_ignores_triangle_order_vertex_order_and_winding():
    rng = np.random.default_rng(5)
    for v, t in (vr.uv_sphere((0.45, 0.55, 0.5), (0.3, 0.25, 0.35), 9, 14), vr.torus((0.5, 0.5, 0.5), 0.27, 0.12),
                 vr.box_mesh(vr.cell_centre(DIMS, (8, 4, 4)), vr.cell_centre(DIMS, (30, 19, 15)))):
        base, rep = vr.voxelise([(v, t, None)], DIMS)
        assert rep["open_columns"] == 0 and rep["solid_cells"] > 100
        for variant in (t[rng.permutation(len(t))], np.roll(t, 1, axis=1), np.roll(t, 2, axis=1), t[:, ::-1],
                        np.where((np.arange(len(t)) % 3 == 0)[:, None], t[:, ::-1], np.roll(t, 1, axis=1))):
            got, rep2 = vr.voxelise([(v, np.ascontiguousarray(variant), None)], DIMS)
            assert np.array_equal(got, base) and rep2 == rep


def test_a_whole_cell_shift_through_the_transform_shifts_the_mask():
    dims = (64, 32, 16)                                               # powers of two: k / N and the products are exact in fp32
    v, t = vr.uv_sphere((0.4, 0.5, 0.5), 0.21, 10, 16)
    v = (np.round(v.astype(np.float64) * 2 ** 18) / 2 ** 18).astype(f32)   # ... and so are the sums: the positions are multiples of 2^-18
    base, rep = vr.voxelise([(v, t, vr.translation((0, 0, 0)))], dims)
    assert np.array_equal(base, vr.voxelise([(v, t, None)], dims)[0]) and rep["open_columns"] == 0
    for k in ((5, 0, 0), (0, -3, 0), (0, 0, 2), (7, 4, -3)):
        got, rep2 = vr.voxelise([(v, t, vr.translation([k[a] / dims[a] for a in range(3)]))], dims)
        assert rep2 == rep
        assert np.array_equal(got, np.roll(base, (k[2], k[1], k[0]), axis=(0, 1, 2)))


def test_an_open_mesh_is_reported():
    v, t = vr.uv_sphere((0.5, 0.5, 0.5), 0.3, 12, 24)
    a = vr.toggles(v, t, None, DIMS)[0]
    for drop in range(0, len(t), 37):
        one = vr.toggles(v, t[drop:drop + 1], None, DIMS)[0]
        if one.any():                                                 # a triangle that covers a column
            _, rep = vr.voxelise([(v, np.delete(t, drop, axis=0), None)], DIMS)
            assert rep["open_columns"] == int(one.sum()) > 0
            break
    else:
        pytest.fail("no triangle covered a column")
    assert a.sum() % 2 == 0


def test_bad_geometry_is_counted_not_refused():
    v, t = vr.uv_sphere((0.5, 0.5, 0.5), 0.3, 8, 12)
    base, rep = vr.voxelise([(v, t, None)], DIMS)
    bad_v = np.vstack([v, [[np.nan, 0.5, 0.5]], [[0.5, np.inf, 0.5]]]).astype(f32)
    n = len(v)
    extra = np.array([[0, 1, n + 2], [0, 1, 0xFFFFFFFF], [0, n, 2], [n + 1, 1, 2], [3, 3, 4], [5, 5, 5]], np.uint32)
    got, rep2 = vr.voxelise([(bad_v, np.vstack([t, extra]), None)], DIMS)
    assert np.array_equal(got, base)                                  # out-of-range, NaN, inf: skipped; a repeated index: no area
    assert rep2 == dict(rep, skipped_triangles=4)
    # a coordinate that overflows only in the quantising multiply is finite: clamped, not skipped
    far = np.array([[0.5, 0.5, 0.5], [3e38, 0.5, 0.5], [0.5, 3e38, 0.5]], f32)
    _, rep3 = vr.voxelise([(far, np.array([[0, 1, 2]], np.uint32), None)], DIMS)
    assert rep3["skipped_triangles"] == 0
    assert vr.voxelise([(np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32), None)], DIMS)[1] == {"solid_cells": 0, "open_columns": 0, "skipped_triangles": 0}


def test_the_union_keeps_the_overlap_solid():
    a = vr.uv_sphere((0.4, 0.5, 0.5), 0.25, 10, 16)
    b = vr.uv_sphere((0.6, 0.5, 0.5), 0.25, 10, 16)
    ma, mb = vr.voxelise([a + (None,)], DIMS)[0], vr.voxelise([b + (None,)], DIMS)[0]
    both, rep = vr.voxelise([a + (None,), b + (None,)], DIMS)
    assert (ma & mb).sum() > 50 and np.array_equal(both, ma | mb) and rep["open_columns"] == 0
    # ... where one mesh holding both spheres is hollow there: XOR within a mesh, OR across meshes
    v = np.vstack([a[0], b[0]])
    t = np.vstack([a[1], b[1] + len(a[0])])
    assert np.array_equal(vr.voxelise([(v, t, None)], DIMS)[0], ma ^ mb)


# ---- the header and the argument check ---------------------------------------------------------------------------------------------------
def test_the_header_declares_the_mesh_setter(tmp_path):
    from fluidx12_amd import capi
    assert capi.SYMBOLS["fx_set_obstacle_meshes"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(capi.ObstacleMesh), C.c_uint32, C.POINTER(capi.MeshReport)])
    assert C.sizeof(capi.ObstacleMesh) == 40 and C.sizeof(capi.MeshReport) == 16 and capi.MAX_OBSTACLE_MESHES == 16 and capi.MESH_DEVICE == 1
    assert capi.ABI_VERSION == 7
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src, exe = tmp_path / "mesh_abi.c", str(tmp_path / "mesh_abi")
    src.write_text('#include "fluidx_hip.h"\n#include <stddef.h>\n'
                   'int main(void) { fx_obstacle_mesh m; fx_mesh_report r; m.struct_size = sizeof m; r.solid_cells = 0; (void)r;\n'
                   '  return sizeof(fx_obstacle_mesh) == 40 && offsetof(fx_obstacle_mesh, positions) == 8 && offsetof(fx_obstacle_mesh, vertex_count) == 24 &&\n'
                   '    offsetof(fx_obstacle_mesh, transform) == 32 && sizeof(fx_mesh_report) == 16 && offsetof(fx_mesh_report, open_columns) == 8 &&\n'
                   '    FX_MAX_OBSTACLE_MESHES == 16u && FX_MESH_DEVICE == 0x1u && FX_ABI_VERSION == 7 && m.struct_size == 40 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0


ARGS_CXX = r'''
#include "fx_mesh_args.h"
#include <vector>
int main()
{
	using namespace fx;
	const float pos[9] = { 0 };
	const uint32_t idx[3] = { 0, 1, 2 };
	fx_obstacle_mesh good = { (uint32_t)sizeof(fx_obstacle_mesh), 0u, pos, idx, 3u, 1u, nullptr };
	std::vector<fx_obstacle_mesh> list(17, good);                       // heap: a read past `count` entries is out of bounds
	list.shrink_to_fit();
	if (mesh_args_status(list.data(), 1) != FX_OK || mesh_args_status(list.data(), 16) != FX_OK) return 1;
	if (mesh_args_status(list.data(), 0) != FX_E_INVALID || mesh_args_status(list.data(), 17) != FX_E_INVALID) return 2;
	if (mesh_args_status(nullptr, 1) != FX_E_INVALID || mesh_args_status(nullptr, 0) != FX_E_INVALID) return 3;
	if (mesh_args_status(nullptr, 0xFFFFFFFFu) != FX_E_INVALID) return 4;
	for (uint32_t size : { 0u, 36u, 39u, 41u, 48u }) { list[3] = good; list[3].struct_size = size; if (mesh_args_status(list.data(), 4) != FX_E_INVALID) return 5; }
	for (uint32_t flags : { 2u, 3u, 0x80000000u }) { list[3] = good; list[3].flags = flags; if (mesh_args_status(list.data(), 4) != FX_E_INVALID) return 6; }
	list[3] = good; list[3].flags = FX_MESH_DEVICE;
	if (mesh_args_status(list.data(), 4) != FX_OK) return 7;
	list[3] = good; list[3].positions = nullptr;
	if (mesh_args_status(list.data(), 4) != FX_E_INVALID || mesh_args_status(list.data(), 3) != FX_OK) return 8;
	list[3] = good; list[3].indices = nullptr;
	if (mesh_args_status(list.data(), 4) != FX_E_INVALID) return 9;
	list[3].positions = nullptr; list[3].triangle_count = 0;            // no triangles: both may be NULL
	if (mesh_args_status(list.data(), 4) != FX_OK) return 10;
	// the work buffer: the list of large triangles, and a host mesh's copy behind it
	list[0] = good; list[0].triangle_count = 1000; list[0].vertex_count = 600; list[0].flags = FX_MESH_DEVICE;
	if (mesh_work_bytes(list.data(), 1) != 16000) return 11;
	list[0].flags = 0;
	if (mesh_work_bytes(list.data(), 1) != 16000 + 12000 + 7200 + 48) return 12;
	list[1] = good; list[1].triangle_count = 0xFFFFFFFFu; list[1].flags = FX_MESH_DEVICE;
	if (mesh_work_bytes(list.data(), 2) != (size_t)16 * 0xFFFFFFFFu) return 13;
	if (mesh_work_bytes(list.data() + 3, 1) != 16) return 14;
	return 0;
}
'''


def test_the_argument_check_in_a_stand_alone_program(tmp_path):
    """fx_set_obstacle_meshes' argument check is host code with no HIP in it (csrc/fx_mesh_args.h): built into a program of its own with the
    host compiler's address and undefined-behaviour sanitizers, it refuses what the header says it refuses and reads nothing else"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src, exe = tmp_path / "mesh_args.cpp", str(tmp_path / "mesh_args")
    src.write_text(ARGS_CXX)
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fluidx12_amd", "csrc"), str(src), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)                              # a toolchain without the sanitizers' runtimes: the plain build
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
