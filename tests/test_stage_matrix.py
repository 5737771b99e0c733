"""Which kernel serves which shape, asked of the library itself (no device): fx::sim_row_kernel (fluidx12_amd/csrc/fx_sim.hip) is the one
function both launch_divergence and launch_project take their kernel from.  tests/test_gpu_stage_matrix.py compares every storage x row-class
kernel of the two families with the oracle on a table of shapes; this module checks that the table still reaches every kernel -- with one
shape whose row fits a single block along x and one with more than 64 threads along x that ends in a partial block -- so that a changed
launcher rule cannot quietly leave a kernel without a parity test.  Also fx::digest_range_ok, the range rule of fx_field_digest: 64-bit sums,
so no z_begin + z_count can wrap past it."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_gpu_stage_matrix as matrix
from test_jacobi_plan import FAMILIES, Geom, Launch, Planner, expand, geom

SCALAR, VW2, VW3, V4 = 0, 2, 3, 4                       # enum SimRowKernel (fx_internal.h): cells per thread along the row, 0 = the scalar kernel
NAMES = {"scalar": SCALAR, "vw2": VW2, "vw3": VW3, "v4": V4}
DIVERGENCE, PROJECT = 0, 1                               # enum SimStage
# the kernels of DESIGN.md section 2 rows a-2 / a-4 for 3-D grids: storage -> the row classes it has
FAMILY = {"fp32": ("v4", "vw3", "vw2", "scalar"), "fp16": ("v4", "vw2", "scalar")}


@pytest.fixture(scope="module")
def host():
    from fluidx12_amd import build, capi
    lib = capi.load()
    path = os.environ.get("FLUIDX_LIB_PATH") or build.LIB
    syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout

    def fn(name, res, *args):
        names = re.findall(r"\b(_ZN2fx%d%sE\w+)" % (len(name), name), syms)
        assert len(names) == 1, (name, names)
        f = getattr(lib, names[0])
        f.restype, f.argtypes = res, list(args)
        return f

    class Host:
        row_kernel = fn("sim_row_kernel", C.c_int, C.POINTER(Geom), C.c_int, C.c_int, C.c_int)
        range_ok = fn("digest_range_ok", C.c_bool, C.POINTER(Geom), C.c_uint32, C.c_uint32)
    return Host


def row_class(host, dims, storage, stage):
    g = geom(dims)
    return host.row_kernel(C.byref(g), int(storage == "fp16"), stage, int(dims[2] > 1))


def test_every_shape_takes_the_kernel_the_table_says(host):
    assert len(set(matrix.SHAPES)) == len(matrix.SHAPES) == len(matrix.ROW_CLASS)
    for dims in matrix.SHAPES:
        assert dims[0] == dims[1] and dims[2] > 1, dims                     # square planes (fx_create), 3-D
        for k, storage in enumerate(("fp32", "fp16")):
            for stage in (DIVERGENCE, PROJECT):
                assert row_class(host, dims, storage, stage) == NAMES[matrix.ROW_CLASS[dims][k]], (dims, storage, stage)


@pytest.mark.parametrize("stage", [DIVERGENCE, PROJECT])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_every_kernel_is_reached_by_a_small_and_a_wide_shape(host, storage, stage):
    """every cell of the storage x row-class table: a shape whose row is one block along x, and one with more than 64 threads along x whose
    last block is partial (a workgroup's last lane has a neighbour in the next block; lanes beyond the row are switched off)"""
    small, wide = set(), set()
    for dims in matrix.SHAPES:
        c = row_class(host, dims, storage, stage)
        threads = dims[0] // (c or 1)                                        # the launchers' XW / X4 (scalar: one cell per thread)
        if threads <= 64:
            small.add(c)
        elif threads % 64:
            wide.add(c)
    want = {NAMES[n] for n in FAMILY[storage]}
    assert small == want and wide == want, (storage, stage, small, wide)


def test_two_dimensional_grids_and_the_step_cases_stay_where_they_were(host):
    for storage in ("fp32", "fp16"):
        for X in (36, 64, 70, 150):                                         # Z = 1: the scalar kernels, whatever divides the row
            assert row_class(host, (X, X, 1), storage, DIVERGENCE) == SCALAR and row_class(host, (X, X, 1), storage, PROJECT) == SCALAR
    # slabs: the class is the whole grid's unless the 16-byte alignment of the component planes is lost (cells_local() & 3)
    for dims, slab, c32, c16 in (((70, 70, 24), (12, 12, 6), VW2, VW2), ((35, 35, 24), (8, 8, 6), SCALAR, SCALAR), ((201, 201, 18), (0, 9, 6), VW3, SCALAR),
                                 ((36, 36, 24), (8, 8, 6), V4, V4), ((6, 6, 9), (3, 3, 0), VW3, VW2)):
        g = geom(dims + slab)
        for stage in (DIVERGENCE, PROJECT):
            assert host.row_kernel(C.byref(g), 0, stage, 1) == c32 and host.row_kernel(C.byref(g), 1, stage, 1) == c16, (dims, slab, stage)
    for c in matrix.STEP_CASES:                                              # one whole-step case per class and storage, in both Jacobi modes
        assert c["dims"] in matrix.SHAPES
    for storage in FAMILY:
        for mode in ("fixed", "faithful"):
            got = {matrix.ROW_CLASS[c["dims"]][storage == "fp16"] for c in matrix.STEP_CASES if c["storage"] == storage and c["mode"] == mode}
            assert got == set(FAMILY[storage]), (storage, mode, got)


def test_the_subnormal_cases_run_the_launches_they_name():
    """the Jacobi launches test_gpu_stage_matrix.py::test_fp32_subnormal_fields_bit_exact counts are the planner's for the default schedule, and
    between them the cases reach every family the shipped planner hands out"""
    from fluidx12_amd import build, capi
    pl = Planner(capi.load(), os.environ.get("FLUIDX_LIB_PATH") or build.LIB)
    seen = set()
    for dims, mode, sweeps, plan in matrix.SUBNORMAL_CASES:
        if mode != "fixed":
            continue
        g = geom(dims)
        pol = pl.policy(C.byref(g), 0, False, False)
        out = (Launch * sweeps)()
        n = pl.plan(C.byref(pol), sweeps, out)
        got = [(FAMILIES[out[i].family], out[i].sweeps) for i in range(n)]
        assert got == expand(plan) and n == matrix.launches_of(plan), (dims, sweeps, got, plan)
        seen |= {f for f, _ in got}
    assert seen == set(FAMILIES[1:]), seen
    assert [c for c in matrix.SUBNORMAL_CASES if c[1] == "faithful"]
    assert {c[0] for c in matrix.SUBNORMAL_CASES} >= set(matrix.SHAPES)


GEOMS = [(64, 64, 64), (6, 6, 2), (150, 150, 7), (64, 64, 1), (64, 64, 64, 0, 16, 6), (64, 64, 64, 16, 32, 8), (64, 64, 64, 48, 16, 4), (35, 35, 24, 8, 8, 6),
         (8, 8, 100, 3, 5, 2)]


@pytest.mark.parametrize("v", GEOMS)
def test_digest_range_rule(host, v):
    """planes [z_begin, z_begin + z_count) must be owned ones; z_count = 0 stands for all of them.  A 32-bit sum let (5, 0xFFFFFFFF) through:
    5 + 0xFFFFFFFF wraps to 4, and the digest kernel then read 2^32 - 1 planes"""
    g = geom(v)
    z0, nz = g.z0, g.nz
    ok = lambda a, n: bool(host.range_ok(C.byref(g), a, n))
    top = 0xFFFFFFFF
    for a, n in ((5, top), (0, nz + 1), (z0, nz + 1), (z0 + nz, 1), (z0 + nz - 1, 2), (z0 + 1, nz), (z0 + 1, top), (z0, top), (top, 1), (top, 2), (top, top),
                 (z0 + nz, top - nz + 1), (z0 + 1, top - 1), (1 << 31, 1 << 31), ((1 << 31) + z0, nz), (z0, (1 << 31) + 1)):
        assert not ok(a, n), (v, a, n)
    if z0 > 0:
        assert not ok(z0 - 1, 1) and not ok(z0 - 1, nz) and not ok(0, 1)
    for a, n in ((z0, nz), (z0, 1), (z0 + nz - 1, 1), (z0, 0), (z0 + nz // 2, nz - nz // 2)):
        assert ok(a, n), (v, a, n)
    # ... and every small pair against the rule in Python's integers
    for a in list(range(0, z0 + nz + 3)) + [top - 1, top]:
        for n in list(range(1, nz + 3)) + [top - a, top - a + 1 + z0, top]:
            n &= top
            if n:
                assert ok(a, n) == (z0 <= a and a + n <= z0 + nz), (v, a, n)


def test_digest_refuses_what_ctypes_would_truncate():
    """Fluid.digest hands its range to a uint32_t pair: 2^32 + 1 planes would arrive as one plane, -1 as 2^32 - 1"""
    import fluidx12_amd as fx
    f = fx.Fluid()
    for a, n in ((-1, 1), (0, -1), (1 << 32, 1), (0, (1 << 32) + 1), (0, 1 << 32), (-(1 << 32), 0)):
        with pytest.raises(ValueError):
            f.digest(fx.FIELD_PRESSURE, a, n)
