"""CPU checks of the particle sort (fx_set_particle_sort, fx_sort_particles): the numpy model tests/particle_sort_ref.py against its plain-loop
twin on edge records, the C ABI surface without a device, and the planner (fx::psort_plan of csrc/fx_particle_sort_plan.cpp) linked into a small
program -- also under the address and undefined-behaviour sanitizers.  tests/test_gpu_particle_sort.py holds the kernels against the model."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import particle_ref as pr
import particle_sort_ref as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CALLS = ("fx_set_particle_sort", "fx_get_particle_sort", "fx_sort_particles", "fx_particle_sort_info", "fx_particle_order_device")
GRIDS = ps.SHAPES + [(3, 3, 2), (256, 256, 256), (512, 512, 512), (1024, 1024, 1024)]
PLAN_COUNTS = (0, 1, 1 << 26)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(ps.bits(a), ps.bits(b))


# ---- the model against its twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(7, 6, 5), (9, 4, 1), (5, 3, 2)])
def test_the_vectorised_model_is_the_loop_model(dims):
    for name in ps.ARRANGEMENTS:
        for n in (1, 2, 97):
            rec = ps.arrangement(name, dims, n, seed=n)
            assert np.array_equal(ps.keys(rec, dims), ps.keys_loops(rec, dims)), (name, n)
            a, b = ps.sort(rec, dims), ps.sort_loops(rec, dims)
            assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (name, n)
            assert a[1].dtype == np.uint32 and sorted(a[1].tolist()) == list(range(n))
            k = ps.keys(a[0], dims)
            cells = dims[0] * dims[1] * dims[2]
            assert (np.diff(k.astype(np.int64)) >= 0).all() and (k[:a[2]] < cells).all() and (k[a[2]:] == cells).all()


def test_the_rule_by_hand():
    dims = (8, 4, 2)
    top = np.nextafter(f32(1), f32(0))
    rec = np.array([[0.5, 0.5, 0.5, 0.0],            # cell (4, 2, 1)
                    [np.nan, -np.inf, -0.0, 1.0],    # cell (0, 0, 0)
                    [1.0, np.inf, 1e30, -0.0],       # the last cell; -0.0 is live
                    [top, top, top, 2.0],            # the last cell too
                    [0.5, 0.5, 0.5, -1e-45],         # dead
                    [0.5, 0.5, 0.5, np.nan],         # dead
                    [0.124, 0.26, 0.49, 3.0]], f32)  # cell (0, 1, 0)
    want = np.array([(1 * 4 + 2) * 8 + 4, 0, 63, 63, 64, 64, 8], np.uint32)
    assert np.array_equal(ps.keys(rec, dims), want)
    out, order, live = ps.sort(rec, dims)
    assert order.tolist() == [1, 6, 0, 2, 3, 4, 5] and live == 5 and same_bits(out, rec[order])
    flat = np.array([[0.5, 0.5, 7.0, 0.0], [0.5, 0.5, np.nan, 0.0]], f32)                 # a 2-D grid does not look at z
    assert ps.keys(flat, (8, 4, 1)).tolist() == [2 * 8 + 4] * 2
    # dead records keep their bits and their order, NaN payloads included
    dead = ps.arrangement("all_dead", dims, 33)
    out, order, live = ps.sort(dead, dims)
    assert live == 0 and order.tolist() == list(range(33)) and same_bits(out, dead)
    assert len(set(ps.bits(dead[:, 3]).tolist())) == 33


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx_with_the_sort_calls(tmp_path):
    src = tmp_path / "sort_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'typedef char sort_is_16[sizeof(fx_particle_sort) == 16 ? 1 : -1];\n'
                   'typedef char info_is_16[sizeof(struct fx_particle_sort_info) == 16 ? 1 : -1];\n'
                   'static int (*set_)(fx_ctx*, const fx_particle_sort*) = fx_set_particle_sort;\n'
                   'static int (*get_)(fx_ctx*, fx_particle_sort*) = fx_get_particle_sort;\n'
                   'static int (*sort_)(fx_ctx*, void*) = fx_sort_particles;\n'
                   'static int (*info_)(fx_ctx*, void*, struct fx_particle_sort_info*) = fx_particle_sort_info;\n'
                   'static int (*dev_)(fx_ctx*, void**, void**) = fx_particle_order_device;\n'
                   'int main(void) { (void)set_; (void)get_; (void)sort_; (void)info_; (void)dev_; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        val = tmp_path / "sort_values.c"
        val.write_text('#include "fluidx_hip.h"\nint main(void) { return sizeof(fx_particle_sort) == 16 && sizeof(struct fx_particle_sort_info) == 16 && '
                       'FX_ABI_VERSION == 7 ? 0 : 1; }\n')
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
    assert capi.SYMBOLS["fx_set_particle_sort"] == (C.c_int, [vp, C.POINTER(capi.ParticleSort)])
    assert capi.SYMBOLS["fx_particle_sort_info"] == (C.c_int, [vp, vp, C.POINTER(capi.ParticleSortInfo)])
    assert capi.SYMBOLS["fx_particle_order_device"] == (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)])
    assert C.sizeof(capi.ParticleSort) == 16 and C.sizeof(capi.ParticleSortInfo) == 16 and capi.ABI_VERSION == 7
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetParticleSort", "GetParticleSort", "SortParticles", "ParticleSortInfo", "ParticleOrderDevice"):
        assert callable(getattr(fx.Fluid, name)) and name in hpp, name
    assert callable(fx.Fluid.ParticleOrder)
    for name in CALLS:
        assert name in hpp, name
    assert "fx_particle_sort.hip" in build.SOURCES and "fx_particle_sort_plan.cpp" in build.SOURCES
    assert "PSORT_KEY_BITS" in capi.LAB_KNOBS and "PSORT_KEY_BITS" not in capi.knob_names()      # the shipped switch list does not grow


def test_a_null_context_is_refused():
    from fluidx12_amd import capi
    lib = capi.load()
    cfg, info = capi.ParticleSort(16, 0, 1, 0), capi.ParticleSortInfo(16, 77, 78, 79)
    a, b = C.c_void_p(5), C.c_void_p(6)
    assert lib.fx_set_particle_sort(None, C.byref(cfg)) == capi.FX_E_INVALID and lib.fx_set_particle_sort(None, None) == capi.FX_E_INVALID
    assert lib.fx_get_particle_sort(None, C.byref(cfg)) == capi.FX_E_INVALID and cfg.enabled == 1
    assert lib.fx_sort_particles(None, None) == capi.FX_E_INVALID
    assert lib.fx_particle_sort_info(None, None, C.byref(info)) == capi.FX_E_INVALID and (info.live, info.sorts, info.reserved) == (77, 78, 79)
    assert lib.fx_particle_order_device(None, C.byref(a), C.byref(b)) == capi.FX_E_INVALID and (a.value, b.value) == (5, 6)


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------
def check_plan(run, dims, count, force=0):
    k = run("k")
    cells = dims[0] * dims[1] * dims[2]
    p = run(cells, count, force)
    assert p["rc"] == 0 and p["cells"] == cells and p["count"] == count
    natural = cells.bit_length()
    assert p["bits"] == max(natural, min(force, 32))
    d = p["digit_bits"]
    assert len(d) == p["passes"] == -(-p["bits"] // k["max_digit_bits"]) <= k["max_passes"]
    assert sum(d) == p["bits"] and all(1 <= w <= k["max_digit_bits"] for w in d)            # no digit wider than the histogram the kernels hold
    assert p["shift"] == [sum(d[:i]) for i in range(len(d))]
    assert p["records_per_wg"] == k["records"] == k["threads"] * k["items"]
    assert p["wgs"] * p["records_per_wg"] >= count and (p["wgs"] == 0 or (p["wgs"] - 1) * p["records_per_wg"] < count)
    assert p["scan_entries"] == [p["wgs"] << w for w in d]
    assert p["scan_blocks"] == [-(-e // k["scan_tile"]) for e in p["scan_entries"]]
    # the scratch block: live, order, index, two key arrays, the records, the histogram, the block sums -- in this order, aligned, none overlapping
    al = k["align"]
    up = lambda v: -(-v // al) * al
    sizes = [al, 4 * count, 4 * count, 4 * count, 4 * count, 16 * count, 4 * max(p["scan_entries"]), 4 * max(p["scan_blocks"])]
    at = 0
    for off, size in zip(p["offsets"], sizes):
        assert off == at and off % al == 0
        at += up(size)
    assert p["scratch_bytes"] == at
    return p


@pytest.fixture(scope="module")
def plain():
    exe = ps.build_planner()
    return functools.lru_cache(maxsize=None)(lambda *a: ps.run_planner(exe, *a))


@pytest.fixture(scope="module")
def sanitized():
    exe = ps.build_planner(["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], name="psort_probe_san")
    return functools.lru_cache(maxsize=None)(lambda *a: ps.run_planner(exe, *a))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_planner(which, request):
    run = request.getfixturevalue(which)
    for dims in GRIDS:
        cells = dims[0] * dims[1] * dims[2]
        counts = list(PLAN_COUNTS) + ps.COUNTS + (ps.threshold_counts(dims) if which == "plain" else [])
        for count in counts:
            p = check_plan(run, dims, count)
            assert p["bits"] == cells.bit_length()
            forced = check_plan(run, dims, count, 32)                                     # PSORT_KEY_BITS = 32: four passes on any grid
            assert forced["bits"] == 32 and forced["passes"] == 4 and forced["passes"] >= p["passes"]
            assert check_plan(run, dims, count, 3)["bits"] == p["bits"]                   # never fewer bits than the dead key needs
    assert check_plan(run, (256, 256, 256), 1 << 20)["digit_bits"] == [7, 6, 6, 6]       # 25 bits
    assert [check_plan(run, d, 1)["bits"] for d in ps.SHAPES] == [13, 15, 11, 19, 5]
    # refused: no cells, 2^32 - 1 cells and more, more records than FX_MAX_PARTICLES
    for cells, count in ((0, 1), (0xFFFFFFFF, 1), (1 << 32, 1), (1 << 40, 0), (1000, (1 << 26) + 1)):
        assert run(cells, count, 0) == {"rc": -1}
    assert run(0xFFFFFFFE, 1, 0)["bits"] == 32


def test_the_thresholds_the_gpu_tests_read():
    k = ps.constants()
    for dims in ps.SHAPES + ps.GPU_SHAPES:
        below, at, above, second = ps.threshold_counts(dims)
        cells = dims[0] * dims[1] * dims[2]
        assert (ps.planner(cells, below)["wgs"], ps.planner(cells, at)["wgs"], ps.planner(cells, above)["wgs"]) == (1, 1, 2)
        assert max(ps.planner(cells, second - 1)["scan_blocks"]) == 1 and max(ps.planner(cells, second)["scan_blocks"]) == 2
    assert k["records"] >= 256 and k["scan_tile"] >= 256


def test_the_counts_that_reach_a_second_round_of_block_sums():
    """tests/test_gpu_particle_sort.py sorts these two on (70, 70, 5): 15 key bits as digits of 8 + 7, the widest digit the kernels have"""
    k = ps.constants()
    dims = (70, 70, 5)
    cells = dims[0] * dims[1] * dims[2]
    assert ps.planner(cells, 1)["digit_bits"] == [8, 7] and k["max_digit_bits"] == 8
    single, second = ps.scan_round_counts(dims)
    assert max(ps.planner(cells, single)["scan_blocks"]) == k["threads"] == 256              # the last single round ...
    assert max(ps.planner(cells, single + 1)["scan_blocks"]) == k["threads"] + 1             # ... one record more starts the second
    assert max(ps.planner(cells, second)["scan_blocks"]) == 260 and max(ps.planner(cells, second - 1)["scan_blocks"]) == 259
    assert 2_000_000 < single < second < 2_200_000 <= k["max_count"]
    # no count the GPU tests sorted so far gets there, on any of their grids
    for d in ps.SHAPES + ps.GPU_SHAPES:
        for n in ps.COUNTS + ps.threshold_counts(d):
            assert max(ps.planner(d[0] * d[1] * d[2], n)["scan_blocks"]) <= k["threads"], (d, n)
