"""numpy model of the particle sort (include/fluidx_hip.h fx_set_particle_sort / fx_sort_particles, fluidx12_amd/csrc/fx_particle_sort.hip).

The rule: a record (x, y, z, age) is live iff age >= 0; its cell per axis is min((int)(c(p_a) * (float)N_a), N_a - 1) in fp32, c = particle_ref.c01
(a 2-D grid does not look at z); its key is (c_z Y + c_y) X + c_x, or X Y Z when it is dead; the buffer becomes rec[order] with order the stable
ascending permutation of the keys, and live counts the live records.  Everything is integers and bit patterns: the GPU tests compare as uint32.
`keys` / `sort` are vectorised, `keys_loops` / `sort_loops` their plain-loop twins (tests/test_particle_sort_ref.py holds one against the other).

`arrangements` builds the buffers the GPU tests sort; `planner` is fx::psort_plan of csrc/fx_particle_sort_plan.cpp linked into a small program
of its own (host compiler, no device), which is where the tests read the kernels' constants from."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import particle_ref as pr

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluidx12_amd", "csrc")

SHAPES = list(pr.SHAPES) + [(5, 3, 2)]                # keys of 11 to 19 bits, and one of 5: a single pass
# fx_create takes grids with X == Y only (the reference asserts it), so no context can hold (5, 3, 2): on the device the single pass runs on
# (3, 3, 2), 18 cells, the same 5 key bits; the model and the planner, which know no such limit, keep (5, 3, 2)
GPU_SHAPES = list(pr.SHAPES) + [(3, 3, 2)]
COUNTS = [1, 2, 255, 256, 257, 4099, 65537, (1 << 18) + 1]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def keys(rec, dims):
    """uint32 key of every record"""
    X, Y, Z = dims
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        live = rec[:, 3] >= 0
    c = []
    for a, n in enumerate(dims):
        if a == 2 and Z == 1:
            c.append(np.zeros(len(rec), np.int64))
            continue
        s = pr.c01(rec[:, a])
        c.append(np.minimum((s * f32(n)).astype(f32).astype(np.int64), n - 1))
    k = (c[2] * Y + c[1]) * X + c[0]
    return np.where(live, k, X * Y * Z).astype(np.uint32)


def sort(rec, dims):
    """-> (the sorted records, order (uint32: where the record now at i stood), live)"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    k = keys(rec, dims)
    order = np.argsort(k, kind="stable")
    live = int((k < dims[0] * dims[1] * dims[2]).sum())
    return rec.view(np.uint32)[order].view(f32), order.astype(np.uint32), live


# ---- the same in plain loops ---------------------------------------------------------------------------------------------------------------
def keys_loops(rec, dims):
    X, Y, Z = dims
    out = []
    for x, y, z, age in np.ascontiguousarray(rec, f32).reshape(-1, 4):
        if not age >= 0:
            out.append(X * Y * Z)
            continue
        c = []
        for v, n in ((x, X), (y, Y), (z, Z)):
            v = f32(v)
            s = f32(0) if (v != v or v <= 0) else (f32(1) if v > 1 else v)
            c.append(min(int(f32(s * f32(n))), n - 1))
        if Z == 1:
            c[2] = 0
        out.append((c[2] * Y + c[1]) * X + c[0])
    return np.array(out, np.uint32).reshape(-1)


def sort_loops(rec, dims):
    """an insertion sort that never passes an equal key: stable by construction"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    k = [int(v) for v in keys_loops(rec, dims)]
    order = []
    for i in range(len(k)):
        j = len(order)
        while j > 0 and k[order[j - 1]] > k[i]:
            j -= 1
        order.insert(j, i)
    order = np.array(order, np.int64).reshape(-1)
    live = sum(1 for v in k if v < dims[0] * dims[1] * dims[2])
    return rec.view(np.uint32)[order].view(f32), order.astype(np.uint32), live


# ---- the buffers the tests sort ------------------------------------------------------------------------------------------------------------
def centre(dims, cell):
    """the centre of cell (i, j, k) in texture space"""
    return [f32((cell[a] + 0.5) / dims[a]) for a in range(3)]


def nan_ages(n):
    """n dead ages: NaNs of distinct payloads and both signs"""
    w = (np.uint32(0x7FC00000) + np.arange(1, n + 1, dtype=np.uint32) * np.uint32(3)) | ((np.arange(n, dtype=np.uint32) & np.uint32(1)) << np.uint32(31))
    return w.view(f32)


ARRANGEMENTS = ("random", "one_cell", "two_cells", "live_dead", "all_dead", "all_live", "sorted", "reversed", "edges", "ages")


def arrangement(name, dims, n, seed=0):
    """n records of the arrangement `name` (float32 (n, 4))"""
    rng = np.random.default_rng(9000 + seed)
    rec = pr.records(dims, n, 700 + seed)                                 # uniform random, the edge set first, every fifth record dead
    if name == "random":
        return rec
    if name == "one_cell":                                                # all live in one cell, every record distinct: stability decides every position
        c = centre(dims, [d // 2 for d in dims])
        rec[:, :3] = c
        rec[:, 3] = np.arange(n, dtype=f32)
        rec[:, 0] += (rng.random(n).astype(f32) - f32(0.5)) * f32(0.5 / dims[0])
    elif name == "two_cells":
        a, b = centre(dims, [d - 1 for d in dims]), centre(dims, [0, 0, 0])
        rec[:, :3] = np.where((np.arange(n) % 2 == 0)[:, None], np.array(a, f32), np.array(b, f32))
        rec[:, 3] = np.arange(n, dtype=f32)
    elif name == "live_dead":
        rec[:, 3] = np.where(np.arange(n) % 2 == 0, rng.random(n).astype(f32), f32(-1) - np.arange(n, dtype=f32))
    elif name == "all_dead":
        rec[:, 3] = np.where(np.arange(n) % 2 == 0, f32(-1) - np.arange(n, dtype=f32), nan_ages(n))
    elif name == "all_live":
        rec[:, 3] = rng.random(n).astype(f32)
    elif name in ("sorted", "reversed"):
        rec = sort(rec, dims)[0].copy()
        if name == "reversed":
            rec = rec[::-1].copy()
    elif name == "edges":                                                 # the edge positions with live ages, as often as they fit
        e = pr.edge_points(dims)
        m = min(len(e), n)
        rec[:m, :3] = e[:m]
        top = np.nextafter(f32(1), f32(0))                                # the largest float below 1
        if n > m:
            rec[m:, :3] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -0.25, 1.5, top], f32), (n - m, 3))
        rec[:, 3] = rng.random(n).astype(f32)
    elif name == "ages":                                                  # dead NaNs of distinct payloads, -0.0 (live) and the smallest negative (dead)
        pick = np.arange(n) % 4
        ages = rng.random(n).astype(f32)
        ages = np.where(pick == 0, nan_ages(n), ages)
        ages = np.where(pick == 1, f32(-0.0), ages)
        ages = np.where(pick == 2, np.array(-1e-45, f32), ages)
        rec[:, 3] = ages
    else:
        raise ValueError(name)
    return np.ascontiguousarray(rec, f32)


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
PROBE = r"""
// fx::psort_plan through its own header: cells count force_bits -> the plan, one "name values..." line per member
#include "fx_particle_sort_plan.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
	if (argc == 2 && argv[1][0] == 'k') {
		printf("threads %u\nitems %u\nrecords %u\nmax_digit_bits %u\nmax_passes %u\nscan_tile %u\nmax_count %u\nalign %zu\n", fx::kPsortThreads, fx::kPsortItems,
			fx::kPsortRecords, fx::kPsortDigitBits, fx::kPsortMaxPasses, fx::kPsortScanTile, fx::kPsortMaxCount, fx::kPsortAlign);
		return 0;
	}
	if (argc != 4) return 2;
	fx::PsortPlan p;
	const int rc = fx::psort_plan(strtoull(argv[1], nullptr, 10), (uint32_t)strtoul(argv[2], nullptr, 10), atoi(argv[3]), &p);
	printf("rc %d\n", rc);
	if (rc) return 0;
	printf("cells %u\ncount %u\nbits %u\npasses %u\nwgs %u\nrecords_per_wg %u\n", p.cells, p.count, p.bits, p.passes, p.wgs, p.records_per_wg);
	printf("digit_bits"); for (uint32_t i = 0; i < p.passes; ++i) printf(" %u", p.digit_bits[i]); printf("\n");
	printf("shift"); for (uint32_t i = 0; i < p.passes; ++i) printf(" %u", p.shift[i]); printf("\n");
	printf("scan_entries"); for (uint32_t i = 0; i < p.passes; ++i) printf(" %u", p.scan_entries[i]); printf("\n");
	printf("scan_blocks"); for (uint32_t i = 0; i < p.passes; ++i) printf(" %u", p.scan_blocks[i]); printf("\n");
	printf("offsets %zu %zu %zu %zu %zu %zu %zu %zu\n", p.off_live, p.off_order, p.off_index, p.off_keys[0], p.off_keys[1], p.off_records, p.off_hist, p.off_sums);
	printf("scratch_bytes %zu\n", p.scratch_bytes);
	return 0;
}
"""

_dirs = []


def build_planner(extra=(), name="psort_probe"):
    """the planner and the probe above compiled by the host compiler with `extra` flags -> the program's path"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler")
    d = tempfile.TemporaryDirectory(prefix="psort_plan_")
    _dirs.append(d)                                                       # (removed when the interpreter exits)
    src, exe = os.path.join(d.name, "probe.cpp"), os.path.join(d.name, name)
    with open(src, "w") as fh:
        fh.write(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + list(extra) + ["-I", CSRC, src, os.path.join(CSRC, "fx_particle_sort_plan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def run_planner(exe, *args):
    out = {}
    for line in subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        out[w[0]] = v[0] if len(v) == 1 and w[0] not in ("digit_bits", "shift", "scan_entries", "scan_blocks") else v
    return out


@functools.lru_cache(maxsize=None)
def _exe():
    return build_planner()


@functools.lru_cache(maxsize=None)
def constants():
    """the kernels' constants (csrc/fx_particle_sort_plan.h): threads, items, records (per workgroup), max_digit_bits, max_passes, scan_tile ..."""
    return run_planner(_exe(), "k")


@functools.lru_cache(maxsize=None)
def planner(cells, count, force_bits=0):
    """fx::psort_plan(cells, count, force_bits) as a dict; {"rc": -1} where it refuses"""
    return run_planner(_exe(), cells, count, force_bits)


def threshold_counts(dims):
    """one below, at and one above the records of a workgroup, and the first count whose histogram needs a second scan block on this grid"""
    k = constants()
    cells = dims[0] * dims[1] * dims[2]
    widest = max(planner(cells, 1)["digit_bits"])
    wgs = k["scan_tile"] // (1 << widest) + 1                             # the first workgroup count whose (1 << widest) * wgs passes one tile
    return [k["records"] - 1, k["records"], k["records"] + 1, (wgs - 1) * k["records"] + 1]


SCAN_ROUND_EXTRA = 4                                                      # block sums the second round holds at the least: more than one


def scan_round_counts(dims):
    """k_psort_scan_sums scans the block sums in rounds of one per thread and carries a running total from round to round: -> [the largest count
    whose widest pass still has `threads` scan blocks, the last single round; the first count with threads + SCAN_ROUND_EXTRA of them]"""
    k = constants()
    cells = dims[0] * dims[1] * dims[2]
    widest = max(planner(cells, 1)["digit_bits"])
    last_single = (k["threads"] * k["scan_tile"]) >> widest               # workgroups: (wgs << widest) entries fill `threads` tiles exactly
    blocks = k["threads"] + SCAN_ROUND_EXTRA
    first_wgs = -(-((blocks - 1) * k["scan_tile"] + 1) // (1 << widest))    # the first workgroup count whose entries reach into tile `blocks`
    return [last_single * k["records"], (first_wgs - 1) * k["records"] + 1]
