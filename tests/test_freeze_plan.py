"""The faithful solve's launch policy (fluidx12_amd/csrc/fx_jacobi_plan.cpp: freeze_*) against what the commit before it ran.

tests/golden/freeze_plan.json holds what that commit's fx_schedule.cpp decided inside jacobi_freeze (its own lines, compiled unchanged around stubs;
the commit id is in the file), as the full product of its axes: whether the sparse solver runs; the launches of a solve -- the dense sweep with one
or two copies of level 1, strip launches of four or three levels, tile launches -- for every geometry class, third mask buffer, count of strip
launches in use and value of the four switches; the hysteresis on the count of relaxing tiles; which generations count and which take a count over.
The planner is called through its C++ names in the built library -- no device is needed -- and must give the same answer for every entry."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "freeze_plan.json")))
ITERS, GEOMS = TABLE["iters"], TABLE["geoms"]
CASES = [(name, third, n) for name in GEOMS for third in (0, 1) for n in (0, 1, 2)]      # the order of a block's maps
SLOTS = 128                                        # kFreezeSlots (fx_internal.h)
DENSE, DENSE_ONE, STRIP, TILES = range(4)          # enum FreezeKind


class Geom(C.Structure):                           # fx_internal.h struct Geom
    _fields_ = [(n, C.c_int) for n in ("X", "Y", "Zg", "z0", "nz", "H", "zlo", "zhi")]


class Launch(C.Structure):                         # struct FreezeLaunch
    _fields_ = [("kind", C.c_int), ("levels", C.c_int), ("base", C.c_int)]


class Cadence(C.Structure):                        # struct FreezeCadence
    _fields_ = [("count", C.c_bool), ("take_over", C.c_bool)]


def geom(v):
    X, Y, Zg = v[:3]
    z0, nz, H = v[3:] if len(v) > 3 else (0, Zg, 0)
    return Geom(X, Y, Zg, z0, nz, H, max(z0 - H, 0), min(z0 + nz + H, Zg) - 1)


class Planner:
    def __init__(self, lib, path):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout

        def fn(name, res, *args):
            names = re.findall(r"\b(_ZN2fx%d%sE\w+)" % (len(name), name), syms)
            assert len(names) == 1, (name, names)
            f = getattr(lib, names[0])
            f.restype, f.argtypes = res, list(args)
            return f
        G = C.POINTER(Geom)
        self.takes = fn("freeze_takes_sparse_solver", C.c_bool, G, C.c_uint32, C.c_bool, C.c_bool, C.c_int)
        self.plan = fn("freeze_plan", C.c_int, G, C.c_uint32, C.c_bool, C.c_bool, C.c_int, C.POINTER(Launch))
        self.hysteresis = fn("freeze_strip_hysteresis", C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_bool)
        self.cadence = fn("freeze_cadence", Cadence, C.c_uint32)
        self.predicates = {"freeze": fn("jacobi_freeze_supported", C.c_bool, G), "strip": fn("jacobi_freeze_strip_supported", C.c_bool, G),
                           "strip4": fn("jacobi_freeze_strip4_supported", C.c_bool, G), "tiles": fn("jacobi_freeze_tiles", C.c_int, G)}


def planner(library, knob, lab_switch=None):
    """the planner of the shipped or the lab library; a lab switch (at its default here) moves the test onto the lab build (conftest.knob)"""
    from fluidx12_amd import build, capi
    if library == "lab":
        knob(*(lab_switch or ("FREEZE_T", "4")))
    lib = capi.load()
    path = os.environ.get("FLUIDX_LIB_PATH") or build.LIB
    assert (library == "lab") == (path != build.LIB), (library, path)
    return Planner(lib, path)


def expand(text):
    """'D1 2*s4 t4 t3' -> [(DENSE_ONE, 1, 0), (STRIP, 4, 1), (STRIP, 4, 5), (TILES, 4, 9), (TILES, 3, 13)]: kind, levels, the level it starts from"""
    items = text.split()
    out, level = [({"D1": DENSE_ONE, "D2": DENSE}[items[0]], 1, 0)], 1
    for item in items[1:]:
        n, _, launch = item.rpartition("*")
        for _ in range(int(n) if n else 1):
            out.append(({"s": STRIP, "t": TILES}[launch[0]], int(launch[1:]), level))
            level += int(launch[1:])
    return out


MAPS = [[None if t == "-" else expand(t) for t in m.split("|")] for m in TABLE["maps"]]


@pytest.mark.parametrize("index", range(len(TABLE["sections"])), ids=["%s-dense_levels=%d" % (s["library"], s["dense_levels"]) for s in TABLE["sections"]])
def test_every_recorded_plan_is_reproduced(index, knob):
    sec = TABLE["sections"][index]
    lab = sec["library"] == "lab"
    pl = planner(sec["library"], knob, ("FREEZE_DENSE_LEVELS", str(sec["dense_levels"])))
    geoms = {name: geom(v) for name, v in GEOMS.items()}
    strip = {name: pl.predicates["strip"](C.byref(g)) for name, g in geoms.items()}
    strip4 = {name: pl.predicates["strip4"](C.byref(g)) for name, g in geoms.items()}
    out = (Launch * SLOTS)()
    bad, seen = [], 0
    for blk in sec["blocks"]:
        knob("FREEZE_STRIP4", str(blk["strip4"]))
        if lab:
            knob("FREEZE_DENSE_ONE", str(blk["dense_one"]))
            knob("FREEZE_T", str(blk["T"]))
        else:
            assert (sec["dense_levels"], blk["dense_one"], blk["T"]) == (-1, 1, 4)       # the shipped library has these at their defaults
        assert len(blk["maps"]) == len(CASES)
        for (name, third, n), m in zip(CASES, blk["maps"]):
            g, slab = geoms[name], len(GEOMS[name]) > 3
            for iters, want in zip(ITERS, MAPS[m]):
                where = (blk, name, third, n, iters)
                seen += 1
                if pl.takes(C.byref(g), iters, True, slab, g.nz) != (want is not None):
                    bad.append((where, "sparse solver", want is not None))
                if want is None:
                    continue
                count = pl.plan(C.byref(g), iters, slab, bool(third), n, out)
                got = [(out[i].kind, out[i].levels, out[i].base) for i in range(count)]
                if got != want or not 1 <= count <= SLOTS:
                    bad.append((where, "planned", got, "recorded", want))
                if 1 + sum(l for _, l, _ in got[1:]) != iters:
                    bad.append((where, "levels", got))
                if any(k == STRIP and not (strip[name] and third and not slab and (l == 3 or (l == 4 and strip4[name]))) for k, l, _ in got):
                    bad.append((where, "unsupported strip launch", got))
    assert not bad, (len(bad), bad[:6])
    assert seen == len(sec["blocks"]) * len(CASES) * len(ITERS)


@pytest.mark.parametrize("index", range(len(TABLE["takes"])), ids=["%s-T=%d" % (s["library"], s["T"]) for s in TABLE["takes"]])
def test_whether_the_sparse_solver_runs(index, knob):
    sec = TABLE["takes"][index]
    pl = planner(sec["library"], knob, ("FREEZE_T", str(sec["T"])))
    assert sec["library"] == "lab" or sec["T"] == 4
    for key, digits in sec["rows"].items():
        name, masks, min_nz = key.split("/")
        g = geom(GEOMS[name])
        got = "".join("01"[pl.takes(C.byref(g), iters, masks == "1", len(GEOMS[name]) > 3, int(min_nz))] for iters in ITERS)
        assert got == digits, key


@pytest.mark.parametrize("library", ["shipped", "lab"])
def test_hysteresis_and_cadence(library, knob):
    pl = planner(library, knob)
    (hyst,), (cad,) = [s for s in TABLE["hysteresis"] if s["library"] == library], [s for s in TABLE["cadence"] if s["library"] == library]
    for key, steps in hyst["rows"].items():
        tiles, four, n = (int(x) for x in key.split("/"))
        want = []
        for (a, v), nxt in zip(steps, steps[1:] + [[tiles + 1, None]]):
            want += [v] * (nxt[0] - a)
        assert len(want) == tiles + 1
        assert [pl.hysteresis(n, active, tiles, bool(four)) for active in range(tiles + 1)] == want, key
    got = [pl.cadence(gen) for gen in range(1, 17)]
    assert [gen for gen, c in zip(range(1, 17), got) if c.count] == cad["count"]
    assert [gen for gen, c in zip(range(1, 17), got) if c.take_over] == cad["take_over"]


def test_the_geometries_cover_every_class():
    """what the table says of its geometries is what the built predicates say, and every class occurs"""
    from fluidx12_amd import build, capi
    pl = Planner(capi.load(), os.environ.get("FLUIDX_LIB_PATH") or build.LIB)
    for name, v in GEOMS.items():
        g = geom(v)
        assert {k: int(f(C.byref(g))) for k, f in pl.predicates.items()} == TABLE["predicates"][name], name
    p = TABLE["predicates"]
    assert p["octet"]["strip"] and p["octet"]["strip4"] and p["strip3"]["strip"] and not p["strip3"]["strip4"]
    assert all(p[n]["freeze"] and not p[n]["strip"] for n in ("shallow", "g128", "g150", "slab4")) and not p["slab2"]["freeze"]
    assert (GEOMS["slab4"][5], GEOMS["slab2"][5]) == (4, 2)


def test_the_table_is_whole():
    """every entry belongs to a section a test above runs: nothing recorded is left unchecked"""
    n = sum(len(b["maps"]) * len(ITERS) for s in TABLE["sections"] for b in s["blocks"]) + sum(len(s["rows"]) * len(ITERS) for s in TABLE["takes"])
    n += sum(int(k.split("/")[0]) + 1 for s in TABLE["hysteresis"] for k in s["rows"]) + 16 * len(TABLE["cadence"])
    assert n == TABLE["entries"] and n > 180000
    assert re.fullmatch(r"[0-9a-f]{40}", TABLE["parent"])
    for part in ("sections", "takes", "hysteresis", "cadence"):
        assert {s["library"] for s in TABLE[part]} == {"shipped", "lab"}, part
    lab = [s for s in TABLE["sections"] if s["library"] == "lab"]
    assert sorted(s["dense_levels"] for s in lab) == [-1, 0, 3, 4, 6, 7, 8, 9, 11, 12, 16]
    assert all(sorted((b["strip4"], b["dense_one"], b["T"]) for b in s["blocks"]) == [(a, b, t) for a in (0, 1) for b in (0, 1) for t in (1, 2, 3, 4)] for s in lab)
    assert all(len(m.split("|")) == len(ITERS) for m in TABLE["maps"]) and ITERS == [*range(1, 13), 16, 17, 20, 23, 40, 63, 64, 65, 100, 255, 256]
    assert {k.split("/")[0] for s in TABLE["hysteresis"] for k in s["rows"]} == {"96", "1000"} and all(len(s["rows"]) == 12 for s in TABLE["hysteresis"])
