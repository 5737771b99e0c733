"""The Jacobi launch planner (fluidx12_amd/csrc/fx_jacobi_plan.cpp) against the schedule recorded from the commit before it.

tests/golden/jacobi_plan.json holds, for every (library, launcher switch, geometry, jacobi_fuse request, freeze mask, sweep count) of its grid, the
launches the scheduling code ran BEFORE the planner existed (read from that commit's own predicates; the commit id is in the file): the kernel
family and the sweeps of every launch of a round, and for the overlapped slab schedule the sweeps per interior launch and the launches of a round
for every member.  The planner is called through its C++ names in the built library -- no device is needed -- and must give the same list for every
entry; every launch of two or more sweeps must be one its family's own jacobi_*_supported() accepts."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "jacobi_plan.json")))
FAMILIES = [None, "sweep1", "tile2d", "strip", "strip3", "strip4", "block2", "blockg"]         # enum JacobiFamily (fx_internal.h)


class Geom(C.Structure):                           # fx_internal.h struct Geom
    _fields_ = [(n, C.c_int) for n in ("X", "Y", "Zg", "z0", "nz", "H", "zlo", "zhi")]


class Launch(C.Structure):                         # struct JacobiLaunch
    _fields_ = [("family", C.c_int), ("sweeps", C.c_int)]


class Policy(C.Structure):                         # struct JacobiPolicy
    _fields_ = [("fam", C.c_int * 5), ("unit", C.c_int), ("three", C.c_int), ("four", C.c_int)]


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
        self.policy = fn("jacobi_policy", Policy, G, C.c_int, C.c_bool, C.c_bool)
        self.plan = fn("jacobi_plan", C.c_int, C.POINTER(Policy), C.c_int, C.POINTER(Launch))
        self.group_sweeps = fn("jacobi_group_sweeps", C.c_int, C.POINTER(Policy), C.c_int)
        self.group_parts = fn("jacobi_group_parts", C.c_int, C.POINTER(Policy), C.c_int, C.c_int, C.POINTER(C.c_int))
        tiles = fn("jacobi2d_max_sweeps", C.c_int, G)
        strip, wide = fn("jacobi_strip_supported", C.c_bool, G), fn("jacobi_strip_wide", C.c_bool, G)
        self.supported = {"tile2d": lambda g, t: t <= tiles(g),
                          "strip": lambda g, t: strip(g) and (t == 2 or (t == 3 and not wide(g))),
                          "strip3": lambda g, t, f=fn("jacobi_strip3_supported", C.c_bool, G): t == 3 and f(g),
                          "strip4": lambda g, t, f=fn("jacobi_strip4_supported", C.c_bool, G): t == 4 and f(g),
                          "block2": lambda g, t, f=fn("jacobi_block2_supported", C.c_bool, G): t == 2 and f(g),
                          "blockg": lambda g, t, f=fn("jacobi_blockg_supported", C.c_bool, G): t == 2 and f(g)}


def expand(text):
    """'2*strip4:4 strip:2' -> [('strip4', 4), ('strip4', 4), ('strip', 2)]"""
    out = []
    for item in text.split():
        n, _, launch = item.rpartition("*")
        family, sweeps = launch.split(":")
        out += [(family, int(sweeps))] * (int(n) if n else 1)
    return out


def check(pl, g, launches, want, count, where, bad):
    if launches != expand(want):
        bad.append((where, "planned", launches, "recorded", want))
    if sum(t for _, t in launches) != count:
        bad.append((where, "sweeps", launches, count))
    for family, t in launches:
        if not ((family == "sweep1" and t == 1) or (family in pl.supported and t >= 1 and pl.supported[family](C.byref(g), t))):
            bad.append((where, "unsupported launch", family, t))


@pytest.mark.parametrize("index", range(len(TABLE["sections"])), ids=["%s-%s" % (s["library"], "=".join(s["knob"]) if s["knob"] else "defaults") for s in TABLE["sections"]])
def test_every_recorded_plan_is_reproduced(index, knob):
    from fluidx12_amd import build, capi
    sec = TABLE["sections"][index]
    if sec["knob"]:
        knob(*sec["knob"])                       # a lab switch moves the test onto the lab build (conftest.knob)
    elif sec["library"] == "lab":
        pytest.fail("a lab section without a switch")
    lib = capi.load()
    path = os.environ.get("FLUIDX_LIB_PATH") or build.LIB
    assert (sec["library"] == "lab") == (path != build.LIB), (sec["library"], path)
    pl = Planner(lib, path)
    bad, seen = [], 0
    for r in sec["rounds"]:
        g, fuse, frozen = geom(r["geom"]), r.get("fuse", 0), r.get("frozen", 0)
        pol = pl.policy(C.byref(g), fuse, frozen != 0, frozen == 2)
        for count, want in r["plans"].items():
            count = int(count)
            out = (Launch * count)()
            n = pl.plan(C.byref(pol), count, out)
            check(pl, g, [(FAMILIES[out[i].family], out[i].sweeps) for i in range(n)], want, count, (r["geom"], fuse, frozen, count), bad)
            seen += 1
    for grp in sec["groups"]:
        members = [geom(v) for v in grp["members"]]
        pol = (Policy * (len(members) + 1))()     # the lead (the first member), then every member: what jacobi_all collects
        for i, g in enumerate([members[0]] + members):
            pol[i] = pl.policy(C.byref(g), grp["fuse"], False, False)
        t = pl.group_sweeps(pol, len(pol))
        if t != grp["t"]:
            bad.append((grp["name"], grp["fuse"], "sweeps per interior launch", t, grp["t"]))
        for cnt, want in grp["rounds"].items():
            cnt = int(cnt)
            parts = (C.c_int * cnt)()
            m = pl.group_parts(C.byref(pol[0]), t, cnt, parts)
            for i, g in enumerate(members):
                check(pl, g, [(FAMILIES[pol[i + 1].fam[min(parts[j], 4)]], parts[j]) for j in range(m)], want[i], cnt, (grp["name"], grp["fuse"], grp["k"], cnt, i), bad)
            seen += 1
    assert not bad, (len(bad), bad[:8])
    assert seen == sum(len(r["plans"]) for r in sec["rounds"]) + sum(len(grp["rounds"]) for grp in sec["groups"]) and seen > 0


def test_the_table_is_whole():
    """every entry belongs to a section the test above runs: nothing recorded is left unchecked"""
    n = sum(len(r["plans"]) for s in TABLE["sections"] for r in s["rounds"]) + sum(len(g["rounds"]) for s in TABLE["sections"] for g in s["groups"])
    assert n == TABLE["entries"] and n > 4000
    assert re.fullmatch(r"[0-9a-f]{40}", TABLE["parent"])
    assert {s["library"] for s in TABLE["sections"]} == {"shipped", "lab"}
