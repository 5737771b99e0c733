"""The obstacle draw (fx_set_obstacle_draw), CPU side: the C ABI surface and the numpy model of tests/obstacle_draw_ref.py -- vectorised against
plain loops, the conditions the GPU tests' scene is chosen under, and the walk held to a float64 sampling of the ray that knows nothing of
planes or steps.

The scene: a ball, a slab on the floor that touches the y and z walls (rays enter the box straight into it) and a beam through both x walls, on
32^3, 30 x 30 x 18 (ragged bricks) and 32 x 32 x 16; the default camera, its opposite, an axis-aligned one on 65 x 65 (a row and a column of rays
with a zero component) and one inside the box.

What the model gives at 32^3 (rays that enter the box / hits / face codes 0 .. 5): default 200 x 150: 11662 / 2490 / 9, 0, 971, 0, 0, 1510,
140 of the hits start hits; opposite: 11662 / 2254 / 0, 159, 0, 579, 1516, 0, 484 start hits; axis 65 x 65: 4225 / 911, at most 47 advances;
inside: 30000 / 28809.  Face code 6 -- a start hit with no entry axis -- needs the eye inside a solid cell: by the rule the entry axis is the
axis whose quotient became U, and every ray from outside has one.  (A prototype that read the entry axis off which component of the moved
origin equals +-1 exactly finds none on 47 and 81 of these start hits, where the fma rounds to 0.99999994; the rule as written has no such
pixels.)  The inside camera with a solid block around the eye covers code 6."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import obstacle_draw_ref as od

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
VP, SMALL, AXIS = (200, 150), (67, 41), (65, 65)
ALBEDO = (0.8, 0.7, 0.6, 2.0)
# camera, viewport, (X, Z)
SCENES = [("default", VP, (32, 32)), ("opposite", VP, (32, 32)), ("axis", AXIS, (32, 32)), ("inside", VP, (32, 32)), ("default", SMALL, (32, 32)),
          ("default", SMALL, (30, 18)), ("opposite", SMALL, (32, 16))]

_CACHE = {}


def scene(cam, vp, grid, light=None):
    """(mask, frame constants, the model's draw) computed once"""
    key = (cam, vp, grid, None if light is None else tuple(sorted((k, str(v)) for k, v in light.items())))
    if key not in _CACHE:
        S = od.scene_mask(*grid)
        view, proj, eye = od.cameras(cam, *vp)
        fr = od.frame(view, proj, eye, vp[0], vp[1], grid[0], light=light)
        _CACHE[key] = (S, fr, od.draw(S, fr, vp[0], vp[1], ALBEDO))
    return _CACHE[key]


def eye_cell(fr, grid):
    """the cell the eye of an inside camera lies in"""
    q = od.local_point(fr, fr["eye"])
    N = (grid[0], grid[0], grid[1])
    return tuple(min(max(int(np.floor((float(q[a]) * 0.5 + 0.5) * N[a])), 0), N[a] - 1) for a in range(3))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_abi_offers_the_obstacle_draw():
    from fluidx12_amd import capi
    import fluidx12_amd as fx
    src = open(os.path.join(ROOT, "include", "fluidx_hip.h")).read()
    names = ("fx_set_obstacle_draw", "fx_get_obstacle_draw", "fx_draw_obstacles", "fx_obstacle_depth_device", "fx_obstacle_hits")
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.load(), name)
    assert re.search(r"typedef\s+struct\s+fx_obstacle_draw\s*\{", src)
    assert C.sizeof(capi.ObstacleDraw) == 24
    assert "sizeof(fx_obstacle_draw) = 24" in src
    assert int(re.search(r"#define\s+FX_ABI_VERSION\s+(\d+)", src).group(1)) == capi.ABI_VERSION == 7
    lib = capi.load()
    assert lib.fx_set_obstacle_draw(None, None) == capi.FX_E_INVALID
    assert lib.fx_get_obstacle_draw(None, None) == capi.FX_E_INVALID
    assert lib.fx_draw_obstacles(None, None, 0, None) == capi.FX_E_INVALID
    assert lib.fx_obstacle_depth_device(None, None) == capi.FX_E_INVALID
    assert lib.fx_obstacle_hits(None, None, 0, None, None, None, 0) == capi.FX_E_INVALID
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for m in ("SetObstacleDraw", "DrawObstacles", "AttachObstacleDepth", "ObstacleHits"):
        assert callable(getattr(fx.Fluid, m)), m
        assert m in hpp, m


# ---- vectorised == loops ------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_twin(S, fr, vp, target=None, scene_depth=None):
    D = od.draw(S, fr, vp[0], vp[1], ALBEDO, target, scene_depth)
    L = od.draw_loops(S, fr, vp[0], vp[1], ALBEDO, target, scene_depth)
    for name, b in zip(("hits", "depth", "target_float", "target"), L):
        assert same_bits(D[name], b), name
    return D


@pytest.mark.parametrize("cam,vp,grid", SCENES)
def test_vectorised_equals_loops(cam, vp, grid):
    S, fr, D = scene(cam, vp, grid)
    L = od.draw_loops(S, fr, vp[0], vp[1], ALBEDO)
    for name, b in zip(("hits", "depth", "target_float", "target"), L):
        assert same_bits(D[name], b), name
    assert D["cast"]["hit"].sum() > 100 and D["cast"]["drawn"].any()


def test_vectorised_equals_loops_with_lights_a_scene_depth_a_target_and_the_eye_in_a_solid():
    from test_depth_ref import analytic_depth
    vp, grid = SMALL, (30, 18)
    S = od.scene_mask(*grid)
    target = np.random.default_rng(2).integers(0, 256, (vp[1], vp[0], 4)).astype(np.uint8)
    view, proj, eye = od.cameras("default", *vp)
    for light in ({"kind": "directional", "position": (-30.0, 50.0, -20.0), "color": (0.2, 0.9, 0.5, 4.0), "ambient": (0.5, 0.4, 0.9, 0.7)},
                  {"kind": "point", "position": (2.0, 6.0, -7.0)}):
        fr = od.frame(view, proj, eye, vp[0], vp[1], grid[0], light=light)
        D = check_twin(S, fr, vp, target)
        dr = D["cast"]["drawn"].reshape(vp[1], vp[0])
        assert dr.any() and np.array_equal(D["target"][~dr], target[~dr]) and (D["target"][dr][:, 3] == 255).all()
    depth = analytic_depth(proj, vp[0], vp[1], plane=(0.3, 0.2, float(np.linalg.norm(eye))))
    fr = od.frame(view, proj, eye, vp[0], vp[1], grid[0])
    D = check_twin(S, fr, vp, target, depth)
    C = D["cast"]
    hidden = C["hit"] & ~C["drawn"]
    assert hidden.any() and C["drawn"].any()
    assert np.array_equal(D["depth"].reshape(-1)[~C["drawn"]], depth.reshape(-1)[~C["drawn"]])
    # the eye inside a solid block: every pixel a start hit with no entry axis -- face code 6, ambient light alone
    view, proj, eye = od.cameras("inside", *vp)
    fr = od.frame(view, proj, eye, vp[0], vp[1], grid[0])
    x, y, z = eye_cell(fr, grid)
    S6 = S.copy()
    S6[max(z - 3, 0):z + 4, max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = True    # (the rays start on the near plane, 1 / 10 of the box's half width from the eye)
    D = check_twin(S6, fr, vp)
    C = D["cast"]
    assert C["start"].all() and (C["face"] == 6).all()
    assert ((D["hits"] >> np.uint64(32)) & np.uint64(7) == 6).all()
    # (p is the near plane's point, cz = 0 up to rounding: drawn or clipped pixel by pixel.)  What is drawn has one colour
    print("eye in a solid: drawn", int(C["drawn"].sum()), "of", len(C["drawn"]))
    lit = D["target_float"].reshape(-1, 4)[C["drawn"]]
    assert len(np.unique(lit.view(np.uint32), axis=0)) <= 1


# ---- the conditions on the scene -------------------------------------------------------------------------------------------------------------------
def test_the_scene_shows_every_face_and_both_ways_into_the_box():
    faces = np.zeros(7, np.int64)
    for cam in ("default", "opposite"):
        C = scene(cam, VP, (32, 32))[2]["cast"]
        n = np.bincount(C["face"][C["hit"]], minlength=7)
        print(cam, "rays", int(C["rays"]["ok"].sum()), "hits", int(C["hit"].sum()), "faces", n.tolist(), "start hits", int(C["start"].sum()))
        assert C["hit"].sum() >= 2000 and C["start"].sum() >= 20
        assert (C["hit"] & ~C["start"]).sum() >= 1000
        faces += n
    assert (faces[:6] >= 5).all()
    C = scene("axis", AXIS, (32, 32))[2]["cast"]
    d, ok = C["rays"]["d"], C["rays"]["ok"]
    assert (ok & (d[:, 0] == 0)).sum() >= 50 and (ok & (d[:, 1] == 0)).sum() >= 50
    assert C["advances"].max() <= 48 and C["hit"].sum() >= 800
    C = scene("inside", VP, (32, 32))[2]["cast"]
    assert C["rays"]["ok"].all() and (C["rays"]["e"] == -1).all() and C["hit"].sum() >= 25000
    base = {cam: int(scene(cam, VP, (32, 32))[2]["cast"]["hit"].sum()) for cam in ("default", "opposite")}
    for grid in ((30, 18), (32, 16)):                                  # ragged bricks and a flat grid draw the same scene
        for cam in ("default", "opposite"):
            S = od.scene_mask(*grid)
            view, proj, eye = od.cameras(cam, *VP)
            n = int(od.cast(S, od.frame(view, proj, eye, VP[0], VP[1], grid[0]), *VP)["hit"].sum())
            print(grid, cam, n, base[cam])
            assert abs(n - base[cam]) <= 0.1 * base[cam]


def test_the_words_carry_the_cell_the_face_and_the_flags():
    S, fr, D = scene("default", VP, (32, 32))
    C, w = D["cast"], D["hits"].reshape(-1)
    assert np.array_equal(w != 0, C["hit"]) and np.array_equal((w >> np.uint64(63)) == 1, C["hit"])
    assert np.array_equal(((w >> np.uint64(62)) & np.uint64(1)) == 1, C["drawn"])
    cell = (w & np.uint64(0xFFFFFFFF)).astype(np.int64)[C["hit"]]
    assert S.reshape(-1)[cell].all()                                   # every hit names a solid cell
    assert not (w & np.uint64(0x3FFFFFF800000000)).any()
    assert (D["depth"].reshape(-1)[~C["drawn"]] == 1).all() and (D["depth"].reshape(-1)[C["drawn"]] < 1).all()


# ---- the walk against a sampling of the ray ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam,vp", [("default", VP), ("opposite", VP), ("axis", AXIS)])
def test_the_walk_agrees_with_a_float64_sampling_of_the_ray(cam, vp):
    """3501 points over t in [0, 3.5] (the box's diagonal is 3.47) per ray that enters the box, each looked up in the mask in float64: no ray
    that hit has a solid sample more than 2e-3 in front of its hit, no ray that missed has three solid samples in a row.  The limit is zero rays."""
    S, fr, D = scene(cam, vp, (32, 32))
    C = D["cast"]
    Z, Y, X = S.shape
    N = np.array([X, Y, Z])
    ok = np.nonzero(C["rays"]["ok"])[0]
    t = np.linspace(0.0, 3.5, 3501)
    early = runs = 0
    for lo in range(0, len(ok), 500):
        idx = ok[lo:lo + 500]
        o, d = C["rays"]["o"][idx].astype(np.float64), C["rays"]["d"][idx].astype(np.float64)
        p = o[:, None, :] + t[None, :, None] * d[:, None, :]
        inside = (np.abs(p) <= 1).all(2)
        c = np.clip(np.floor((p * 0.5 + 0.5) * N).astype(np.int64), 0, N - 1)
        solid = inside & S[c[..., 2], c[..., 1], c[..., 0]]
        hit = C["hit"][idx]
        early += int((solid & (t[None, :] < C["t"][idx].astype(np.float64)[:, None] - 2e-3))[hit].any(1).sum())
        three = solid[:, :-2] & solid[:, 1:-1] & solid[:, 2:]
        runs += int(three[~hit].any(1).sum())
    print(cam, "rays", len(ok), "hit rays with a solid sample in front of the hit", early, "missed rays with three solid samples in a row", runs)
    assert early == 0 and runs == 0
