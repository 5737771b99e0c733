"""Scene depth (fx_set_scene_depth, the reference's _HAS_DEPTH_MAP_ variants), CPU side: the C ABI surface, and the depth-aware CPU
reference of tests/depth_ref/ -- anchored to the oracle (a far-plane depth buffer changes no byte) and checked on a toy case (a depth
buffer in front of the volume leaves every ray its first sample only: the shaders sample, then test t > tMax)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_u8 = C.POINTER(C.c_uint8)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- the reference: built from tests/depth_ref/ + the oracle's other sources with the oracle's flags ---------------------------------
_SRCS = [os.path.join(ROOT, "tests", "depth_ref", s) for s in ("orc_depth_render.cpp", "orc_depth_resolve.cpp")]
_ORACLE = [os.path.join(ROOT, "oracle", s) for s in ("orc_sim.cpp", "orc_host.cpp", "orc_sh.cpp", "orc_bc6h.cpp", "orc_render.cpp",
                                                      "orc_resolve.cpp", "orc_common.h", "fx_oracle.h")]
_LIB = None


def depth_ref_lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "_build", "liborcdepth.so")
        deps = _SRCS + _ORACLE
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = ["-O3", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2"]   # oracle/Makefile
            subprocess.run(["g++"] + flags + ["-shared", "-o", out] + _SRCS + [p for p in _ORACLE if p.endswith(".cpp") and
                           not p.endswith(("orc_render.cpp", "orc_resolve.cpp"))] + ["-lm"], check=True)
        _LIB = C.CDLL(out)
    return _LIB


@pytest.fixture(scope="module")
def dref():
    return depth_ref_lib()


def ref_direct(col, lm, fr, wvp_i, W, H, ns, nl, sh, separate, depth):
    col = np.ascontiguousarray(col, f32)
    Z, Y, X, _ = col.shape
    out = np.empty((H, W, 4), f32)
    cov = np.empty((H, W), np.uint8)
    lmp = _fp(np.ascontiguousarray(lm, f32)) if lm is not None else None
    depth_ref_lib().orcd_raycast_direct(_fp(col), lmp, X, Y, Z, C.byref(fr), _fp(np.ascontiguousarray(wvp_i, f32)), W, H, ns, nl, int(sh),
                                        int(separate), _fp(np.ascontiguousarray(depth, f32)), _fp(out), cov.ctypes.data_as(_u8))
    return out, cov


def ref_view(col, lm, fr, size, mask, ns, nl, sh, separate, depth, wvp, wvp_i, cube_depth=None):
    """(cube float, cube RGBA8, cube depth): texels without a ray keep 0 / 0 / what cube_depth held (default 1.0)"""
    col = np.ascontiguousarray(col, f32)
    Z, Y, X, _ = col.shape
    H, W = depth.shape
    cf = np.zeros((6, size, size, 4), f32)
    cu = np.zeros((6, size, size, 4), np.uint8)
    cd = np.ones((6, size, size), f32) if cube_depth is None else np.array(cube_depth, f32)
    lmp = _fp(np.ascontiguousarray(lm, f32)) if lm is not None else None
    depth_ref_lib().orcd_raymarch_view(_fp(col), lmp, X, Y, Z, C.byref(fr), size, mask, ns, nl, int(sh), int(separate),
                                       _fp(np.ascontiguousarray(depth, f32)), W, H, _fp(np.ascontiguousarray(wvp, f32)),
                                       _fp(np.ascontiguousarray(wvp_i, f32)), _fp(cf), cu.ctypes.data_as(_u8), _fp(cd))
    return cf, cu, cd


def ref_resolve(cube_u8, cube_depth, fr, wvp_i, depth, zn=1.0, zf=1000.0):
    cube_u8 = np.ascontiguousarray(cube_u8, np.uint8)
    N = cube_u8.shape[1]
    H, W = depth.shape
    out = np.empty((H, W, 4), f32)
    cov = np.empty((H, W), np.uint8)
    depth_ref_lib().orcd_resolve_cube(cube_u8.ctypes.data_as(_u8), _fp(np.ascontiguousarray(cube_depth, f32)), N, C.byref(fr),
                                      _fp(np.ascontiguousarray(wvp_i, f32)), W, H, _fp(np.ascontiguousarray(depth, f32)),
                                      C.c_float(zn), C.c_float(zf), _fp(out), cov.ctypes.data_as(_u8))
    return out, cov


# ---- scenes and depth buffers --------------------------------------------------------------------------------------------------------
def smoke_scene(X, steps=8, seed=6):
    """the smoke_state scenes of tests/test_gpu_render.py: a few oracle steps + a noise blob"""
    s = orc.Sim(X, X, X, iters=20)
    for _ in range(steps):
        s.step()
    col = s.color.copy()
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(X),) * 3, indexing="ij")
    blob = np.exp(-(((x - X * .55) ** 2 + (y - X * .5) ** 2 + (z - X * .45) ** 2) / (X * .22) ** 2)).astype(f32)
    col += (blob[..., None] * rng.random((X, X, X, 4)) * np.array([.3, .5, .8, .6])).astype(f32)
    return np.clip(col, 0, 1).astype(f32)


def world_view_proj_rows(view, proj):
    """CBPerObject.WorldViewProj (Fluid.cpp:315-318: world = scale 10) as its four constant-buffer rows"""
    wvp = np.diag([10.0, 10.0, 10.0, 1.0]) @ np.asarray(view, np.float64).reshape(4, 4) @ np.asarray(proj, np.float64).reshape(4, 4)
    return np.ascontiguousarray(wvp.T, f32)


def analytic_depth(proj, W, H, plane=None, sphere=None):
    """D3D depth of a view-space scene: plane = (a, b, c): z = c + a x + b y; sphere = (cx, cy, cz, r).  1.0 where nothing is hit."""
    P = np.asarray(proj, np.float64).reshape(4, 4)
    px, py = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H)
    dx, dy = (px * 2 - 1) / P[0, 0], (1 - py * 2) / P[1, 1]           # view-space ray (dx, dy, 1) through the pixel centre
    zv = np.full((H, W), np.inf)
    if plane is not None:
        a, b, c = plane
        den = 1 - a * dx - b * dy
        t = np.where(den > 0, c / np.where(den > 0, den, 1), np.inf)
        zv = np.minimum(zv, np.where(t > 0, t, np.inf))
    if sphere is not None:
        cx, cy, cz, r = sphere
        dd = dx * dx + dy * dy + 1
        bq = dx * cx + dy * cy + cz
        disc = bq * bq - dd * (cx * cx + cy * cy + cz * cz - r * r)
        t = (bq - np.sqrt(np.maximum(disc, 0))) / dd
        zv = np.minimum(zv, np.where((disc > 0) & (t > 0), t, np.inf))
    z = np.where(np.isfinite(zv), P[2, 2] + P[3, 2] / np.where(np.isfinite(zv), zv, 1), 1.0)
    return np.clip(z, 0, 1).astype(f32)


def scene(X=32, vp=(160, 120), max_samples=(48, 16), sh=False):
    col = smoke_scene(X)
    view, proj, eye = orc.default_camera(*vp)
    fr, lod, rs, mask, _ = orc.update_frame(view, proj, eye, vp[0], vp[1], X, max_samples[0])
    shc = (np.random.default_rng(4).random((9, 3)) * np.array([[2.0]] + [[0.5]] * 8)).astype(f32) if sh else None
    if sh:
        for i, v in enumerate(shc.reshape(27)):
            fr.sh[i] = v
    wvp_i = orc.world_view_proj_inverse(view, proj)
    return col, view, proj, eye, fr, lod, rs, mask, wvp_i, shc


# ---- 1: the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_abi_offers_scene_depth():
    from fluidx12_amd import capi
    import fluidx12_amd as fx
    src = open(os.path.join(ROOT, "include", "fluidx_hip.h")).read()
    assert re.search(r"\bint\s+fx_set_scene_depth\s*\(", src)
    assert int(re.search(r"FX_FIELD_CUBE_DEPTH\s*=\s*(\d+)", src).group(1)) == capi.FIELD_CUBE_DEPTH == fx.FIELD_CUBE_DEPTH == 10
    assert int(re.search(r"#define\s+FX_DEPTH_DEVICE\s+0x([0-9a-fA-F]+)u", src).group(1), 16) == capi.DEPTH_DEVICE == 1
    assert int(re.search(r"#define\s+FX_ABI_VERSION\s+(\d+)", src).group(1)) == capi.ABI_VERSION == 7
    assert "fx_set_scene_depth" in capi.SYMBOLS
    lib = capi.load()
    assert hasattr(lib, "fx_set_scene_depth") and lib.fx_abi_version() == 7
    assert lib.fx_set_scene_depth(None, None, None, 0, 0, 1.0, 1000.0, 0) == capi.FX_E_INVALID
    assert callable(getattr(fx.Fluid, "SetSceneDepth"))
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    assert "bool SetSceneDepth(const float* depth, float zNear, float zFar, bool onDevice = false)" in hpp


def test_the_depth_reference_includes_nothing_of_the_product():
    for s in _SRCS:
        txt = open(s).read()
        assert "fluidx12_amd" not in txt and "fluidx_hip.h" not in txt and "fx_march" not in txt


# ---- 2: the anchor: a far-plane depth buffer reproduces the oracle byte for byte ------------------------------------------------------
@pytest.mark.parametrize("separate,sh", [(True, False), (False, False), (False, True)])
def test_far_plane_depth_reproduces_the_oracle_direct_march(dref, separate, sh):
    col, view, proj, eye, fr, lod, rs, mask, wvp_i, shc = scene(sh=sh)
    W, H = 160, 120
    lm = orc.raymarch_light(col, fr, 16, sh, 2) if separate else None
    ns = rs if separate else 48
    out, cov = orc.raycast_direct(col, lm, fr, wvp_i, W, H, ns, 16, sh, separate)
    got, gcov = ref_direct(col, lm, fr, wvp_i, W, H, ns, 16, sh, separate, np.ones((H, W), f32))
    assert 0.05 < cov.mean() < 0.9
    assert np.array_equal(gcov, cov) and np.array_equal(got.view(np.uint32), out.view(np.uint32))


@pytest.mark.parametrize("separate", [True, False])
def test_far_plane_depth_reproduces_the_oracle_cube_march_and_resolve(dref, separate):
    col, view, proj, eye, fr, lod, rs, mask, wvp_i, _ = scene()
    W, H = 160, 120
    X = col.shape[0]
    lm = orc.raymarch_light(col, fr, 16, False, 2) if separate else None
    cf, cu = orc.raymarch_view(col, lm, fr, X >> lod, mask, rs, 16, False, separate)
    depth = np.ones((H, W), f32)
    gf, gu, gd = ref_view(col, lm, fr, X >> lod, mask, rs, 16, False, separate, depth, world_view_proj_rows(view, proj), wvp_i)
    assert cu[..., 3].max() > 50
    assert np.array_equal(gf.view(np.uint32), cf.view(np.uint32)) and np.array_equal(gu, cu)
    assert np.all(gd == 1.0)
    out, cov = orc.resolve_cube(cu, fr, wvp_i, W, H)
    got, gcov = ref_resolve(gu, gd, fr, wvp_i, depth)
    assert cov.mean() > 0.05
    assert np.array_equal(gcov, cov) and np.array_equal(got.view(np.uint32), out.view(np.uint32))


# ---- 3: the toy case: depth in front of the volume = the first sample only ------------------------------------------------------------
@pytest.mark.parametrize("separate", [True, False])
def test_depth_in_front_of_the_volume_leaves_one_sample(dref, separate):
    col, view, proj, eye, fr, lod, rs, mask, wvp_i, _ = scene()
    W, H = 160, 120
    X = col.shape[0]
    lm = orc.raymarch_light(col, fr, 16, False, 2) if separate else None
    near = np.zeros((H, W), f32)
    ns = rs if separate else 48
    one, cov1 = orc.raycast_direct(col, lm, fr, wvp_i, W, H, 1, 16, False, separate)
    got, gcov = ref_direct(col, lm, fr, wvp_i, W, H, ns, 16, False, separate, near)
    full, _ = orc.raycast_direct(col, lm, fr, wvp_i, W, H, ns, 16, False, separate)
    assert np.array_equal(gcov, cov1) and np.array_equal(got.view(np.uint32), one.view(np.uint32))
    assert full[..., 3].sum() > 2 * got[..., 3].sum()                  # (and the occlusion does take most of the smoke away)
    cf1, cu1 = orc.raymarch_view(col, lm, fr, X >> lod, mask, 1, 16, False, separate)
    gf, gu, gd = ref_view(col, lm, fr, X >> lod, mask, rs, 16, False, separate, near, world_view_proj_rows(view, proj), wvp_i)
    assert np.array_equal(gf.view(np.uint32), cf1.view(np.uint32))
    ray = np.zeros(gd.shape, bool)
    ray[[f for f in range(6) if mask >> f & 1]] = True
    assert np.all(gd[ray] == 0.0) and np.all(gd[~ray] == 1.0)


def test_depth_reference_occludes_behind_a_plane(dref):
    """a plane through the volume: rays whose scene point lies behind the grid are untouched, rays that meet it inside see less"""
    col, view, proj, eye, fr, lod, rs, mask, wvp_i, _ = scene()
    W, H = 160, 120
    dist = float(np.linalg.norm(eye))
    out, cov = orc.raycast_direct(col, None, fr, wvp_i, W, H, 48, 16, False, False)
    far = analytic_depth(proj, W, H, plane=(0.0, 0.0, dist + 30.0))
    mid = analytic_depth(proj, W, H, plane=(0.3, 0.2, dist))
    g_far, _ = ref_direct(col, None, fr, wvp_i, W, H, 48, 16, False, False, far)
    g_mid, _ = ref_direct(col, None, fr, wvp_i, W, H, 48, 16, False, False, mid)
    assert np.array_equal(g_far.view(np.uint32), out.view(np.uint32))
    assert np.all(g_mid[..., 3] <= out[..., 3]) and g_mid[..., 3].sum() < 0.9 * out[..., 3].sum()
