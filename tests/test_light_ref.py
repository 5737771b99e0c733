"""The settable scene light (fx_set_light, the reference's _POINT_LIGHT_ variants), CPU side: the C ABI surface, and the CPU reference of
tests/light_ref/ -- anchored to the oracle (a directional light changes no byte), checked on a toy scene that proves the per-voxel
direction and that a ray to a point light ends at the light, and on a light that sits exactly on a voxel's centre."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc
from test_depth_ref import scene, smoke_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_u8 = C.POINTER(C.c_uint8)
DIRECTIONAL, POINT = 0, 1
PI = f32(3.141592654)
DEFAULT_LIGHT = ((75.0, 75.0, -75.0), (1.0, 0.7, 0.3, float(PI * f32(3.0))), (1.0, 1.0, 1.0, float(PI * f32(1.5))))   # Fluid.cpp:169-173


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- the reference: built from tests/light_ref/ + the oracle's other sources with the oracle's flags -----------------------------------
_SRCS = [os.path.join(ROOT, "tests", "light_ref", "orc_point_light.cpp")]
_ORACLE = [os.path.join(ROOT, "oracle", s) for s in ("orc_sim.cpp", "orc_host.cpp", "orc_sh.cpp", "orc_bc6h.cpp", "orc_render.cpp",
                                                      "orc_resolve.cpp", "orc_common.h", "fx_oracle.h")]
_LIB = None


def light_ref_lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "_build", "liborclight.so")
        deps = _SRCS + _ORACLE
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = ["-O3", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2"]   # oracle/Makefile
            subprocess.run(["g++"] + flags + ["-shared", "-o", out] + _SRCS + [p for p in _ORACLE if p.endswith(".cpp") and
                           not p.endswith("orc_render.cpp")] + ["-lm"], check=True)
        _LIB = C.CDLL(out)
        _LIB.orcl_zero_vectors.restype = C.c_longlong
    return _LIB


@pytest.fixture(scope="module")
def lref():
    return light_ref_lib()


def set_light(fr, position, color=None, ambient=None):
    """fills orc_frame.light_pt / light_color / ambient (the oracle has always taken them as inputs)"""
    for i, v in enumerate(position):
        fr.light_pt[i] = v
    for i, v in enumerate(color if color is not None else DEFAULT_LIGHT[1]):
        fr.light_color[i] = v
    for i, v in enumerate(ambient if ambient is not None else DEFAULT_LIGHT[2]):
        fr.ambient[i] = v
    return fr


def ref_light(col, fr, nl, sh, fmt, kind):
    col = np.ascontiguousarray(col, f32)
    Z, Y, X, _ = col.shape
    lm = np.empty((Z, Y, X, 3), f32)
    light_ref_lib().orcl_raymarch_light(_fp(col), _fp(lm), X, Y, Z, C.byref(fr), nl, int(sh), fmt, kind)
    return lm


def ref_view(col, lm, fr, size, mask, ns, nl, sh, separate, kind):
    col = np.ascontiguousarray(col, f32)
    Z, Y, X, _ = col.shape
    cf = np.zeros((6, size, size, 4), f32)
    cu = np.zeros((6, size, size, 4), np.uint8)
    lmp = _fp(np.ascontiguousarray(lm, f32)) if lm is not None else None
    light_ref_lib().orcl_raymarch_view(_fp(col), lmp, X, Y, Z, C.byref(fr), size, mask, ns, nl, int(sh), int(separate), kind,
                                       _fp(cf), cu.ctypes.data_as(_u8))
    return cf, cu


def ref_direct(col, lm, fr, wvp_i, W, H, ns, nl, sh, separate, kind):
    col = np.ascontiguousarray(col, f32)
    Z, Y, X, _ = col.shape
    out = np.empty((H, W, 4), f32)
    cov = np.empty((H, W), np.uint8)
    lmp = _fp(np.ascontiguousarray(lm, f32)) if lm is not None else None
    light_ref_lib().orcl_raycast_direct(_fp(col), lmp, X, Y, Z, C.byref(fr), _fp(np.ascontiguousarray(wvp_i, f32)), W, H, ns, nl, int(sh),
                                        int(separate), kind, _fp(out), cov.ctypes.data_as(_u8))
    return out, cov


# ---- the toy scene: a wall between the two halves of the volume ----------------------------------------------------------------------------
TOY_X, TOY_NL = 32, 64


def voxel_centres(X):
    return ((np.arange(X, dtype=f32) + f32(0.5)) / f32(X) * f32(2.0) - f32(1.0)).astype(f32)      # CSRayMarchL.hlsl:22


def toy_scene(X=TOY_X):
    """a wall |x_local| < 0.2 of alpha 1 (the step factor is then 1 and every sample multiplies the transmittance by 0.2) in smoke of alpha
    0.02 (every voxel is lit: >= 0.01); all colour channels 1"""
    col = np.ones((X, X, X, 4), f32)
    col[..., 3] = 0.02
    col[:, :, np.abs(voxel_centres(X)) < 0.2, 3] = 1.0
    return col


def toy_frame(position, color=(1.0, 1.0, 1.0, 1.0), ambient=(0.0, 0.0, 0.0, 0.0), vp=(160, 120), X=TOY_X):
    """light colour 1, no ambient: the red light-map value of a voxel IS its shadow term"""
    view, proj, eye = orc.default_camera(*vp)
    fr = orc.update_frame(view, proj, eye, vp[0], vp[1], X, 48)[0]
    return set_light(fr, position, color, ambient)


def toy_sides(X=TOY_X, light_x=0.6):
    """(bright, dark, beyond): voxels right of the wall, left of it, and right of the light -- without the ones within two cells of
    the wall's faces and of the plane through the light"""
    c = voxel_centres(X).astype(np.float64)
    cell = 2.0 / X
    keep = (np.abs(np.abs(c) - 0.2) > 2 * cell) & (np.abs(c - light_x) > 2 * cell)
    x = np.broadcast_to(c, (X, X, X))
    k = np.broadcast_to(keep, (X, X, X))
    return k & (x > 0.2), k & (x < -0.2), k & (x > light_x)


# ---- 1: the anchor: kind = directional reproduces the oracle byte for byte -------------------------------------------------------------------
OTHER_LIGHT = ((-30.0, -55.0, 40.0), (0.4, 0.9, 1.0, 5.5), (0.2, 0.5, 0.3, 2.25))      # below and behind the volume


@pytest.mark.parametrize("light", [DEFAULT_LIGHT, OTHER_LIGHT], ids=["default", "other"])
@pytest.mark.parametrize("sh", [False, True])
def test_a_directional_light_reproduces_the_oracle(lref, light, sh):
    col, view, proj, eye, fr, lod, rs, mask, wvp_i, shc = scene(sh=sh)
    set_light(fr, *light)
    X = col.shape[0]
    W, H = 160, 120
    for fmt in (0, 2):
        assert np.array_equal(ref_light(col, fr, 16, sh, fmt, DIRECTIONAL).view(np.uint32), orc.raymarch_light(col, fr, 16, sh, fmt).view(np.uint32))
    lm = orc.raymarch_light(col, fr, 16, sh, 2)
    for separate in (False, True):
        cf, cu = orc.raymarch_view(col, lm if separate else None, fr, X >> lod, mask, rs, 16, sh, separate)
        gf, gu = ref_view(col, lm if separate else None, fr, X >> lod, mask, rs, 16, sh, separate, DIRECTIONAL)
        assert cu[..., 3].max() > 50
        assert np.array_equal(gf.view(np.uint32), cf.view(np.uint32)) and np.array_equal(gu, cu)
    out, cov = orc.raycast_direct(col, None, fr, wvp_i, W, H, 48, 16, sh, False)
    got, gcov = ref_direct(col, None, fr, wvp_i, W, H, 48, 16, sh, False, DIRECTIONAL)
    assert 0.05 < cov.mean() < 0.9
    assert np.array_equal(gcov, cov) and np.array_equal(got.view(np.uint32), out.view(np.uint32))
    if light is OTHER_LIGHT and not sh:                               # ... and the other light is another picture
        base = orc.raycast_direct(col, None, set_light(fr, *DEFAULT_LIGHT), wvp_i, W, H, 48, 16, sh, False)[0]
        assert not np.array_equal(base, out)


def test_the_light_reference_includes_nothing_of_the_product():
    for s in _SRCS:
        txt = open(s).read()
        assert "fluidx12_amd" not in txt and "fluidx_hip.h" not in txt and "fx_march" not in txt


# ---- 2: the toy scene: the direction is per voxel, and the ray ends at the light --------------------------------------------------------------
def test_a_point_light_lights_its_side_of_a_wall(lref):
    """light at local (0.6, 0, 0): every voxel right of the wall sees it (at least 0.984^64 = 0.36 of it through the thin smoke), every
    voxel left of the wall sits in the wall's shadow (below 0.01) -- an ordering, not a threshold.  The voxels right of the LIGHT are on
    the bright side only because their ray ends at the light (addition A): with the rule off -- the compiled-out variant as written -- the
    ray goes on through the light into the wall.  (That holds for the voxels whose line through the light meets the whole wall inside the
    volume, which is what the second half asserts; the line of a voxel far off the axis leaves the volume before it gets there.)"""
    col = toy_scene()
    fr = toy_frame((6.0, 0.0, 0.0))
    bright, dark, beyond = toy_sides()
    assert bright.sum() > 5000 and dark.sum() > 5000 and beyond.sum() > 2000
    lm = ref_light(col, fr, TOY_NL, False, 0, POINT)[..., 0]
    print("bright side min %.4f, dark side max %.5f" % (lm[bright].min(), lm[dark].max()))
    assert lm[bright].min() > lm[dark].max()
    assert lm[bright].min() >= 0.984 ** 64 * 0.99 and lm[dark].max() < 0.01
    c = voxel_centres(TOY_X).astype(np.float64)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    s = (x + 0.2) / (x - 0.6)                                       # parameter at which the line voxel -> light reaches the wall's far face
    through = beyond & (np.abs(y * (1 - s)) < 1) & (np.abs(z * (1 - s)) < 1)
    assert through.sum() > 100
    lref.orcl_set_end_rule(0)
    try:
        off = ref_light(col, fr, TOY_NL, False, 0, POINT)[..., 0]
    finally:
        lref.orcl_set_end_rule(1)
    print("beyond the light, rule on: min %.4f; rule off: max %.5f over %d voxels" % (lm[through].min(), off[through].max(), through.sum()))
    assert off[through].max() < 0.01 and off[through].max() < lm[bright].min()
    assert np.all(off <= lm)                                         # (a ray that goes on can only lose light: no voxel gains by the rule being off) ...
    rest = beyond & ~through                                         # their line leaves the volume before it has crossed the wall:
    assert off[rest].max() > 0.01                                    # not all of them can be dark, which is why `through` is what is asserted
    assert np.array_equal(ref_light(col, fr, TOY_NL, False, 0, POINT)[..., 0], lm)   # ... and the switch is back on


# ---- 3: addition B: the light on a voxel's centre ---------------------------------------------------------------------------------------------
COINCIDENT_VOXEL = (15, 15, 15)


def coincident_light(fr=None):
    """world position of voxel 15's centre of 32 (local -0.03125 per axis): its product with the world's 0.1 scale is exact"""
    w = (-0.3125,) * 3
    if fr is not None:
        assert all(f32(w[a]) * f32(fr.world_i[5 * a]) == voxel_centres(32)[15] for a in range(3))
    return w


def test_a_light_on_a_voxel_centre_casts_no_ray_there(lref):
    col = toy_scene()
    fr = toy_frame((0.0, 0.0, 0.0), color=(1.0, 0.5, 0.25, 2.0), ambient=(0.5, 0.5, 0.5, 0.25))
    set_light(fr, coincident_light(fr), (1.0, 0.5, 0.25, 2.0), (0.5, 0.5, 0.5, 0.25))
    x, y, z = COINCIDENT_VOXEL
    for fmt in (0, 2):
        lref.orcl_reset_zero_vectors()
        lm = ref_light(col, fr, TOY_NL, False, fmt, POINT)
        assert lref.orcl_zero_vectors() >= 1
        assert np.isfinite(lm).all()
        unlit = ref_light(np.zeros_like(col), fr, TOY_NL, False, fmt, POINT)[0, 0, 0]      # shadow = 1: light colour + ambient
        assert np.array_equal(lm[z, y, x], unlit)
        assert np.array_equal(unlit, np.array([2.125, 1.125, 0.625], f32))
        assert lm[z, y, x + 1, 0] < unlit[0] and lm[z, y + 1, x, 0] < unlit[0]              # its neighbours look through the wall's smoke
    # the merged marches meet no such sample here, and stay finite
    view, proj, eye = orc.default_camera(160, 120)
    wvp_i = orc.world_view_proj_inverse(view, proj)
    out, cov = ref_direct(col, None, fr, wvp_i, 160, 120, 48, 16, False, False, POINT)
    assert np.isfinite(out).all() and cov.mean() > 0.05


# ---- 4: the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_abi_offers_the_scene_light(tmp_path):
    from fluidx12_amd import capi
    import fluidx12_amd as fx
    src = open(os.path.join(ROOT, "include", "fluidx_hip.h")).read()
    assert re.search(r"\bint\s+fx_set_light\s*\(\s*fx_ctx\s*\*\s*ctx\s*,\s*const\s+fx_light\s*\*\s*light\s*\)", src)
    assert re.search(r"\bint\s+fx_get_light\s*\(\s*fx_ctx\s*\*\s*ctx\s*,\s*fx_light\s*\*\s*out\s*\)", src)
    assert int(re.search(r"#define\s+FX_LIGHT_DIRECTIONAL\s+(\d+)u", src).group(1)) == capi.LIGHT_DIRECTIONAL == 0
    assert int(re.search(r"#define\s+FX_LIGHT_POINT\s+(\d+)u", src).group(1)) == capi.LIGHT_POINT == 1
    assert int(re.search(r"#define\s+FX_ABI_VERSION\s+(\d+)", src).group(1)) == capi.ABI_VERSION == 7
    assert "fx_set_light" in capi.SYMBOLS and "fx_get_light" in capi.SYMBOLS
    # the struct as a C compiler lays it out
    prog = tmp_path / "light_size.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidx_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu", sizeof(fx_light), '
                    'offsetof(fx_light, kind), offsetof(fx_light, position), offsetof(fx_light, color), offsetof(fx_light, ambient)); return 0; }\n')
    exe = tmp_path / "light_size"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    L = capi.Light
    assert sizes == [C.sizeof(L), L.kind.offset, L.position.offset, L.color.offset, L.ambient.offset] == [52, 4, 8, 20, 36]
    lib = capi.load()
    assert hasattr(lib, "fx_set_light") and hasattr(lib, "fx_get_light") and lib.fx_abi_version() == 7
    assert lib.fx_set_light(None, None) == capi.FX_E_INVALID and lib.fx_get_light(None, None) == capi.FX_E_INVALID
    assert callable(getattr(fx.Fluid, "SetLight")) and callable(getattr(fx.Fluid, "GetLight"))
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    assert "bool SetLight(const fx_light* light)" in hpp and "bool GetLight(fx_light* out)" in hpp
