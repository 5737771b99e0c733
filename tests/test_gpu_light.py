"""The settable scene light on the MI355X (fx_set_light; FX_LIGHT_POINT = the reference's _POINT_LIGHT_ variants): the default light changes
no bit, directional lights equal the pinned oracle, point lights equal the CPU reference of tests/light_ref/, the accelerated kernels
equal the plain ones with a point light, the light is state that survives what it should, and bad arguments are refused without harm."""
import ctypes as C
import functools

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi
from oracle import orc
from test_depth_ref import analytic_depth, smoke_scene
from test_light_ref import (COINCIDENT_VOXEL, DEFAULT_LIGHT, DIRECTIONAL, OTHER_LIGHT, POINT, TOY_NL, coincident_light, ref_direct, ref_light,
                            ref_view, set_light, toy_scene, toy_sides)

pytestmark = pytest.mark.gpu
f32 = np.float32
VP = (200, 150)
FLAGS = (fx.Fluid.RAY_MARCH_DIRECT, fx.Fluid.RAY_MARCH_CUBEMAP, fx.Fluid.SEPARATE_LIGHT_PASS, fx.Fluid.OPTIMIZED)
# below and behind the volume / above, in front, nearly level
DIRECTIONAL_LIGHTS = (OTHER_LIGHT, ((20.0, 3.0, -60.0), (1.0, 0.2, 0.6, 7.0), (0.1, 0.3, 0.9, 1.5)))
# outside the volume ([-10, 10]^3), inside the plume, on the +x face
POINT_LIGHTS = {"outside": (14.0, 18.0, -16.0), "inside": (1.0, 0.5, -1.0), "face": (10.0, 2.0, -3.0)}
POINT_COLOR, POINT_AMBIENT = (1.0, 0.8, 0.5, 6.0), (0.6, 0.7, 1.0, 0.75)


def make(X, col, vp=VP, storage="fp32", sh=None, max_samples=(48, 16), accel=1):
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], (X, X, X), storage=storage)
    f.SetMaxSamples(*max_samples)
    if sh is not None:
        f.SetSH(sh)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    view, proj, eye = fx.default_camera(*vp)
    f.upload(fx.FIELD_COLOR, col)
    f.UpdateFrame(0.0, 0, view, proj, eye)
    return f, view, proj, eye


def pictures(f, flags):
    """everything a render leaves: light map (separate pass), cube map (cube paths), target and float target"""
    f.ClearRenderTarget()
    f.Render(0, flags)
    out = {}
    if flags & fx.Fluid.SEPARATE_LIGHT_PASS:
        out["lightmap"] = f.download(fx.FIELD_LIGHTMAP)
    if flags & fx.Fluid.RAY_MARCH_CUBEMAP:
        out["cube"] = f.download(fx.FIELD_CUBEMAP)
        f.RenderCube(0)
    f.Synchronize()
    out["target"] = f.download(fx.FIELD_TARGET)
    out["target_float"] = f.download(fx.FIELD_TARGET_FLOAT)
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def finite(p):
    return all(np.isfinite(v).all() for v in p.values() if v.dtype != np.uint8)


def sh27():
    return (np.random.default_rng(4).random((9, 3)) * np.array([[2.0]] + [[0.5]] * 8)).astype(f32)


def frame_of(f, view, proj, eye, X, light, sh=None, max_samples=48):
    """the oracle's frame constants of this context, with `light` = (position, colour, ambient) filled in"""
    fr, lod, rs, mask, _ = orc.update_frame(view, proj, eye, f.viewport[0], f.viewport[1], X, max_samples)
    fi = f.frame_info()
    assert (fi.cube_lod, fi.ray_samples, fi.visibility_mask) == (lod, rs, mask)
    set_light(fr, *light)
    if sh is not None:
        for i, v in enumerate(np.asarray(sh, f32).reshape(27)):
            fr.sh[i] = v
    return fr, lod, rs, mask, np.array(list(fi.world_view_proj_i), f32).reshape(4, 4)


@functools.lru_cache(maxsize=None)
def scene_of(X):
    return smoke_scene(X)


def cube_close(gpu, ref, max_lsb=1, frac=0.02):                    # tests/test_gpu_render.py:49-52
    d = np.abs(gpu.astype(np.int32) - ref.astype(np.int32))
    print("cube: max %d LSB, share %.5f" % (int(d.max()), float((d > 0).mean())))
    assert d.max() <= max_lsb, int(d.max())
    assert (d > 0).mean() <= frac, float((d > 0).mean())


def lightmap_close(lm, ref, share):
    """test_gpu_render.py:69-70,144: rare R11G11B10 rounding flips only"""
    print("light map: share of differing texels %.6f, max error %.5f of max %.3f" % (float((lm != ref).mean()), float(np.abs(lm - ref).max()), float(np.abs(ref).max())))
    assert (lm != ref).mean() < share
    assert np.abs(lm - ref).max() <= np.abs(ref).max() * 2.0 ** -5


def against_reference(f, col, fr, lod, rs, mask, wvp_i, nl, use_sh, kind, lm_share):
    """the four render paths of `f` against the CPU reference (kind = DIRECTIONAL: byte for byte the pinned oracle, tests/test_light_ref.py)"""
    X = col.shape[0]
    W, H = f.viewport
    got = pictures(f, fx.Fluid.OPTIMIZED)
    lm_ref = ref_light(col, fr, nl, use_sh, 2, kind)
    lightmap_close(got["lightmap"], lm_ref, lm_share)
    assert np.unique(lm_ref[..., 0]).size > 20                       # (shadows of many depths: the light does reach into the smoke)
    _, cu = ref_view(col, lm_ref, fr, X >> lod, mask, rs, nl, use_sh, True, kind)
    assert cu[..., 3].max() > 50
    cube_close(got["cube"], cu)
    _, cu = ref_view(col, None, fr, X >> lod, mask, rs, nl, use_sh, False, kind)           # the merged cube march
    cube_close(pictures(f, fx.Fluid.RAY_MARCH_CUBEMAP)["cube"], cu)
    out, cov = ref_direct(col, None, fr, wvp_i, W, H, 48, nl, use_sh, False, kind)          # the merged direct march
    gf = pictures(f, fx.Fluid.RAY_MARCH_DIRECT)["target_float"]
    print("merged direct: %d of %d floats differ" % (int((gf.view(np.uint32) != out.view(np.uint32)).sum()), gf.size))
    assert cov.mean() > 0.05 and np.array_equal(gf.view(np.uint32), out.view(np.uint32))   # tests/test_gpu_depth.py:107
    out, _ = ref_direct(col, lm_ref, fr, wvp_i, W, H, rs, nl, use_sh, True, kind)          # the separate direct march
    gf = pictures(f, fx.Fluid.SEPARATE_LIGHT_PASS)["target_float"]
    print("separate direct: share %.6f, max %.5f" % (float(np.mean(gf != out)), float(np.abs(gf - out).max())))
    assert np.mean(gf != out) < 2e-3 and np.abs(gf - out).max() < 0.05                     # tests/test_gpu_depth.py:105


# ---- 5: the default light changes nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,use_sh,accel", [("fp32", False, 1), ("fp32", True, 1), ("fp16", False, 1), ("fp16", True, 0), ("fp32", False, 0)])
def test_the_default_light_changes_no_bit(storage, use_sh, accel):
    X = 32
    f, view, proj, eye = make(X, scene_of(X), storage=storage, sh=sh27() if use_sh else None, accel=accel)
    got = f.GetLight()
    assert got["kind"] == "directional"
    assert np.array_equal(np.array(got["position"], f32), np.array(DEFAULT_LIGHT[0], f32))
    assert np.array_equal(np.array(got["color"], f32), np.array(DEFAULT_LIGHT[1], f32))
    assert np.array_equal(np.array(got["ambient"], f32), np.array(DEFAULT_LIGHT[2], f32))
    for flags in FLAGS:
        base = pictures(f, flags)                                    # a context that never called the setter
        f.SetLight(DEFAULT_LIGHT[0], "directional", DEFAULT_LIGHT[1], DEFAULT_LIGHT[2])
        same(pictures(f, flags), base)
        f.SetLight(POINT_LIGHTS["inside"], "point", POINT_COLOR, POINT_AMBIENT)
        other = pictures(f, flags)
        assert not np.array_equal(other["target"], base["target"])
        f.SetLight(None)
        same(pictures(f, flags), base)
    f.Release()


# ---- 6: directional light, colour, ambient against the pinned oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("which,X,use_sh", [(0, 32, False), (1, 40, False), (0, 40, True), (1, 32, True)])
def test_a_directional_light_equals_the_oracle(which, X, use_sh):
    col = scene_of(X)
    sh = sh27() if use_sh else None
    light = DIRECTIONAL_LIGHTS[which]
    f, view, proj, eye = make(X, col, sh=sh)
    f.SetLight(light[0], "directional", light[1], light[2])
    before = pictures(f, fx.Fluid.OPTIMIZED)
    f.UpdateFrame(0.0, 0, view, proj, eye)                          # the light is kept across UpdateFrame
    got = f.GetLight()
    assert got["kind"] == "directional" and np.array_equal(np.array(got["position"] + got["color"] + got["ambient"], f32), np.array(sum(light, ()), f32))
    same(pictures(f, fx.Fluid.OPTIMIZED), before)
    fr, lod, rs, mask, wvp_i = frame_of(f, view, proj, eye, X, light, sh)
    # orc.* with these frame constants, through the reference that equals it byte for byte for a directional light
    assert np.array_equal(ref_light(col, fr, 16, use_sh, 2, DIRECTIONAL), orc.raymarch_light(col, fr, 16, use_sh, 2))
    against_reference(f, col, fr, lod, rs, mask, wvp_i, 16, use_sh, DIRECTIONAL, 5e-3 if use_sh else 1e-3)
    f.Release()


# ---- 7: point lights against tests/light_ref/ ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_sh", [False, True])
@pytest.mark.parametrize("X", [32, 40])
@pytest.mark.parametrize("where", ["outside", "inside", "face"])
def test_a_point_light_equals_the_reference(where, X, use_sh):
    col = scene_of(X)
    sh = sh27() if use_sh else None
    light = (POINT_LIGHTS[where], POINT_COLOR, POINT_AMBIENT)
    f, view, proj, eye = make(X, col, sh=sh)
    f.SetLight(light[0], "point", light[1], light[2])
    fr, lod, rs, mask, wvp_i = frame_of(f, view, proj, eye, X, light, sh)
    # (the point light normalises per voxel, as the GI ray does: the GI path's share of rounding flips)
    against_reference(f, col, fr, lod, rs, mask, wvp_i, 16, use_sh, POINT, 5e-3)
    f.Release()


def toy_context(position, color, ambient):
    col = toy_scene()
    f, view, proj, eye = make(32, col, max_samples=(48, TOY_NL))
    f.SetLight(position, "point", color, ambient)
    fr = frame_of(f, view, proj, eye, 32, (position, color, ambient))[0]
    return f, col, fr


@pytest.mark.parametrize("accel", [1, 0])
def test_a_point_light_lights_its_side_of_a_wall(accel):
    """tests/test_light_ref.py's toy: everything right of the wall -- right of the light too, whose rays end at the light -- is brighter
    than everything left of it"""
    f, col, fr = toy_context((6.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0))
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    lm = pictures(f, fx.Fluid.OPTIMIZED)["lightmap"]
    bright, dark, beyond = toy_sides()
    red = lm[..., 0]
    print("bright side min %.4f (beyond the light %.4f), dark side max %.5f" % (red[bright].min(), red[beyond].min(), red[dark].max()))
    assert red[bright].min() > red[dark].max()
    assert red[bright].min() >= 0.984 ** 64 * 0.99 and red[dark].max() < 0.01 * (1 + 2.0 ** -6)      # (R11G11B10: 6 bits of mantissa)
    lightmap_close(lm, ref_light(col, fr, TOY_NL, False, 2, POINT), 5e-3)
    f.Release()


@pytest.mark.parametrize("accel", [1, 0])
def test_a_light_on_a_voxel_centre_casts_no_ray_there(accel):
    color, ambient = (1.0, 0.5, 0.25, 2.0), (0.5, 0.5, 0.5, 0.25)
    f, col, fr = toy_context(coincident_light(), color, ambient)
    coincident_light(fr)                                             # (the product with the world's scale is exact)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    x, y, z = COINCIDENT_VOXEL
    for flags in FLAGS:
        p = pictures(f, flags)
        assert finite(p)
        if "lightmap" in p:
            lm = p["lightmap"]
            assert np.array_equal(lm[z, y, x], np.array([2.125, 1.125, 0.625], f32))       # shadow = 1: light colour + ambient
            assert lm[z, y, x + 1, 0] < 2.125 and lm[z, y + 1, x, 0] < 2.125
            lightmap_close(lm, ref_light(col, fr, TOY_NL, False, 2, POINT), 5e-3)
    f.Release()


# ---- 8: accelerated = plain, bit for bit, with a point light -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparse_noise(X):
    return np.clip(np.random.default_rng(1).random((X, X, X, 4), f32) ** 8, 0, 1)


@pytest.mark.parametrize("X,use_sh", [(32, False), (32, True), (40, False), (40, True), (288, False), (288, True)])
def test_accelerated_equals_plain_with_a_point_light(X, use_sh):
    """light map, cube map and the direct float target; 288^3 holds a coarser mask level in the LDS (AccelVol<.., COARSE>) and takes the
    three-pass light volume; with the light probe the shadow ray's transmittance is parked for the occlusion pass (RAYS_SHADOW_KEEP ->
    RAYS_AO); a scene depth is attached throughout"""
    vp = (160, 120)
    col = scene_of(X) if X <= 64 else sparse_noise(X)
    f, view, proj, eye = make(X, col, vp=vp, sh=sh27() if use_sh else None, max_samples=(96, 24) if X <= 64 else (96, 16))
    f.SetLight(POINT_LIGHTS["inside"], "point", POINT_COLOR, POINT_AMBIENT)
    dist = float(np.linalg.norm(eye))
    f.SetSceneDepth(analytic_depth(proj, vp[0], vp[1], plane=(0.8, 0.2, dist), sphere=(2.0, -1.0, dist - 9.0, 4.0)))
    for flags in FLAGS:
        f.set_option(capi.OPT_RENDER_ACCEL, 1)
        a = pictures(f, flags)
        f.set_option(capi.OPT_RENDER_ACCEL, 0)
        b = pictures(f, flags)
        same(a, b)
        assert finite(a) and a["target_float"][..., 3].max() > 0.05
    f.Release()


# ---- 9: state and errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["1", "0"])
def test_a_change_of_colour_or_ambient_reaches_the_filled_light_map(fill, knob):
    """the accelerated filling pass rewrites the unlit constant only where a cell held a lit voxel while light colour, ambient and light
    probe are what they were (fx_api.cpp lightmap_key): changing only the colour, then only the ambient, between two renders must give
    what a fresh context with that light gives.  The filling pass serves a power-of-two grid whose side volume the advection wrote (a
    context that renders the frames it simulates) while the launcher switch LIGHT_FILL is 1, its default; the pictures cannot show which
    path ran (they are the same bit for bit), so the test runs under both settings of the switch: 1 is the filling pass where its
    conditions hold, 0 the three-pass light volume on the same context -- as tests/test_gpu_render.py alternates them."""
    knob("LIGHT_FILL", fill)
    X = 32
    f = fx.Fluid()
    assert f.Init(VP[0], VP[1], (X, X, X))
    f.SetMaxSamples(48, 16)
    view, proj, eye = fx.default_camera(*VP)
    for k in range(8):
        f.UpdateFrame(f32(f.default_time_step()), k % 3, view, proj, eye)
        f.Simulate(k % 3)
        if k == 6:
            f.Render(k % 3, fx.Fluid.OPTIMIZED)
    f.UpdateFrame(0.0, 0, view, proj, eye)
    f.Synchronize()
    col = f.download(fx.FIELD_COLOR)
    assert (col[..., 3] >= 0.01).mean() > 0.001
    fresh, *_ = make(X, col)
    lights = [(POINT_LIGHTS["inside"], "point", POINT_COLOR, POINT_AMBIENT),
              (POINT_LIGHTS["inside"], "point", (0.2, 0.9, 0.4, 3.0), POINT_AMBIENT),            # only the colour
              (POINT_LIGHTS["inside"], "point", (0.2, 0.9, 0.4, 3.0), (0.9, 0.1, 0.3, 2.0)),       # only the ambient
              (DEFAULT_LIGHT[0], "directional", (0.2, 0.9, 0.4, 3.0), (0.9, 0.1, 0.3, 2.0)),       # only kind and position
              (DEFAULT_LIGHT[0], "directional", DEFAULT_LIGHT[1], DEFAULT_LIGHT[2])]
    for light in lights:
        f.SetLight(*light)
        fresh.SetLight(*light)
        for _ in range(2):                                           # the second render is the incremental one
            same(pictures(f, fx.Fluid.OPTIMIZED), pictures(fresh, fx.Fluid.OPTIMIZED))
    f.Release()
    fresh.Release()


def _light(kind=capi.LIGHT_POINT, position=(1.0, 2.0, 3.0), color=(1.0, 1.0, 1.0, 1.0), ambient=(0.5, 0.5, 0.5, 1.0), size=None):
    l = capi.Light()
    l.struct_size = C.sizeof(capi.Light) if size is None else size
    l.kind = kind
    l.position = (C.c_float * 3)(*position)
    l.color = (C.c_float * 4)(*color)
    l.ambient = (C.c_float * 4)(*ambient)
    return l


def test_light_errors_leave_the_previous_light_in_force():
    X = 32
    f, view, proj, eye = make(X, scene_of(X))
    lib, ctx = f._lib, f._ctx
    f.SetLight(POINT_LIGHTS["outside"], "point", POINT_COLOR, POINT_AMBIENT)
    before = f.GetLight()
    base = pictures(f, fx.Fluid.OPTIMIZED)
    nan, inf = float("nan"), float("inf")
    bad = [_light(size=C.sizeof(capi.Light) - 4), _light(size=0), _light(kind=2), _light(kind=0xFFFFFFFF),
           _light(position=(nan, 0, 0)), _light(position=(0, inf, 0)), _light(position=(0, 0, -inf)),
           _light(color=(1, nan, 1, 1)), _light(color=(1, 1, 1, inf)), _light(ambient=(nan, 1, 1, 1)), _light(ambient=(1, 1, inf, 1)),
           _light(color=(-0.5, 1, 1, 1)), _light(color=(1, 1, 1, -1)), _light(ambient=(1, -1e-3, 1, 1)), _light(ambient=(1, 1, 1, -2)),
           _light(kind=capi.LIGHT_DIRECTIONAL, position=(0.0, 0.0, 0.0)), _light(kind=capi.LIGHT_DIRECTIONAL, position=(0.0, -0.0, 0.0))]
    for l in bad:
        assert lib.fx_set_light(ctx, C.byref(l)) == capi.FX_E_INVALID
        assert f.GetLight() == before
    assert lib.fx_set_light(None, C.byref(_light())) == capi.FX_E_INVALID
    assert lib.fx_get_light(ctx, None) == capi.FX_E_INVALID
    same(pictures(f, fx.Fluid.OPTIMIZED), base)
    assert lib.fx_set_light(ctx, C.byref(_light(position=(0.0, 0.0, 0.0)))) == capi.FX_OK     # a point light may sit at the origin
    assert lib.fx_set_light(ctx, C.byref(_light(color=(0, 0, 0, 0), ambient=(0, 0, 0, 0)))) == capi.FX_OK   # ... and zero is not negative
    assert finite(pictures(f, fx.Fluid.OPTIMIZED))
    f.Release()
    g2 = fx.Fluid()
    assert g2.Init(64, 64, (32, 32, 1))                               # 2-D grid
    assert g2._lib.fx_set_light(g2._ctx, C.byref(_light())) == capi.FX_E_INVALID and g2._lib.fx_set_light(g2._ctx, None) == capi.FX_E_INVALID
    g2.Release()
    sl = fx.Fluid()
    assert sl.Init(0, 0, (X, X, X), slab=(0, 12), halo_advect=6, halo_jacobi=2)                # slab context
    assert sl._lib.fx_set_light(sl._ctx, C.byref(_light())) == capi.FX_E_INVALID
    sl.Release()


def test_gathered_render_only_context_is_lit_like_the_single_domain():
    X, vp = 32, VP
    col = scene_of(X)
    view, proj, eye = fx.default_camera(*vp)
    single, *_ = make(X, col)
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (X, X, X), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        r.upload(fx.FIELD_COLOR, col[z0:z0 + nz])
        ranks.append(r)
    fx.comm_init_local(ranks)
    full = fx.Fluid()
    assert full.Init(vp[0], vp[1], (X, X, X), render_only=True)
    full.SetMaxSamples(48, 16)
    full.SetLight(POINT_LIGHTS["inside"], "point", POINT_COLOR, POINT_AMBIENT)                  # before the first UpdateFrame: kept
    single.SetLight(POINT_LIGHTS["inside"], "point", POINT_COLOR, POINT_AMBIENT)
    ranks[0].gather_color(full, root=0)
    full.UpdateFrame(0.0, 0, view, proj, eye)
    for flags in FLAGS:
        same(pictures(full, flags), pictures(single, flags))
    for o in [full, single] + ranks:
        o.Release()


def test_a_checkpoint_does_not_store_the_light(tmp_path):
    X = 32
    a, view, proj, eye = make(X, scene_of(X))
    a.SetLight(POINT_LIGHTS["face"], "point", POINT_COLOR, POINT_AMBIENT)
    lit = a.GetLight()
    path = str(tmp_path / "state.fxc")
    a.SaveCheckpoint(path)
    b, *_ = make(X, np.zeros((X, X, X, 4), f32))
    default = b.GetLight()
    b.LoadCheckpoint(path)
    assert b.GetLight() == default and default["kind"] == "directional"
    b.SetLight(None)
    a.LoadCheckpoint(path)
    assert a.GetLight() == lit
    b.UpdateFrame(0.0, 0, view, proj, eye)
    a.UpdateFrame(0.0, 0, view, proj, eye)
    assert not np.array_equal(pictures(a, fx.Fluid.OPTIMIZED)["cube"], pictures(b, fx.Fluid.OPTIMIZED)["cube"])
    a.Release()
    b.Release()


# ---- 10: random lights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_lights(seed):
    rng = np.random.default_rng(1000 + seed)
    X = (32, 40)[seed & 1]
    use_sh = bool(seed & 2)
    flags = FLAGS[(seed >> 2) % 4] if seed < 8 else FLAGS[seed % 4]
    kind = "point" if rng.random() < 0.7 else "directional"
    position = tuple(float(v) for v in rng.uniform(-14.0, 14.0, 3))   # in and around the volume [-10, 10]^3
    color = tuple(float(v) for v in np.concatenate([rng.random(3), rng.uniform(0.0, 12.0, 1)]))
    ambient = tuple(float(v) for v in np.concatenate([rng.random(3), rng.uniform(0.0, 6.0, 1)]))
    f, view, proj, eye = make(X, scene_of(X), sh=sh27() if use_sh else None, max_samples=(96, 24))
    f.SetLight(position, kind, color, ambient)
    got = f.GetLight()
    assert got["kind"] == kind and np.array_equal(np.array(got["position"], f32), np.array(position, f32))
    f.set_option(capi.OPT_RENDER_ACCEL, 1)
    a = pictures(f, flags)
    f.set_option(capi.OPT_RENDER_ACCEL, 0)
    b = pictures(f, flags)
    same(a, b)
    assert finite(a)
    assert f._lib.fx_synchronize(f._ctx) == capi.FX_OK
    f.Release()
