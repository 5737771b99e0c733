"""Scene depth on the MI355X (fx_set_scene_depth, the reference's _HAS_DEPTH_MAP_ variants): a far-plane buffer changes no bit, the
direct and cube-map marches and the depth-weighted resolve equal the depth-aware CPU reference (tests/depth_ref/), the accelerated
kernels equal the plain ones with depth attached, occlusion is monotonic in depth, both ways of passing the buffer agree, and bad
arguments are refused without harm."""
import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi
from oracle import orc
from test_depth_ref import analytic_depth, ref_direct, ref_resolve, ref_view, smoke_scene, world_view_proj_rows

pytestmark = pytest.mark.gpu
f32 = np.float32
VP = (200, 150)
FLAGS = (fx.Fluid.RAY_MARCH_DIRECT, fx.Fluid.RAY_MARCH_CUBEMAP, fx.Fluid.SEPARATE_LIGHT_PASS, fx.Fluid.OPTIMIZED)


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


def pictures(f, flags, resolve=True):
    f.ClearRenderTarget()
    f.Render(0, flags)
    out = {"target_float": None}
    if flags & fx.Fluid.RAY_MARCH_CUBEMAP:
        out["cube"] = f.download(fx.FIELD_CUBEMAP)
        if resolve:
            f.RenderCube(0)
    f.Synchronize()
    out["target"] = f.download(fx.FIELD_TARGET)
    out["target_float"] = f.download(fx.FIELD_TARGET_FLOAT)
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def sh27():
    return (np.random.default_rng(4).random((9, 3)) * np.array([[2.0]] + [[0.5]] * 8)).astype(f32)


def frame_of(f, view, proj, eye, X, max_samples=48):
    fr, lod, rs, mask, _ = orc.update_frame(view, proj, eye, f.viewport[0], f.viewport[1], X, max_samples)
    fi = f.frame_info()
    assert (fi.cube_lod, fi.ray_samples, fi.visibility_mask) == (lod, rs, mask)
    return fr, lod, rs, mask, np.array(list(fi.world_view_proj_i), f32).reshape(4, 4)


def scene_depth(proj, vp, eye):
    dist = float(np.linalg.norm(eye))
    return analytic_depth(proj, vp[0], vp[1], plane=(0.8, 0.2, dist), sphere=(2.0, -1.0, dist - 9.0, 4.0))


# ---- 1: a far-plane depth changes no bit; detaching restores the pictures ------------------------------------------------------------
@pytest.mark.parametrize("storage,use_sh,accel", [("fp32", False, 1), ("fp32", True, 1), ("fp16", False, 1), ("fp16", True, 0), ("fp32", False, 0)])
def test_far_plane_depth_changes_no_bit(storage, use_sh, accel):
    X = 32
    col = smoke_scene(X)
    f, view, proj, eye = make(X, col, storage=storage, sh=sh27() if use_sh else None, accel=accel)
    for flags in FLAGS:
        base = pictures(f, flags)
        f.SetSceneDepth(np.ones((VP[1], VP[0]), f32))
        same(pictures(f, flags), base)
        f.SetSceneDepth(None)
        same(pictures(f, flags), base)
    f.Release()


# ---- 2: direct march against the depth-aware reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("flags,use_sh", [(fx.Fluid.RAY_MARCH_DIRECT, False), (fx.Fluid.RAY_MARCH_DIRECT, True), (fx.Fluid.SEPARATE_LIGHT_PASS, False)])
def test_direct_march_with_depth_equals_the_reference(flags, use_sh):
    X = 32
    col = smoke_scene(X)
    sh = sh27() if use_sh else None
    f, view, proj, eye = make(X, col, sh=sh)
    fr, lod, rs, mask, wvp_i = frame_of(f, view, proj, eye, X)
    if use_sh:
        for i, v in enumerate(sh.reshape(27)):
            fr.sh[i] = v
    depth = scene_depth(proj, VP, eye)
    assert (depth < 1).mean() > 0.5
    separate = bool(flags & fx.Fluid.SEPARATE_LIGHT_PASS)
    lm = orc.raymarch_light(col, fr, 16, use_sh, 2) if separate else None
    ns = rs if separate else 48
    out, cov = ref_direct(col, lm, fr, wvp_i, VP[0], VP[1], ns, 16, use_sh, separate, depth)
    nodepth = pictures(f, flags)
    f.SetSceneDepth(depth)
    got = pictures(f, flags)
    gf = got["target_float"]
    if separate:
        assert np.mean(gf != out) < 2e-3 and np.abs(gf - out).max() < 0.05
    else:
        assert np.array_equal(gf.view(np.uint32), out.view(np.uint32))
    target = np.empty((VP[1], VP[0], 4), np.uint8)
    target[...] = (51, 51, 51, 0)
    d = np.abs(got["target"].astype(np.int32) - orc.blend_premultiplied(out, cov, target).astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() <= 0.002
    # scene points behind the volume: the no-depth picture bit for bit; and the occluder does hide smoke
    behind = depth >= analytic_depth(proj, VP[0], VP[1], plane=(0.0, 0.0, float(np.linalg.norm(eye)) + 18.0))
    assert behind.mean() > 0.05
    assert np.array_equal(gf[behind].view(np.uint32), nodepth["target_float"][behind].view(np.uint32))
    assert gf[..., 3].sum() < 0.95 * nodepth["target_float"][..., 3].sum()
    f.Release()


# ---- 3: cube path (march, cube depth, weighted resolve) against the reference ---------------------------------------------------------
def check_cube_depth(got, ref, ray):
    diff = (got != ref) & ray
    assert diff.mean() <= 1e-3, float(diff.mean())
    for fc, y, x in zip(*np.nonzero(diff)):                         # a uv on a texel boundary may pick the neighbour: it holds a neighbour's value
        nb = ref[fc, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
        assert np.any(nb == got[fc, y, x]), (fc, y, x)


@pytest.mark.parametrize("separate,X,vp", [(True, 32, VP), (False, 32, VP), (True, 64, (96, 72))])
def test_cube_path_with_depth_equals_the_reference(separate, X, vp):
    col = smoke_scene(X)
    f, view, proj, eye = make(X, col, vp=vp)
    fr, lod, rs, mask, wvp_i = frame_of(f, view, proj, eye, X)
    if X == 64:
        assert lod >= 1                                              # a coarser cube mip
    depth = scene_depth(proj, vp, eye)
    lm = orc.raymarch_light(col, fr, 16, False, 2) if separate else None
    cf, cu, cd = ref_view(col, lm, fr, X >> lod, mask, rs, 16, False, separate, depth, world_view_proj_rows(view, proj), wvp_i)
    f.SetSceneDepth(depth)
    flags = fx.Fluid.OPTIMIZED if separate else fx.Fluid.RAY_MARCH_CUBEMAP
    got = pictures(f, flags)
    gd = f.download(fx.FIELD_CUBE_DEPTH)
    ray = np.zeros(gd.shape, bool)
    ray[[k for k in range(6) if mask >> k & 1]] = True
    assert (cd[ray] < 1).mean() > 0.05
    check_cube_depth(gd, cd, ray)
    dd = np.abs(got["cube"].astype(np.int32) - cu.astype(np.int32))
    assert dd.max() <= 2 and (dd > 0).mean() <= 0.02, (int(dd.max()), float((dd > 0).mean()))
    # the weighted resolve of the library's own cube map + cube depth
    out, cov = ref_resolve(got["cube"], gd, fr, wvp_i, depth)
    target = np.empty((vp[1], vp[0], 4), np.uint8)
    target[...] = (51, 51, 51, 0)
    d = np.abs(got["target"].astype(np.int32) - orc.blend_premultiplied(out, cov, target).astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() <= 0.002, (int(d.max()), float((d > 0).mean()))
    plain, _ = orc.resolve_cube(got["cube"], fr, wvp_i, vp[0], vp[1])
    assert not np.array_equal(plain, out)                            # the weights did something
    f.Release()


# ---- 4: accelerated = plain with depth attached -------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", [64, 288])
def test_accelerated_equals_plain_with_depth(X):
    vp = (160, 120)
    col = smoke_scene(X, steps=4) if X <= 64 else np.clip(np.random.default_rng(1).random((X, X, X, 4), f32) ** 8, 0, 1)
    f, view, proj, eye = make(X, col, vp=vp, max_samples=(96, 16))
    f.SetSceneDepth(scene_depth(proj, vp, eye))
    for flags in FLAGS:
        f.set_option(capi.OPT_RENDER_ACCEL, 1)
        a = pictures(f, flags)
        da = f.download(fx.FIELD_CUBE_DEPTH) if flags & 1 else None
        f.set_option(capi.OPT_RENDER_ACCEL, 0)
        b = pictures(f, flags)
        same(a, b)
        if da is not None:
            assert np.array_equal(da, f.download(fx.FIELD_CUBE_DEPTH))
    f.Release()


# ---- 5: monotonic in depth; depth 0 = the first sample only ------------------------------------------------------------------------
def test_occlusion_is_monotonic_in_depth():
    X = 32
    col = smoke_scene(X)
    f, view, proj, eye = make(X, col)
    dist = float(np.linalg.norm(eye))
    for flags in (fx.Fluid.RAY_MARCH_DIRECT, fx.Fluid.SEPARATE_LIGHT_PASS):
        prev = None
        for c in (dist - 15, dist - 5, dist, dist + 5, dist + 15):
            f.SetSceneDepth(analytic_depth(proj, VP[0], VP[1], plane=(0.0, 0.0, c)))
            a = pictures(f, flags)["target_float"][..., 3]
            if prev is not None:
                assert np.all(a >= prev)
            prev = a
        f.SetSceneDepth(np.zeros((VP[1], VP[0]), f32))
        occluded = pictures(f, flags)
        f.SetSceneDepth(None)
        f.SetMaxSamples(1, 16)
        f.UpdateFrame(0.0, 0, view, proj, eye)
        one = pictures(f, flags)
        f.SetMaxSamples(48, 16)
        f.UpdateFrame(0.0, 0, view, proj, eye)
        same(occluded, one)
    f.Release()


# ---- 6: device buffer = host copy; the gathered render-only context composites like the single domain ---------------------------------
def test_device_and_host_depth_agree():
    torch = pytest.importorskip("torch")
    X = 32
    col = smoke_scene(X)
    f, view, proj, eye = make(X, col)
    depth = scene_depth(proj, VP, eye)
    for flags in FLAGS:
        f.SetSceneDepth(depth)
        a = pictures(f, flags)
        dev = torch.from_numpy(depth).to("cuda:0")
        torch.cuda.synchronize()
        f.SetSceneDepth(dev)
        b = pictures(f, flags)
        same(a, b)
    f.SetSceneDepth(None)
    f.Release()


def test_gathered_render_only_context_composites_like_the_single_domain():
    X, vp = 32, VP
    col = smoke_scene(X)
    view, proj, eye = fx.default_camera(*vp)
    depth = scene_depth(proj, vp, eye)
    single, *_ = make(X, col)
    single.SetSceneDepth(depth)
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
    ranks[0].gather_color(full, root=0)                             # a loop-back group: the driver gathers for every member
    full.UpdateFrame(0.0, 0, view, proj, eye)
    full.SetSceneDepth(depth)
    for flags in FLAGS:
        same(pictures(full, flags), pictures(single, flags))
    for o in [full, single] + ranks:
        o.Release()


# ---- 7: errors leave the context able to render ------------------------------------------------------------------------------------
def test_scene_depth_errors():
    X = 32
    col = smoke_scene(X)
    f, view, proj, eye = make(X, col)
    lib, ctx = f._lib, f._ctx
    ok = np.ones((VP[1], VP[0]), f32)
    p = ok.ctypes.data_as(capi.C.c_void_p)
    base = pictures(f, fx.Fluid.OPTIMIZED)
    assert lib.fx_set_scene_depth(ctx, None, p, VP[0] + 1, VP[1], 1.0, 1000.0, 0) == capi.FX_E_INVALID      # wrong size
    assert lib.fx_set_scene_depth(ctx, None, p, VP[0], VP[1], 5.0, 5.0, 0) == capi.FX_E_INVALID             # z_near >= z_far
    assert lib.fx_set_scene_depth(ctx, None, p, VP[0], VP[1], 0.0, 1000.0, 0) == capi.FX_E_INVALID          # z_near <= 0
    assert lib.fx_set_scene_depth(ctx, None, p, VP[0], VP[1], 1.0, 1000.0, 0x2) == capi.FX_E_INVALID        # unknown flags
    assert lib.fx_set_scene_depth(ctx, None, p, VP[0], VP[1], 1.0, 1000.0, capi.DEPTH_DEVICE) == capi.FX_E_INVALID   # host memory as device
    same(pictures(f, fx.Fluid.OPTIMIZED), base)
    f.Release()
    g2 = fx.Fluid()
    assert g2.Init(64, 64, (32, 32, 1))                                                                     # 2-D context
    assert g2._lib.fx_set_scene_depth(g2._ctx, None, np.ones((64, 64), f32).ctypes.data_as(capi.C.c_void_p), 64, 64, 1.0, 1000.0, 0) == capi.FX_E_INVALID
    g2.Release()
    g0 = fx.Fluid()
    assert g0.Init(0, 0, (32, 32, 32))                                                                      # 0 x 0 viewport
    assert g0._lib.fx_set_scene_depth(g0._ctx, None, p, 0, 0, 1.0, 1000.0, 0) == capi.FX_E_INVALID
    g0.Release()
