"""The render on alpha outside [0, 1] (recipes and their conditions: tests/render_edges.py, tests/test_render_edges.py).

  1  accelerated == plain, bit for bit (DESIGN.md "accelerated = plain bit for bit"), for every value class of alpha x storage x the grids
     that reach each build kernel -- light map, cube map and float target of all four render flags; NaN once more under a point light,
     negative alpha once more behind a scene depth
  2  plain against the oracle on the finite classes and on the colour-channel field, with the bars of tests/test_gpu_render.py unchanged:
     light-map words differing on < 1e-3 of the voxels, cube map <= 1 LSB on <= 2 % of the texels, the direct marches as rgba8_close.
     For NaN and +inf: which light-map values are NaN and which cube-map channels the oracle's NaN sums leave at 0 -- nothing about payloads
  3  the device's pack_r11g11b10 on every branch, through the light map of an empty volume, as 32-bit words against the oracle's packer
  4  the 2-D visualiser on the colour-channel field, bit for bit (where the value is NaN: that it is NaN, not which)
  5  emitter, obstacle, open wall, MacCormack advection and confinement at once, five rendered steps: accelerated == plain

Every class case runs without a light probe; 16^3 uploaded and 32^3 behind a step run once more with one (the three light passes, and
k_build_fill + the three ray launches).  Without the probe 32^3 behind a step is the product's default frame: k_build_fill, k_light_rays
<RAYS_SHADOW>, k_light_fill_repair.

Nothing here checks WHICH build kernel a stepped case ran: that the advection wrote the alpha side volume follows from reading
fx_schedule.cpp advect_range (the frame before was rendered on the same stream, FX_OPT_RENDER_ACCEL on, ADVECT_ALPHA at its default) and
launch_advect, and no output tells the paths apart -- they are equal by contract.  If that condition changes, the stepped cases become
repeats of the uploaded ones on an advected field."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi
from oracle import orc

import emitter_ref as er
import open_ref as orf
import render_edges as re_
import test_obstacle_ref as ob
from test_depth_ref import analytic_depth
from test_gpu_render import cube_close, oracle_frame_of, rgba8_close

pytestmark = pytest.mark.gpu
f32 = np.float32
OUTPUTS = ("light map (optimized)", "cube map (optimized)", "light map (merged cube march: untouched)", "cube map (merged)", "float target (separate direct)",
           "float target (merged direct)")
GRIDS = [(d, False) for d in re_.FRESH_GRIDS] + [(d, True) for d in re_.STEP_GRIDS]
# every case without the light probe; with it, per class and storage: 16^3 uploaded (three light passes), 32^3 behind a step (k_build_fill +
# the three ray launches)
WITH_SH = [((16, 16, 16), False), ((32, 32, 32), True)]
CASES = [(n, s, d, st, sh) for n in re_.CLASSES for s in re_.storages(n) for d, st in GRIDS for sh in ([False, True] if (d, st) in WITH_SH else [False])]


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def case_id(c):
    return "-".join((c[0], c[1], "x".join(map(str, c[2])), "stepped" if c[3] else "uploaded") + (("probe",) if c[4] else ()))


def camera():
    return fx.default_camera(*re_.VP)


def context(dims, col, storage, accel, use_sh=False, stepped=False):
    """a context that holds `col` -- or, stepped, what one step at rest makes of it, with the advection's alpha side volume current where
    the accelerated path is on (render_edges: a render, then fx_simulate with the impulse off)"""
    f = fx.Fluid()
    assert f.Init(re_.VP[0], re_.VP[1], dims, storage=storage, jacobi_iters=4), f.last_status
    f.SetMaxSamples(re_.NS, re_.NL)
    if use_sh:
        f.SetSH(re_.SH)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    view, proj, eye = camera()
    f.upload(fx.FIELD_COLOR, col)
    f.UpdateFrame(0.0, 0, view, proj, eye)
    if stepped:
        f.SetImpulse(False)
        f.Render(0, fx.Fluid.OPTIMIZED)
        f.UpdateFrame(re_.STEP_DT, 1, view, proj, eye)
        f.Simulate(1)
    return f


def pictures(f, index=0):
    """test_empty_space_skipping_changes_no_bit's six outputs"""
    out = []
    for flags in (fx.Fluid.OPTIMIZED, fx.Fluid.RAY_MARCH_CUBEMAP):
        f.Render(index, flags)
        f.Synchronize()
        out += [f.download(fx.FIELD_LIGHTMAP), f.download(fx.FIELD_CUBEMAP)]
    for flags in (fx.Fluid.SEPARATE_LIGHT_PASS, fx.Fluid.RAY_MARCH_DIRECT):
        f.ClearRenderTarget()
        f.Render(index, flags)
        f.Synchronize()
        out.append(f.download(fx.FIELD_TARGET_FLOAT))
    return out


def differing(a, b):
    return int((a.view(np.uint8) != b.view(np.uint8)).reshape(-1, a.itemsize * a.shape[-1]).any(axis=1).sum())


def assert_same_pictures(a, b, what, col=None):
    counts = [differing(u, v) for u, v in zip(a, b)]
    print("%s: accelerated vs plain, differing words / texels / pixels: %s" % (what, dict(zip(OUTPUTS, counts))))
    if counts[0] and col is not None:                                # where the light maps part, and what the field holds there
        alpha = col[..., 3]
        for z, y, x in np.argwhere((re_.bits(a[0]) != re_.bits(b[0])).any(axis=-1))[:16]:
            near = alpha[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
            print("  voxel z %d y %d x %d: accelerated %s plain %s alpha %r; of the 3^3 around it %d NaN, %d inf, max %r" %
                  (z, y, x, a[0][z, y, x], b[0][z, y, x], float(alpha[z, y, x]), int(np.isnan(near).sum()), int(np.isinf(near).sum()), float(np.nanmax(near))))
    assert not any(counts), (what, dict(zip(OUTPUTS, counts)))


def oracle_frame(f, dims, use_sh):
    view, proj, eye = camera()
    fr, lod, rs, mask, _ = orc.update_frame(view, proj, eye, re_.VP[0], re_.VP[1], dims[0], re_.NS)
    fi = f.frame_info()
    assert (fi.cube_lod, fi.ray_samples, fi.visibility_mask) == (lod, rs, mask)
    if use_sh:
        for i, v in enumerate(re_.SH.reshape(27)):
            fr.sh[i] = v
    _, wvp_i = oracle_frame_of(f, view, proj, eye, dims[0])
    return fr, lod, rs, mask, wvp_i


def clear_target():
    t = np.empty((re_.VP[1], re_.VP[0], 4), np.uint8)
    t[...] = (51, 51, 51, 0)
    return t


def plain_against_the_oracle(f, pics, col, dims, use_sh, what, finite, index=0):
    """`pics` = pictures(f) of the plain kernels on `col`.  finite: the project's bars; else only where the NaN are"""
    fr, lod, rs, mask, wvp_i = oracle_frame(f, dims, use_sh)
    W, H = re_.VP
    with np.errstate(all="ignore"):
        lm_ref = orc.raymarch_light(col, fr, re_.NL, use_sh, 2)
        cf, cu = orc.raymarch_view(col, lm_ref, fr, dims[0] >> lod, mask, rs, re_.NL, use_sh, True)
        cf2, cu2 = orc.raymarch_view(col, None, fr, dims[0] >> lod, mask, rs, re_.NL, use_sh, False)
    lm, cube, _, cube2 = pics[:4]
    if not finite:
        print("%s: %d light-map values NaN in the oracle, %d on the device; %d / %d cube channels NaN in the oracle's sums" %
              (what, int(np.isnan(lm_ref).sum()), int(np.isnan(lm).sum()), int(np.isnan(cf).sum()), int(np.isnan(cf2).sum())))
        assert np.array_equal(np.isnan(lm), np.isnan(lm_ref))
        assert not cube[np.isnan(cf)].any() and not cube2[np.isnan(cf2)].any()       # to_unorm8(NaN) = 0
        return
    share = float((lm != lm_ref).any(axis=-1).mean())
    d1, d2 = (np.abs(c.astype(np.int32) - r.astype(np.int32)) for c, r in ((cube, cu), (cube2, cu2)))
    print("%s: light map differs on %.6f of the voxels; cube map max %d LSB on %.5f of the texels, merged max %d LSB on %.5f" %
          (what, share, int(d1.max()), float((d1 > 0).mean()), int(d2.max()), float((d2 > 0).mean())))
    assert not np.isnan(lm_ref).any() and not np.isnan(lm).any()
    assert share < 1e-3
    cube_close(cube, cu)
    cube_close(cube2, cu2)
    # the direct marches, on the blended RGBA8 target
    with np.errstate(all="ignore"):
        sep, cov = orc.raycast_direct(col, lm_ref, fr, wvp_i, W, H, rs, re_.NL, use_sh, True)
        mer, cov2 = orc.raycast_direct(col, None, fr, wvp_i, W, H, re_.NS, re_.NL, use_sh, False)
    for flags, out, c in ((fx.Fluid.SEPARATE_LIGHT_PASS, sep, cov), (fx.Fluid.RAY_MARCH_DIRECT, mer, cov2)):
        f.ClearRenderTarget()
        f.Render(index, flags)
        f.Synchronize()
        rgba8_close(f.download(fx.FIELD_TARGET), orc.blend_premultiplied(out, c, clear_target()))


# ---- 1, 2: the classes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,storage,dims,stepped,use_sh", CASES, ids=[case_id(c) for c in CASES])
def test_alpha_classes_accelerated_equals_plain_equals_oracle(name, storage, dims, stepped, use_sh):
    c = re_.class_field(dims, name, stepped)
    what = "%s %s %s%s%s" % (name, storage, dims, " behind a step" if stepped else "", " with the light probe" if use_sh else "")
    fa, fp = (context(dims, c.col, storage, accel, use_sh, stepped) for accel in (1, 0))
    index = 1 if stepped else 0
    col = fp.download(fx.FIELD_COLOR)
    if stepped:
        # the render's input is the device's advected field: the class is still in it, in both contexts alike
        assert re_.same_bits(col, fa.download(fx.FIELD_COLOR))
        re_.assert_conditions(re_.case(conditions=re_.stepped_conditions(col[..., 3], c)))
    else:
        assert re_.same_bits(col, c.col)
    a, p = pictures(fa, index), pictures(fp, index)
    assert p[1][..., 3].max() > 30                                    # the body is seen
    assert_same_pictures(a, p, what, col)
    plain_against_the_oracle(fp, p, col, dims, use_sh, what, name in re_.FINITE, index)
    fa.Release(); fp.Release()


def test_nan_under_a_point_light_accelerated_equals_plain():
    dims = (16, 16, 16)
    c = re_.class_field(dims, "nan")
    out = []
    for accel in (1, 0):
        f = context(dims, c.col, "fp32", accel)
        f.SetLight((14.0, 18.0, -16.0), "point", (1.0, 0.8, 0.5, 6.0), (0.6, 0.7, 1.0, 0.75))      # outside the volume, up the default light's way
        out.append(pictures(f))
        f.Release()
    assert np.isnan(out[1][0]).any()                                  # the shadow rays to the light cross the NaN
    assert_same_pictures(out[0], out[1], "nan under a point light")


def test_negative_alpha_behind_a_scene_depth_accelerated_equals_plain():
    dims = (16, 16, 16)
    c = re_.class_field(dims, "negative")
    _, proj, _ = camera()
    depth = analytic_depth(proj, re_.VP[0], re_.VP[1], sphere=(0.0, 0.0, 43.0, 5.0))         # a ball in the middle of the volume
    assert 0.02 < (depth < 1).mean() < 0.9
    out = []
    for accel in (1, 0):
        f = context(dims, c.col, "fp32", accel)
        f.SetSceneDepth(depth)
        out.append(pictures(f) + [f.download(fx.FIELD_CUBE_DEPTH)])
        f.Release()
    free = context(dims, c.col, "fp32", 0)
    assert differing(pictures(free)[5], out[1][5]) > 0                # the depth took part
    free.Release()
    assert_same_pictures(out[0], out[1], "negative alpha behind a scene depth")
    assert re_.same_bits(out[0][6], out[1][6])


# ---- 2: the colour channels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_colour_channel_field_accelerated_equals_plain_equals_oracle(storage):
    dims = (32, 32, 32)
    c = re_.colour_field(dims)
    re_.assert_conditions(c)
    fa, fp = (context(dims, c.col, storage, accel) for accel in (1, 0))
    a, p = pictures(fa), pictures(fp)
    assert p[1][..., 3].max() > 30
    assert_same_pictures(a, p, "colour channels %s" % storage)
    plain_against_the_oracle(fp, p, c.col, dims, False, "colour channels %s" % storage, True)
    fa.Release(); fp.Release()


# ---- 3: the packer -----------------------------------------------------------------------------------------------------------------------
def unpacked(word):
    out = np.empty(3, f32)
    orc.lib().orc_unpack_r11g11b10(C.c_uint32(word), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


@pytest.mark.parametrize("dims,accel,stepped", [((8, 8, 8), 1, False), ((8, 8, 8), 0, False), ((16, 16, 16), 1, True)],
                         ids=["8x8x8-accelerated-uploaded", "8x8x8-plain-uploaded", "16x16x16-accelerated-stepped"])
def test_light_map_of_an_empty_volume_is_the_packed_light(dims, accel, stepped):
    """every voxel's word = orc_pack_r11g11b10(light_value): k_light_cells (8^3 uploaded), the plain kernel, k_build_fill (16^3 behind a
    step; the last light twice: the second pass rewrites only cells that held a lit voxel -- none).  The download decodes the word; the
    decoding is one-to-one on the codes that are not NaN, so equal decoded bits are equal words"""
    X, Y, Z = dims
    f = context(dims, np.zeros((Z, Y, X, 4), f32), "fp32", accel, stepped=stepped)
    index = 1 if stepped else 0
    lights = re_.packer_lights()
    for what, color, ambient, want in lights + lights[-1:]:
        got = re_.light_value(color, ambient)
        assert re_.same_bits(got, want)
        word = orc.lib().orc_pack_r11g11b10(float(got[0]), float(got[1]), float(got[2]))
        assert word == re_.plain_pack3(*got)
        f.SetLight((75.0, 75.0, -75.0), "directional", color, ambient)
        f.Render(index, fx.Fluid.OPTIMIZED)
        f.Synchronize()
        lm = f.download(fx.FIELD_LIGHTMAP)
        ref = np.broadcast_to(unpacked(word), lm.shape)
        bad = int((re_.bits(lm) != re_.bits(ref)).any(axis=-1).sum())
        print("%s: word %08x, %d of %d voxels differ (first voxel %s, expected %s)" % (what, word, bad, lm[..., 0].size, lm[0, 0, 0], ref[0, 0, 0]))
        assert bad == 0, what
    f.Release()


# ---- 4: the 2-D visualiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_2d_visualiser_on_the_colour_channel_field_equals_oracle(storage):
    dims, vp = (36, 36, 1), (100, 60)
    c = re_.colour_field(dims)
    re_.assert_conditions(c)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], dims, storage=storage)
    f.upload(fx.FIELD_COLOR, c.col)
    f.UpdateFrame(0.0, 0)
    f.ClearRenderTarget()
    f.Render(0, fx.Fluid.OPTIMIZED)
    f.Synchronize()
    with np.errstate(all="ignore"):
        out = orc.visualize_color(c.col, *vp)
    got = f.download(fx.FIELD_TARGET_FLOAT)
    # bit for bit, but for the sign and payload of a NaN (inf / (inf + 0.5), inf - inf in the filter), which IEEE 754 leaves to the machine:
    # x86 makes the negative default NaN, the GPU the positive one
    nan = np.isnan(out)
    print("visualiser %s: %d of %d values NaN in the oracle, %d on the device; %d values that are no NaN differ" %
          (storage, int(nan.sum()), out.size, int(np.isnan(got).sum()), int((got.view(np.uint32) != out.view(np.uint32))[~nan].sum())))
    assert nan.any() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], out.view(np.uint32)[~nan])
    target = np.empty((vp[1], vp[0], 4), np.uint8)
    target[...] = (51, 51, 51, 0)
    assert np.array_equal(f.download(fx.FIELD_TARGET), orc.blend_premultiplied(out, np.ones(vp[::-1], np.uint8), target))
    f.Release()


# ---- 5: every stage that keeps the side volume true, at once -------------------------------------------------------------------------------
def combined_rounds(accel):
    dims, vp = (32, 32, 32), (160, 120)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], dims, jacobi_iters=10)
    f.SetMaxSamples(48, 16)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    f.SetOpenWalls(orf.Y_HI)
    f.SetObstacles(ob.ball_mask(dims, center=(0.5, 0.7, 0.5), radius=0.12))
    f.SetAdvectionScheme("maccormack")
    f.SetVorticityConfinement(2.0)
    # a strong source under the lid, pushed up against the ball and out through the face
    f.SetEmitters([er.emitter((0.5, 0.85, 0.5), 0.2, color_rate=(8.0, 16.0, 40.0, 400.0), force=(0.0, 40.0, 0.0), swirl=50.0)])
    view, proj, eye = fx.default_camera(*vp)
    dt = f32(f.default_time_step())
    out = []
    for k in range(5):                                               # from the second step on the advection writes the alpha volume
        f.UpdateFrame(dt, k % 3, view, proj, eye)
        f.Simulate(k % 3)
        f.ClearRenderTarget()
        f.Render(k % 3, fx.Fluid.OPTIMIZED)
        f.RenderCube(k % 3)
        f.Synchronize()
        out.append((f.download(fx.FIELD_CUBEMAP), f.download(fx.FIELD_TARGET), f.download(fx.FIELD_COLOR)))
    f.Release()
    return out


def test_all_stages_that_touch_the_side_volume_at_once():
    a, p = combined_rounds(1), combined_rounds(0)
    assert p[-1][0][..., 3].max() > 30 and p[-1][2][..., 3].max() > 0.9               # smoke is seen (the emitter saturates at 1)
    for k, ((cube1, target1, col1), (cube0, target0, col0)) in enumerate(zip(a, p)):
        assert re_.same_bits(col1, col0), k
        assert np.array_equal(cube1, cube0) and np.array_equal(target1, target0), k
