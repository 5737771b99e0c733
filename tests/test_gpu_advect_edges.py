"""The staged advection (csrc/fx_advect_lds.hip: k_advect_lds, k_advect_far) at the edges its gather kernels are held to.  Recipes, references
and their conditions: tests/advect_edges.py, held on the CPU alone by tests/test_advect_edges.py, which also asks fx::advect_lds_plan that
every grid here reaches the instantiation, tiles and chunks advect_edges.PLAN names.

Three kernel settings, shipped switches only (advect_edges.KERNELS): staged with the far voxels deferred to k_advect_far, staged with the
gathers inside the kernel, and the gather kernels k_advect_fast / k_advect.  Every test calls fx_advect once on uploaded fields.

  geometry   five grids x storage x addressing x three velocity scales: the three settings agree bit for bit over the whole field; the staged
             result == the model bit for bit over the whole field with the impulse off, == the oracle outside the ball with it on
  recipe A   fp16 stores into the binary16 subnormals and of -0: binary16 bit patterns, whole field, all three settings == the model
  recipe B   fp32 subnormal fields: bit for bit, whole field
  recipe C   +-inf and NaN in every input plane: NaN exactly where the model has NaN, every other value bit for bit, all three settings; a
             voxel whose own velocity is not finite stores NaN in all seven quantities
  alpha      recipe C behind a render: the staged kernels write the render's alpha side volume (<ALPHA>); accelerated == plain, six pictures
"""
import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import advect_edges as ae
import render_edges as re_
from test_gpu_render_edges import assert_same_pictures, pictures

pytestmark = pytest.mark.gpu
f32 = np.float32
ids = ae.ids


def advect(c, knob, setting, impulse):
    """(VELOCITY1, COLOR) behind one fx_advect of case c under a kernel setting"""
    for name, value in ae.KERNELS[setting].items():
        knob(name, value)
    f = fx.Fluid()
    assert f.Init(320, 240, c.dims, storage=c.storage, advect_address=c.address), f.last_status
    assert f32(f.default_time_step()) == c.dt
    f.SetImpulse(impulse)
    f.upload(fx.FIELD_VELOCITY, c.vel)
    f.upload(fx.FIELD_COLOR, c.col)                          # parity 0 -> UpdateFrame flips: the advection reads this one
    f.UpdateFrame(c.dt, 0)
    f.Advect()
    f.Synchronize()
    out = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.Release()
    return out


def three(c, knob, impulse=False):
    return {k: advect(c, knob, k, impulse) for k in ae.KERNELS}


def assert_same(got, want, what):
    """(velocity, colour) pairs: NaN exactly where `want` has one, every other value bit for bit"""
    for name, g, w in zip(("velocity", "colour"), got, want):
        ok, n, first = ae.same_but_nan(g, w)
        assert ok, (what, name, n, first, [(float(g[tuple(i)]), float(w[tuple(i)])) for i in first[:3]])


def assert_same_outside_the_ball(c, got, what):
    far = c.far
    assert_same((got[0][:, far], got[1][far]), (c.orc_vel[:, far], c.orc_col[far]), what)


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ae.SCALES)
@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("storage", ae.STORAGES)
@pytest.mark.parametrize("dims", ae.SHAPES, ids=ids)
def test_geometry(dims, storage, address, scale, knob):
    c = ae.geometry(dims, storage, address, scale)
    ae.assert_conditions(c)
    got = three(c, knob)
    for k in ("inline", "gather"):
        assert ae.same_bits(got[k][0], got["staged"][0]) and ae.same_bits(got[k][1], got["staged"][1]), (c.what, k)
    assert ae.same_bits(got["staged"][0], c.want_vel) and ae.same_bits(got["staged"][1], c.want_col), \
        (c.what, ae.same_but_nan(got["staged"][0], c.want_vel)[1:], ae.same_but_nan(got["staged"][1], c.want_col)[1:])
    on = advect(c, knob, "staged", True)
    assert not ae.same_bits(on[1], got["staged"][1])         # the impulse took part
    assert_same_outside_the_ball(c, on, c.what + " with the impulse")


# ---- recipe A -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("dims", ae.RANGE_SHAPES, ids=ids)
def test_fp16_stores_into_the_subnormals_and_of_negative_zero(dims, address, knob):
    c = ae.half_edges(dims, address)
    ae.assert_conditions(c)
    want = ae.half_bits(ae.values(c, np.ones(c.inwin.shape, bool)))
    for k, (gv, gc) in three(c, knob).items():
        got = ae.half_bits(ae.values(c, np.ones(c.inwin.shape, bool), gv, gc))
        assert np.array_equal(got, want), (c.what, k, int((got != want).sum()), np.flatnonzero(got != want)[:6].tolist())
    assert_same_outside_the_ball(c, advect(c, knob, "staged", True), c.what + " with the impulse")


# ---- recipe B -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("dims", ae.RANGE_SHAPES, ids=ids)
def test_fp32_subnormal_fields(dims, address, knob):
    c = ae.subnormal(dims, address)
    ae.assert_conditions(c)
    for k, (gv, gc) in three(c, knob).items():
        assert ae.same_bits(gv, c.want_vel) and ae.same_bits(gc, c.want_col), (c.what, k, ae.same_but_nan(gv, c.want_vel)[1:], ae.same_but_nan(gc, c.want_col)[1:])
    assert_same_outside_the_ball(c, advect(c, knob, "staged", True), c.what + " with the impulse")


# ---- recipe C -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ae.ADDRESSES)
@pytest.mark.parametrize("storage", ae.STORAGES)
@pytest.mark.parametrize("dims", ae.RANGE_SHAPES, ids=ids)
def test_non_finite_fields(dims, storage, address, knob):
    c = ae.nonfinite(dims, storage, address)
    ae.assert_conditions(c)
    lost = ae.own_velocity_not_finite(c)
    for k, got in three(c, knob).items():
        assert_same(got, (c.want_vel, c.want_col), "%s %s" % (c.what, k))
        assert ae.all_seven_nan(lost, *got), (c.what, k)
    assert_same_outside_the_ball(c, advect(c, knob, "staged", True), c.what + " with the impulse")


# ---- the alpha side volume behind the staged kernels -----------------------------------------------------------------------------------------
def rendered_then_advected(c, accel):
    """upload, render, one fx_advect: with the accelerated render on, the frame before was rendered on the same stream and the launch is one
    staged launch over the whole grid that defers -- advect_range offers the side volume and advect_lds_plan takes it (<ALPHA>)"""
    f = fx.Fluid()
    assert f.Init(re_.VP[0], re_.VP[1], c.dims, storage=c.storage, advect_address=c.address), f.last_status
    f.SetMaxSamples(re_.NS, re_.NL)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    view, proj, eye = fx.default_camera(*re_.VP)
    f.upload(fx.FIELD_VELOCITY, c.vel)
    f.upload(fx.FIELD_COLOR, c.col)
    f.UpdateFrame(0.0, 0, view, proj, eye)
    f.Render(0, fx.Fluid.OPTIMIZED)
    f.UpdateFrame(c.dt, 1, view, proj, eye)
    f.Advect()
    f.Synchronize()
    return f


@pytest.mark.parametrize("storage", ae.STORAGES)
@pytest.mark.parametrize("dims", ae.ALPHA_SHAPES, ids=ids)
def test_alpha_side_volume_behind_the_staged_kernels(dims, storage, knob):
    c = ae.nonfinite(dims, storage, "clamp")
    ae.assert_conditions(c)
    alpha = c.want_col[..., 3]                               # (the model's, impulse off: the ball only adds ordinary smoke)
    # the advected alpha the render marches through holds the classes: NaN, inf and ordinary smoke
    assert np.isnan(alpha).mean() >= 0.01 and np.isinf(alpha).mean() >= 1e-3 and (np.isfinite(alpha) & (alpha > 0)).mean() > 0.5
    for name, value in ae.KERNELS["staged"].items():
        knob(name, value)
    fa, fp = (rendered_then_advected(c, accel) for accel in (1, 0))
    col = fp.download(fx.FIELD_COLOR)
    assert ae.same_but_nan(fa.download(fx.FIELD_COLOR), col)[0]
    a, p = pictures(fa, 1), pictures(fp, 1)
    assert_same_pictures(a, p, "%s behind the staged advection" % c.what, col)
    fa.Release(); fp.Release()
