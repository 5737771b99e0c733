"""Vorticity confinement on the GPU (fx_set_vorticity_confinement / fx_confine_vorticity, csrc/fx_vorticity.hip) against the numpy model
tests/vorticity_ref.py, BIT FOR BIT: the pass is fp32 with every operation rounded on its own (no fmaf, correctly rounded sqrtf and /),
so there is no tolerance anywhere in this file."""
import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import vorticity_ref as vr

pytestmark = pytest.mark.gpu
f32 = np.float32
EPS = 8.0


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status        # simulation only: no viewport
    return f


def rand_vel(dims, seed):
    X, Y, Z = dims
    return (np.random.default_rng(seed).standard_normal((3, Z, Y, X)) * 0.5).astype(f32)


def rand_state(dims, seed):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vel = (rng.standard_normal((3, Z, Y, X)) * 0.5).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    return vel, col, p


def explain(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    return "%d of %d differ; first at (c, z, y, x) = %s: got %r want %r; z planes %s" % (
        len(bad), got.size, i, got[i], want[i], sorted(set(bad[:, 1].tolist()))[:12])


# where a z-marching tile kernel can go wrong: rows shorter than the 64-wide tile with walls everywhere; fewer planes than the ring of
# three holds; x seams and a ragged last tile; the reference's preset row length; a power of two; 2-D
SHAPES = [(16, 16, 16), (20, 20, 12), (32, 32, 2), (24, 24, 3), (70, 70, 5), (130, 130, 4), (150, 150, 6), (256, 256, 6), (36, 36, 1), (130, 130, 1)]


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", SHAPES)
def test_stage_matches_the_model_bit_for_bit(dims, storage):
    vel = rand_vel(dims, 101)
    f = make(dims, storage=storage)
    dt = f32(f.default_time_step())
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.UpdateFrame(dt, 0)
    f.SetVorticityConfinement(EPS)
    f.ConfineVorticity()
    f.Synchronize()
    got = f.download(fx.FIELD_VELOCITY1)
    want = vr.confine_stored(vel, EPS, dt, storage == "fp16")
    assert not np.array_equal(want, vel if storage == "fp32" else vel.astype(np.float16).astype(f32))     # the pass does something here
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), explain(got, want)


@pytest.mark.parametrize("dims", [(70, 70, 40), (64, 64, 19)])
def test_several_z_chunks_match_the_model(dims):
    """grids deep enough for the launcher to cut the z march into more than one chunk (two tiles x 8 planes at least; the chunk seams
    re-form m of the planes next to them)"""
    vel = rand_vel(dims, 103)
    f = make(dims)
    dt = f32(f.default_time_step())
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.UpdateFrame(dt, 0)
    f.SetVorticityConfinement(EPS)
    f.ConfineVorticity()
    got = f.download(fx.FIELD_VELOCITY1)
    want = vr.confine(vel, EPS, dt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), explain(got, want)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_stage_twice_is_the_model_twice(storage):
    """the result goes to the other velocity buffer and the two swap: a second call must read the first one's output (a stale scratch
    buffer, or a swap that does not alternate, would show here)"""
    dims = (70, 70, 5)
    vel = rand_vel(dims, 107)
    f = make(dims, storage=storage)
    dt = f32(f.default_time_step())
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.UpdateFrame(dt, 0)
    f.SetVorticityConfinement(EPS)
    f.ConfineVorticity()
    f.ConfineVorticity()
    got = f.download(fx.FIELD_VELOCITY1)
    half = storage == "fp16"
    want = vr.confine_stored(vr.confine_stored(vel, EPS, dt, half), EPS, dt, half)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), explain(got, want)


def run_steps(dims, steps, eps, staged, state, **kw):
    """`steps` steps from `state`: fx_simulate, or the stage calls with the confinement between advection and divergence"""
    vel, col, p = state
    f = make(dims, **kw)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col); f.upload(fx.FIELD_PRESSURE, p)
    if eps is not None:
        f.SetVorticityConfinement(eps)
    dt = f32(f.default_time_step())
    for i in range(steps):
        f.UpdateFrame(dt, i % 3)
        if staged:
            f.Advect(); f.ConfineVorticity(); f.Divergence(); f.Jacobi(kw["jacobi_iters"]); f.Project()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    return [f.download(k) for k in (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE)]


def same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(32, 32, 32), (64, 64, 1)])
def test_simulate_is_the_stage_composition(dims, storage):
    state = rand_state(dims, 109)
    kw = dict(storage=storage, jacobi_iters=10, jacobi_mode="fixed")
    whole = run_steps(dims, 4, EPS, False, state, **kw)
    staged = run_steps(dims, 4, EPS, True, state, **kw)
    assert same(whole, staged)
    assert not same(whole, run_steps(dims, 4, 0.0, False, state, **kw))       # (and the pass took part)


def test_simulate_is_the_stage_composition_faithful():
    """FX_JACOBI_FAITHFUL: the dense sweep's fused divergence reads the confined field.  The premise -- fx_simulate equals the stage calls
    in this mode at all -- is asserted first, with epsilon = 0"""
    dims = (32, 32, 32)
    state = rand_state(dims, 113)
    kw = dict(jacobi_iters=16, jacobi_mode="faithful")
    assert same(run_steps(dims, 4, 0.0, False, state, **kw), run_steps(dims, 4, 0.0, True, state, **kw))
    whole = run_steps(dims, 4, EPS, False, state, **kw)
    assert same(whole, run_steps(dims, 4, EPS, True, state, **kw))
    assert not same(whole, run_steps(dims, 4, 0.0, False, state, **kw))


def test_off_means_off():
    dims = (32, 32, 32)
    state = rand_state(dims, 127)
    kw = dict(jacobi_iters=10)
    never = run_steps(dims, 3, None, False, state, **kw)
    zero = run_steps(dims, 3, 0.0, False, state, **kw)
    on = run_steps(dims, 3, EPS, False, state, **kw)
    assert same(never, zero)
    assert not np.array_equal(on[0], never[0]) and not np.array_equal(on[0], zero[0])


def test_status_codes():
    lib = capi.load()
    slab = fx.Fluid()
    assert slab.Init(0, 0, (32, 32, 32), slab=(0, 16))
    assert lib.fx_set_vorticity_confinement(slab._ctx, 1.0) == capi.FX_E_INVALID
    assert lib.fx_confine_vorticity(slab._ctx, None) == capi.FX_E_INVALID
    ro = fx.Fluid()
    assert ro.Init(64, 64, (32, 32, 32), render_only=True)
    assert lib.fx_set_vorticity_confinement(ro._ctx, 1.0) == capi.FX_E_STATE
    assert lib.fx_confine_vorticity(ro._ctx, None) == capi.FX_E_STATE
    f = make((32, 32, 32))
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert lib.fx_set_vorticity_confinement(f._ctx, bad) == capi.FX_E_INVALID, bad
        with pytest.raises(fx.FluidxError):
            f.SetVorticityConfinement(bad)
    # a refused value changes nothing, and the stage is a no-op while the time step is 0
    vel = rand_vel((32, 32, 32), 131)
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.SetVorticityConfinement(EPS)
    f.UpdateFrame(0.0, 0)
    assert lib.fx_confine_vorticity(f._ctx, None) == capi.FX_OK
    assert np.array_equal(f.download(fx.FIELD_VELOCITY1).view(np.uint32), vel.view(np.uint32))
    # ... and while epsilon is 0
    f.SetVorticityConfinement(0.0)
    f.UpdateFrame(f32(0.1), 1)
    f.ConfineVorticity()
    assert np.array_equal(f.download(fx.FIELD_VELOCITY1).view(np.uint32), vel.view(np.uint32))
    f.SetVorticityConfinement(EPS)
    f.ConfineVorticity()
    assert not np.array_equal(f.download(fx.FIELD_VELOCITY1), vel)


def test_checkpoint_resume(tmp_path):
    """epsilon is configuration, not state: the file holds the fields, the resumed context sets epsilon again and continues bit for bit"""
    dims = (32, 32, 32)
    state = rand_state(dims, 137)
    path = str(tmp_path / "vort.fxck")
    a = make(dims, jacobi_iters=10)
    a.upload(fx.FIELD_VELOCITY, state[0]); a.upload(fx.FIELD_COLOR, state[1]); a.upload(fx.FIELD_PRESSURE, state[2])
    a.SetVorticityConfinement(EPS)
    dt = f32(a.default_time_step())
    for i in range(2):
        a.UpdateFrame(dt, i); a.Simulate(i)
    a.SaveCheckpoint(path)
    for i in range(2, 4):
        a.UpdateFrame(dt, i % 3); a.Simulate(i % 3)
    a.Synchronize()
    b = make(dims, jacobi_iters=10)
    b.LoadCheckpoint(path)
    b.SetVorticityConfinement(EPS)
    for i in range(2, 4):
        b.UpdateFrame(dt, i % 3); b.Simulate(i % 3)
    b.Synchronize()
    for k in (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE):
        assert np.array_equal(a.download(k).view(np.uint32), b.download(k).view(np.uint32)), k
