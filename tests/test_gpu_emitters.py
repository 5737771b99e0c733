"""The settable emitters and the switch of the built-in impulse on the GPU (fx_set_emitters / fx_set_impulse / fx_emit, csrc/fx_emit.hip).

Against the numpy model tests/emitter_ref.py there are two criteria, and no other tolerance in this file:
  * outside every emitter's support the pass leaves the bits alone;
  * inside, rel-L2 < 1e-6 for velocity and for colour -- the figure tests/test_gpu_sim.py::test_advect_matches_oracle uses for the built-in
    ball (the model evaluates exp2 in float64, the device in fp32).
The comparison asserts first that no cell of its inputs has a basis within relative 1e-5 of the threshold e^-4, where one ulp of exp2 would
decide the side.  Everything else here is bit for bit: k_emit against the advection kernels' own impulse, the switch, list order, fx_simulate
against the stage calls, the untouched default, and the render's alpha side volume."""
import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import emitter_ref as er

pytestmark = pytest.mark.gpu
f32 = np.float32

# (centre, radius): the built-in ball's place, one well inside, one clipped by two walls, one more, the whole grid, and one without a cell
SIX = [((0.5, 0.1, 0.5), 1 / 16), ((0.3, 0.6, 0.4), 0.11), ((0.02, 0.97, 0.5), 0.2), ((0.7, 0.3, 0.55), 0.13), ((0.5, 0.5, 0.5), 1.0),
       ((0.41, 0.37, 0.52), 0.004)]
# a power of two; rows shorter than the 64-wide tile; ragged second x tiles; the 32-bit-offset path at the tuned row length; 2-D
SHAPES = [(32, 32, 32), (20, 20, 12), (70, 70, 5), (130, 130, 4), (256, 256, 6), (36, 36, 1), (64, 64, 1)]
# tests/test_gpu_sim.py DIMS
DIMS = [(32, 32, 32), (64, 64, 16), (20, 20, 12), (150, 150, 6), (64, 64, 1), (36, 36, 1), (70, 70, 5), (130, 130, 4), (201, 201, 3)]
# Which advection kernel serves a launch: the switches the parity tests of tests/test_gpu_sim.py use.  A switch states a preference; the
# launchers decide by the geometry (fx_sim.hip launch_advect, fx_advect_lds.hip launch_advect_lds), so every entry runs on grids where
# its kernel is the one that is launched:
#   k_advect          any grid with ADVECT_LDS = 0 and ADVECT_FAST = 0
#   k_advect_fast     ADVECT_LDS = 0 on grids whose extents are powers of two
#   k_advect_lds      ADVECT_LDS = 2 (the staged path also below the size where it pays) on 3-D grids with X >= 64, Y >= 8 and 12 planes or
#                     more; ADVECT_DEFER = 0: the instantiation that gathers far-tracing voxels itself
#   k_advect_lds+far  the same with ADVECT_DEFER = 1: the deferring instantiation, and k_advect_far for the voxels that trace beyond the
#                     staged window (none with a zero velocity; most rows of the random fields below)
KERNELS = {"k_advect": (("ADVECT_LDS", "0"), ("ADVECT_FAST", "0")), "k_advect_fast": (("ADVECT_LDS", "0"),),
           "k_advect_lds": (("ADVECT_LDS", "2"), ("ADVECT_DEFER", "0")), "k_advect_lds+far": (("ADVECT_LDS", "2"), ("ADVECT_DEFER", "1"))}
STAGED = ("k_advect_lds", "k_advect_lds+far")
POW2 = [d for d in DIMS if all(v & (v - 1) == 0 for v in d)]
STAGED_DIMS = [(64, 64, 16), (64, 64, 64), (150, 150, 24)]         # (64, 64, 16) is the one of DIMS the staged path takes
# grids where a zero velocity traces exactly onto the cell (powers of two), per kernel
EXACT_CASES = [(k, d, "fp32") for k in ("k_advect", "k_advect_fast") for d in [(32, 32, 32), (64, 64, 1)]] + \
              [(k, d, st) for k in STAGED for d in [(64, 64, 16), (64, 64, 64)] for st in ("fp32", "fp16")]
RANDOM_CASES = [("k_advect", d, "fp32") for d in DIMS] + [("k_advect_fast", d, "fp32") for d in POW2] + \
               [(k, d, st) for k in STAGED for d in STAGED_DIMS for st in ("fp32", "fp16")]
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)


def six():
    return [er.emitter(c, r, color_rate=(0.5 + k, 1.0 + 2 * k, 3.0, 2.0 + k), force=(10.0 * k - 20.0, 30.0 + 7 * k, 5.0 * k), swirl=40.0 * k - 60.0)
            for k, (c, r) in enumerate(SIX)]


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status        # simulation only: no viewport
    return f


def rand_fields(dims, seed, half=False, scale=0.5):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vel = (rng.standard_normal((3, Z, Y, X)) * scale).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    if half:
        vel, col = vel.astype(np.float16).astype(f32), col.astype(np.float16).astype(f32)
    return vel, col


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.sqrt((b ** 2).sum())
    d = np.sqrt(((a - b) ** 2).sum())
    return d / n if n > 0 else d


def bits(a):
    return a.view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def emit_once(dims, storage, vel, col, emitters, dt):
    f = make(dims, storage=storage)
    f.UpdateFrame(dt, 0)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetEmitters(emitters)
    f.Emit()
    f.Synchronize()
    out = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.Release()
    return out


def check_against_model(dims, storage, vel, col, emitters, dt):
    assert er.near_threshold(dims, emitters) == 0                    # the precondition: nothing is excluded, the cap is zero cells
    gv, gc = emit_once(dims, storage, vel, col, emitters, dt)
    wv, wc, m = er.apply(vel, col, emitters, dt, half=storage == "fp16")
    assert m.any()
    assert same_bits(gv[:, ~m], vel[:, ~m]) and same_bits(gc[~m], col[~m])
    ev, ec = rel_l2(gv[:, m], wv[:, m]), rel_l2(gc[m], wc[m])
    print("%s %s: in-support rel-L2 velocity %.3g colour %.3g (%d cells)" % (dims, storage, ev, ec, int(m.sum())))
    assert not same_bits(gv, vel) and not same_bits(gc, col)         # the pass changed something
    assert ev < 1e-6 and ec < 1e-6, (ev, ec)


# ---- 1: the stage against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", SHAPES)
def test_stage_matches_the_model(dims, storage):
    vel, col = rand_fields(dims, 211, half=storage == "fp16")
    f = make(dims)
    dt = f32(f.default_time_step())
    f.Release()
    check_against_model(dims, storage, vel, col, six(), dt)


# ---- 2: the anchor to the kernels the oracle and the DXBC goldens pin -----------------------------------------------------------------
# From zero fields the trace is zero, so no voxel is deferred: k_advect_far, which shares advect_finish with k_advect_lds, is held to the
# gather kernels under random velocities in section 3 instead.
ANCHOR_CASES = [("k_advect", d) for d in [(32, 32, 32), (20, 20, 12), (70, 70, 5), (64, 64, 1), (36, 36, 1)]] + \
               [("k_advect_fast", d) for d in [(32, 32, 32), (64, 64, 1)]] + [(k, d) for k in STAGED for d in [(64, 64, 16), (150, 150, 24)]]


@pytest.mark.parametrize("kernel,dims", ANCHOR_CASES)
def test_builtin_constants_reproduce_the_builtin_impulse_bit_for_bit(kernel, dims, knob):
    """from zero fields the trace is zero: the built-in leaves rn(injection * atten), an emitter with its constants the injection itself"""
    for name, value in KERNELS[kernel]:
        knob(name, value)
    a = make(dims)
    dt = f32(a.default_time_step())
    a.UpdateFrame(dt, 0)
    a.Advect()
    a.Synchronize()
    av, ac = a.download(fx.FIELD_VELOCITY1), a.download(fx.FIELD_COLOR)
    b = make(dims)
    b.SetImpulse(0)
    b.SetEmitters([er.BUILTIN_3D if dims[2] > 1 else er.BUILTIN_2D])
    b.UpdateFrame(dt, 0)
    b.Advect()
    assert not b.download(fx.FIELD_VELOCITY1).any() and not b.download(fx.FIELD_COLOR).any()       # the switch is off
    b.Emit()
    b.Synchronize()
    bv, bc = b.download(fx.FIELD_VELOCITY1), b.download(fx.FIELD_COLOR)
    atten = np.maximum(er.fma(-dt, f32(0.200000003), f32(1.0)), f32(0.0))
    assert ac.any() and av.any()
    assert same_bits((bv * atten).astype(f32), av)
    assert same_bits((bc * atten).astype(f32), ac)


# ---- 3: the switch, for every advection kernel ------------------------------------------------------------------------------------------
def ball_far(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return ((x + .5) / X - .5) ** 2 + ((y + .5) / Y - .1) ** 2 + ((z + .5) / Z - .5) ** 2 > (1.5 / 16) ** 2     # as tests/test_gpu_sim.py cuts it


def advect_once(dims, vel, col, impulse, **kw):
    f = make(dims, **kw)
    dt = f32(f.default_time_step())
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)      # (UpdateFrame flips the parity: the advection reads this colour)
    f.SetImpulse(impulse)
    f.UpdateFrame(dt, 0)
    f.Advect()
    f.Synchronize()
    out = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR), dt
    f.Release()
    return out


def select(knob, kernel):
    for name, value in KERNELS[kernel]:
        knob(name, value)


def stored(a, storage):
    return a.astype(np.float16).astype(f32) if storage == "fp16" else a


@pytest.mark.parametrize("kernel,dims,storage", EXACT_CASES)
def test_switch_off_leaves_the_pure_advection(kernel, dims, storage, knob):
    """grids where a zero velocity traces exactly onto the cell: without the impulse the colour is rn(colour * atten) everywhere, the ball
    included (fp16 storage: that fp32 product rounded once more, RNE); with it the run differs inside the ball only.  The staged kernels'
    results are also held bit for bit against the gather kernels' (ADVECT_LDS = 0) for either setting of the switch"""
    select(knob, kernel)
    X, Y, Z = dims
    vel = np.zeros((3, Z, Y, X), f32)
    _, col = rand_fields(dims, 223, half=storage == "fp16")
    v0, c0, dt = advect_once(dims, vel, col, 0, storage=storage)
    atten = np.maximum(er.fma(-dt, f32(0.200000003), f32(1.0)), f32(0.0))
    assert same_bits(c0, stored((col * atten).astype(f32), storage))
    assert not v0.any()
    v1, c1, _ = advect_once(dims, vel, col, 1, storage=storage)
    far = ball_far(dims)
    assert same_bits(v1[:, far], v0[:, far]) and same_bits(c1[far], c0[far])
    assert not same_bits(v1[:, ~far], v0[:, ~far]) and not same_bits(c1[~far], c0[~far])
    if kernel in STAGED:
        knob("ADVECT_LDS", "0")
        for impulse, (v, c) in ((0, (v0, c0)), (1, (v1, c1))):
            gv, gc, _ = advect_once(dims, vel, col, impulse, storage=storage)
            assert same_bits(gv, v) and same_bits(gc, c), impulse


@pytest.mark.parametrize("kernel,dims,storage", RANDOM_CASES)
def test_switch_only_acts_inside_the_ball(kernel, dims, storage, knob):
    select(knob, kernel)
    vel, col = rand_fields(dims, 227, half=storage == "fp16", scale=3.0)
    vel[:, :, : dims[1] // 2] *= f32(0.05)               # half of the rows trace less than a cell, the others far: every path of the staged kernels
    vel = stored(vel, storage)
    v0, c0, _ = advect_once(dims, vel, col, 0, storage=storage)
    v1, c1, _ = advect_once(dims, vel, col, 1, storage=storage)
    far = ball_far(dims)
    assert same_bits(v1[:, far], v0[:, far]) and same_bits(c1[far], c0[far])
    if er.support(dims, er.BUILTIN_3D if dims[2] > 1 else er.BUILTIN_2D).any():      # (150, 150, 6) and (130, 130, 4): no plane cuts the ball
        assert not same_bits(v1, v0) and not same_bits(c1, c0)
    if kernel in STAGED:                                  # ... and the staged kernels = the gather kernels, switch off and on
        knob("ADVECT_LDS", "0")
        for impulse, (v, c) in ((0, (v0, c0)), (1, (v1, c1))):
            gv, gc, _ = advect_once(dims, vel, col, impulse, storage=storage)
            assert same_bits(gv, v) and same_bits(gc, c), impulse


# ---- 4: order and overlap -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(70, 70, 5), (36, 36, 1)])
def test_overlapping_emitters_apply_in_list_order(dims):
    A = er.emitter((0.45, 0.5, 0.5), 0.2, color_rate=(300.0, 20.0, 0.0, 500.0), force=(50.0, -20.0, 10.0), swirl=30.0)
    B = er.emitter((0.6, 0.55, 0.5), 0.25, color_rate=(5.0, 400.0, 100.0, 0.5), force=(-70.0, 90.0, 0.0), swirl=-120.0)
    vel, col = rand_fields(dims, 229)
    f = make(dims)
    dt = f32(f.default_time_step())
    f.UpdateFrame(dt, 0)
    res = {}
    for order in ((A, B), (B, A)):
        f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
        f.SetEmitters(list(order))
        f.Emit()
        whole = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
        f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
        for e in order:
            f.SetEmitters([e])
            f.Emit()
        split = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
        assert same_bits(whole[0], split[0]) and same_bits(whole[1], split[1])
        assert whole[1].max() == 1.0                                 # the rates saturate
        res[order[0] is A] = whole
    assert not same_bits(res[True][1], res[False][1])                # ... so the order matters, and each list kept its own


@pytest.mark.parametrize("dims", [(32, 32, 32), (36, 36, 1)])
def test_sixteen_emitters_on_one_cell(dims):
    rng = np.random.default_rng(234)
    ems = [er.emitter((0.5 + 0.1 * rng.standard_normal(), 0.5 + 0.1 * rng.standard_normal(), 0.5 + 0.1 * rng.standard_normal()), 0.3 + 0.02 * k,
                      color_rate=(0.1 * k, 0.3, 0.02 * k, 0.2), force=(3.0 * k - 20.0, 5.0, 11.0 - k), swirl=15.0 - 2 * k) for k in range(16)]
    X, Y, Z = dims
    centre = (Z // 2, Y // 2, X // 2)
    assert all(er.support(dims, e)[centre] for e in ems)
    vel, col = rand_fields(dims, 239)
    f = make(dims)
    dt = f32(f.default_time_step())
    f.Release()
    check_against_model(dims, "fp32", vel, col * f32(0.25), ems, dt)


# ---- 5: nothing set is nothing changed -------------------------------------------------------------------------------------------------
def run_digests(dims, mode, touch):
    f = make(dims, jacobi_iters=12, jacobi_mode=mode)
    if touch:
        f.SetEmitters(six()); f.SetImpulse(0)
        f.SetEmitters(None); f.SetImpulse(1)
        assert f.GetEmitters() == []
    dt = f32(f.default_time_step())
    for k in range(8):
        f.UpdateFrame(dt, k % 3)
        f.Simulate(k % 3)
        if touch:
            f.Emit()                                                  # an empty list: nothing
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS]
    f.Release()
    return out


@pytest.mark.parametrize("mode", ["fixed", "faithful"])
@pytest.mark.parametrize("dims", [(70, 70, 5), (64, 64, 16)])
def test_nothing_set_is_nothing_changed(dims, mode):
    assert run_digests(dims, mode, False) == run_digests(dims, mode, True)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_empty_list_and_zero_time_step_leave_the_bits_alone(storage):
    dims = (70, 70, 5)
    vel, col = rand_fields(dims, 241, half=storage == "fp16")
    vel[0, 0, 0, 0] = f32(-0.0)                                     # a value the arithmetic would not give back
    f = make(dims, storage=storage)
    f.UpdateFrame(f32(0.1), 0)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
    f.Emit()                                                          # no list
    assert same_bits(f.download(fx.FIELD_VELOCITY1), vel) and same_bits(f.download(fx.FIELD_COLOR), col)
    f.SetEmitters(six())
    f.UpdateFrame(0.0, 1)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
    f.Emit()                                                          # dt = 0
    assert same_bits(f.download(fx.FIELD_VELOCITY1), vel) and same_bits(f.download(fx.FIELD_COLOR), col)
    f.UpdateFrame(f32(0.1), 2)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
    f.Emit()
    assert not same_bits(f.download(fx.FIELD_COLOR), col)


# ---- 6: whole steps -------------------------------------------------------------------------------------------------------------------------
def run_steps(dims, staged, state, eps, emitters, **kw):
    vel, col = state
    f = make(dims, **kw)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetImpulse(0)
    f.SetEmitters(emitters)
    if eps:
        f.SetVorticityConfinement(eps)
    dt = f32(f.default_time_step())
    for i in range(4):
        f.UpdateFrame(dt, i % 3)
        if staged:
            f.Advect(); f.Emit()
            if eps:
                f.ConfineVorticity()
            f.Divergence(); f.Jacobi(kw["jacobi_iters"]); f.Project()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    out = [f.download(k) for k in (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE)]
    f.Release()
    return out


def same_all(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("eps", [0.0, 8.0])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(32, 32, 32), (70, 70, 5)])
def test_simulate_is_the_stage_composition(dims, storage, eps):
    state = rand_fields(dims, 251, half=storage == "fp16", scale=0.2)
    ems = six()[:4]
    kw = dict(storage=storage, jacobi_iters=10, jacobi_mode="fixed")
    whole = run_steps(dims, False, state, eps, ems, **kw)
    assert same_all(whole, run_steps(dims, True, state, eps, ems, **kw))
    assert not same_all(whole, run_steps(dims, False, state, eps, None, **kw))       # (and the pass took part)


def test_simulate_is_the_stage_composition_faithful():
    """FX_JACOBI_FAITHFUL: the dense sweep's fused divergence reads the velocity the emitters have added to"""
    dims = (32, 32, 32)
    state = rand_fields(dims, 257, scale=0.2)
    kw = dict(jacobi_iters=16, jacobi_mode="faithful")
    whole = run_steps(dims, False, state, 0.0, six()[:4], **kw)
    assert same_all(whole, run_steps(dims, True, state, 0.0, six()[:4], **kw))
    assert not same_all(whole, run_steps(dims, False, state, 0.0, None, **kw))


# ---- 7: the render's alpha side volume ------------------------------------------------------------------------------------------------
def rendered_rounds(accel):
    vp = (160, 120)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], (32, 32, 32), jacobi_iters=10)
    f.SetMaxSamples(48, 16)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    f.SetImpulse(0)
    f.SetEmitters([er.emitter((0.5, 0.8, 0.45), 0.12, force=(0.0, -60.0, 0.0), swirl=50.0)])      # high in the volume: the built-in never puts smoke there
    view, proj, eye = fx.default_camera(*vp)
    dt = f32(f.default_time_step())
    for k in range(3):                                               # from the second step on the advection writes the alpha volume
        f.UpdateFrame(dt, k, view, proj, eye)
        f.Simulate(k)
        f.ClearRenderTarget()
        f.Render(k, fx.Fluid.OPTIMIZED)
        f.RenderCube(k)
    f.Synchronize()
    out = f.download(fx.FIELD_CUBEMAP), f.download(fx.FIELD_TARGET)
    f.Release()
    return out


def test_emitted_smoke_reaches_the_accelerated_render():
    cube1, target1 = rendered_rounds(1)
    cube0, target0 = rendered_rounds(0)
    assert cube0[..., 3].max() > 0                                   # the cube map is not empty
    assert np.array_equal(cube1, cube0) and np.array_equal(target1, target0)


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------------
def c_emitter(**kw):
    e = capi.Emitter()
    e.struct_size = kw.pop("struct_size", 56)
    e.flags = kw.pop("flags", 0)
    e.center = (0.5, 0.5, 0.5)
    e.radius = 0.1
    e.color_rate = (1.0, 2.0, 3.0, 4.0)
    e.force = (0.0, 10.0, 0.0)
    e.swirl = 5.0
    for k, v in kw.items():
        if isinstance(v, tuple):                                     # (index, value) of an array member
            a = getattr(e, k)
            a[v[0]] = v[1]
        else:
            setattr(e, k, v)
    return e


def test_status_codes():
    import ctypes as C
    lib = capi.load()
    f = make((32, 32, 32))
    good = [er.emitter((0.25, 0.5, 0.75), 0.125, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, 6.0, 7.0), swirl=8.0)]
    f.SetEmitters(good)
    assert f.GetEmitters() == [dict(good[0], flags=0)]

    def one(e, count=1):
        arr = (capi.Emitter * 17)()
        for k in range(17):
            arr[k] = e
        return lib.fx_set_emitters(f._ctx, arr, count)
    nan, inf = float("nan"), float("inf")
    bad = [c_emitter(struct_size=52), c_emitter(struct_size=0), c_emitter(flags=1), c_emitter(flags=0x80000000), c_emitter(radius=0.0),
           c_emitter(radius=-0.1), c_emitter(radius=nan), c_emitter(radius=inf), c_emitter(swirl=nan), c_emitter(swirl=-inf)]
    bad += [c_emitter(center=(a, v)) for a in range(3) for v in (nan, inf)] + [c_emitter(force=(a, v)) for a in range(3) for v in (nan, -inf)]
    bad += [c_emitter(color_rate=(i, v)) for i in range(4) for v in (-1.0, -1e-30, nan, inf)]
    for e in bad:
        assert one(e) == capi.FX_E_INVALID
        assert f.GetEmitters() == [dict(good[0], flags=0)]           # the previous list stays in force
    assert one(c_emitter(), 17) == capi.FX_E_INVALID and f.GetEmitters() == [dict(good[0], flags=0)]
    assert lib.fx_set_emitters(f._ctx, None, 1) == capi.FX_E_INVALID
    assert lib.fx_set_emitters(None, None, 0) == capi.FX_E_INVALID and lib.fx_set_impulse(None, 0) == capi.FX_E_INVALID
    assert lib.fx_emit(None, None) == capi.FX_E_INVALID
    n = C.c_uint32(99)
    assert lib.fx_get_emitters(None, None, 0, C.byref(n)) == capi.FX_E_INVALID and lib.fx_get_emitters(f._ctx, None, 0, None) == capi.FX_E_INVALID
    assert lib.fx_get_emitters(f._ctx, None, 0, C.byref(n)) == capi.FX_OK and n.value == 1         # the length alone
    assert one(c_emitter(), 16) == capi.FX_OK and len(f.GetEmitters()) == 16
    assert one(c_emitter(center=(1, 40.0)), 2) == capi.FX_OK                                        # a centre outside the volume is allowed
    assert lib.fx_set_emitters(f._ctx, None, 0) == capi.FX_OK and f.GetEmitters() == []
    with pytest.raises(fx.FluidxError):
        f.SetEmitters([er.emitter((0.5, 0.5, 0.5), -1.0)])

    # slab ranks: a lone slab context, and the members of an in-process group
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    arr = (capi.Emitter * 1)(c_emitter())
    for r in ranks:
        assert lib.fx_set_emitters(r._ctx, arr, 1) == capi.FX_E_INVALID and lib.fx_set_impulse(r._ctx, 0) == capi.FX_E_INVALID
    fx.comm_init_local(ranks)
    for r in ranks:
        assert lib.fx_set_emitters(r._ctx, arr, 1) == capi.FX_E_INVALID and lib.fx_set_impulse(r._ctx, 0) == capi.FX_E_INVALID
        assert lib.fx_emit(r._ctx, None) == capi.FX_E_INVALID
        assert lib.fx_set_impulse(r._ctx, 1) == capi.FX_OK           # the default may be restated
        assert lib.fx_get_emitters(r._ctx, None, 0, C.byref(n)) == capi.FX_OK and n.value == 0

    ro = fx.Fluid()
    assert ro.Init(64, 64, (32, 32, 32), render_only=True)
    assert lib.fx_set_emitters(ro._ctx, arr, 1) == capi.FX_E_STATE and lib.fx_set_emitters(ro._ctx, None, 0) == capi.FX_E_STATE
    assert lib.fx_get_emitters(ro._ctx, None, 0, C.byref(n)) == capi.FX_E_STATE
    assert lib.fx_set_impulse(ro._ctx, 0) == capi.FX_E_STATE and lib.fx_set_impulse(ro._ctx, 1) == capi.FX_E_STATE
    assert lib.fx_emit(ro._ctx, None) == capi.FX_E_STATE
    # ... whatever else is wrong with the call
    assert lib.fx_set_emitters(ro._ctx, arr, 17) == capi.FX_E_STATE and lib.fx_set_emitters(ro._ctx, None, 3) == capi.FX_E_STATE
    assert lib.fx_get_emitters(ro._ctx, None, 4, None) == capi.FX_E_STATE
    for o in [f, ro] + ranks:
        o.Release()


def test_configuration_survives_update_frame_and_is_not_digested():
    dims = (32, 32, 32)
    f = make(dims)
    f.SetEmitters(six()[:2]); f.SetImpulse(0)
    before = [f.digest(k) for k in ALL_FIELDS]
    f.UpdateFrame(f32(0.05), 0)
    assert len(f.GetEmitters()) == 2
    assert sorted(before) == sorted(f.digest(k) for k in ALL_FIELDS)
    f.Release()
