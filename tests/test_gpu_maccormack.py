"""MacCormack advection on the GPU (fx_set_advection_scheme / fx_advect, csrc/fx_maccormack.hip: k_mc_predict, k_mc_correct).

Against the numpy model tests/maccormack_ref.py there are two criteria, and no other tolerance in this file:
  * outside the built-in impulse ball's support -- everywhere with fx_set_impulse(0) -- the stage equals the model bit for bit, velocity and colour;
  * inside, rel-L2 < 1e-6 -- the project's figure for exp2 in fp32 against float64 (tests/test_gpu_emitters.py; the model evaluates the basis in
    float64, the device in fp32).
The comparison with the impulse on asserts first that no cell's basis lies within relative 1e-5 of the threshold e^-4.  Everything else here is bit
for bit or a digest: fx_simulate against the stage calls, the untouched default, the resume and the two render paths; the blob and the step edge
carry the bounds tests/test_maccormack_ref.py holds the model to."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import buoyancy_ref as br
import emitter_ref as er
import maccormack_ref as mr
from test_gpu_buoyancy import rand_state, time_step, rel_l2, same_bits, masks, make, ALL_FIELDS

pytestmark = pytest.mark.gpu
f32 = np.float32

# rows shorter than a tile; a ragged second x tile and fewer planes than a tile column; a power of two; 150-cell rows; the tuned row length; 2-D
SHAPES = [(20, 20, 12), (70, 70, 5), (64, 64, 16), (150, 150, 6), (256, 256, 6), (36, 36, 1), (64, 64, 1)]
MC, SL = capi.ADVECT_MACCORMACK, capi.ADVECT_SEMI_LAGRANGIAN


def advect(f, vel0, col, dt):
    """one fx_advect on context f from (vel0, col): (VELOCITY1, COLOR) behind it"""
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)      # (UpdateFrame flips the parity: the advection reads this colour)
    f.UpdateFrame(dt, 0)
    f.Advect()
    f.Synchronize()
    assert same_bits(f.download(fx.FIELD_VELOCITY), vel0) and same_bits(f.download(fx.FIELD_COLOR_PREV), col)      # inputs only
    return f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)


# ---- 1: the stage against the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", SHAPES)
def test_stage_matches_the_model(dims, storage, address):
    """velocities that carry a trace two cells per axis (standard deviation; six at the tails): traces cross several cells and leave the box on
    every side"""
    half = storage == "fp16"
    _, vel0, _, col = rand_state(dims, 809, half=half, cells=2.0)
    dt = time_step(dims)
    X, Y, Z = dims
    p = br.cell_centres(dims)
    for a, n in enumerate(dims):                                          # the premise: every wall is crossed by a back-trace and by a forward trace
        if n > 1:
            for sign in (-1.0, 1.0):
                t = (p[a].astype(np.float64) + sign * vel0[a].astype(np.float64) * float(dt)) * n - 0.5
                assert (t < -1).any() and (t > n).any(), (a, sign)
    f = make(dims, storage=storage, advect_address=address)
    f.SetAdvectionScheme(MC)
    u, c = mr.corrected(vel0, col, dt, address)

    # the impulse off: bit for bit everywhere
    f.SetImpulse(0)
    gv, gc = advect(f, vel0, col, dt)
    wv, wc = mr.tail(u, c, dt, impulse=False, half=half)
    assert not same_bits(gc, mr.step(vel0, col, dt, address, impulse=False, half=half, scheme="semi-lagrangian")[1])      # not the other scheme
    assert same_bits(gv, wv) and same_bits(gc, wc)

    # three consecutive calls, each from the previous one's output: the model applied three times
    for k in range(2):
        gv, gc = advect(f, gv, gc, dt)
        wv, wc = mr.step(wv, wc, dt, address, impulse=False, half=half)
        assert same_bits(gv, wv) and same_bits(gc, wc), k

    # the impulse on: bit for bit outside the ball's support, rel-L2 inside
    assert mr.near_threshold(dims) == 0                               # the precondition: nothing is excluded
    f.SetImpulse(1)
    gv, gc = advect(f, vel0, col, dt)
    f.Release()
    wv, wc = mr.tail(u, c, dt, impulse=True, half=half)
    m = mr.impulse_support(dims)
    assert (m.any() or Z == 6) and not m.all()                        # (six planes: no cell centre within 1/16 of z = 0.5, the ball is empty)
    assert same_bits(gv[:, ~m], wv[:, ~m]) and same_bits(gc[~m], wc[~m])
    assert Z == 6 or not same_bits(gc, mr.tail(u, c, dt, impulse=False, half=half)[1])      # the impulse added something
    ev, ec = rel_l2(gv[:, m], wv[:, m]), rel_l2(gc[m], wc[m])
    print("%s %s %s: in-support rel-L2 velocity %.3g colour %.3g (%d cells)" % (dims, storage, address, ev, ec, int(m.sum())))
    assert ev < 1e-6 and ec < 1e-6, (ev, ec)


# ---- 2: signed zeros ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_signed_zeros_and_empty_regions(storage, address):
    """taps of -0 and +0 mixed with values of both signs, and regions where the colour is all +0 or all -0: the selects of rules 1 and 4 decide
    the sign of a zero result, bit for bit"""
    dims = (40, 40, 6)
    X, Y, Z = dims
    half = storage == "fp16"
    _, vel0, _, _ = rand_state(dims, 811, half=half, cells=1.5)
    rng = np.random.default_rng(821)
    pick = rng.integers(0, 4, (Z, Y, X, 4))
    col = np.choose(pick, [np.full(pick.shape, f32(-0.0)), np.zeros(pick.shape, f32), rng.random(pick.shape).astype(f32), -rng.random(pick.shape).astype(f32)]).astype(f32)
    col[:, :8, :20] = f32(0.0)
    col[:, 24:, 20:] = f32(-0.0)
    pickv = rng.integers(0, 3, vel0.shape)
    vel0 = np.choose(pickv, [np.full(vel0.shape, f32(-0.0)), np.zeros(vel0.shape, f32), vel0]).astype(f32)
    if half:
        col = col.astype(np.float16).astype(f32)
    f = make(dims, storage=storage, advect_address=address)
    f.SetAdvectionScheme(MC)
    f.SetImpulse(0)
    gv, gc = advect(f, vel0, col, time_step(dims))
    f.Release()
    wv, wc = mr.step(vel0, col, time_step(dims), address, impulse=False, half=half)
    neg = np.signbit(wc) & (wc == 0)
    assert neg.any() and (~np.signbit(wc) & (wc == 0)).any()           # both zeros occur in the result
    assert same_bits(gv, wv) and same_bits(gc, wc)


# ---- 3: fx_simulate is the composition of the stage calls ---------------------------------------------------------------------------------------
def run_steps(dims, staged, extra, **kw):
    _, vel0, _, col = rand_state(dims, 823, half=kw.get("storage") == "fp16", cells=0.3)
    f = make(dims, **kw)
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)
    f.SetAdvectionScheme(MC)
    if extra == "emitter":
        f.SetEmitters([er.emitter((0.5, 0.3, 0.5), 0.2, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, 20.0, -3.0), swirl=30.0)])
    elif extra == "obstacle":
        f.SetObstacles(masks(dims)["ball"])
    elif extra == "buoyancy":
        f.SetBuoyancy(**br.params(ambient=0.25, density_weight=0.7, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2)))
        f.SetHeatSources(br.list_a()[:3])
    elif extra == "open wall":
        f.SetOpenWalls(capi.WALL_Y_HI)
    elif extra == "confinement":
        f.SetVorticityConfinement(4.0)
    dt = time_step(dims)
    for i in range(4):
        f.UpdateFrame(dt, i % 3)
        if staged:
            f.Advect(); f.OpenInflow(); f.Emit(); f.Heat(); f.EnforceObstacles(); f.ConfineVorticity()
            f.Divergence(); f.Jacobi(kw["jacobi_iters"]); f.Project()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS]
    if extra == "buoyancy":
        out.append(f.download(fx.FIELD_TEMPERATURE).tobytes())
    f.Release()
    return out


FIXED, FAITHFUL = ((32, 32, 32), dict(jacobi_mode="fixed", jacobi_iters=10)), ((64, 64, 16), dict(jacobi_mode="faithful", jacobi_iters=16))


# (fx_set_obstacles and fx_set_open_walls refuse FX_JACOBI_FAITHFUL contexts: those two run in fixed mode)
@pytest.mark.parametrize("case,storage,extra", [(FIXED, "fp32", None), (FIXED, "fp16", None), (FAITHFUL, "fp32", None), (FAITHFUL, "fp16", None),
                                                (FAITHFUL, "fp32", "emitter"), (FIXED, "fp16", "obstacle"), (FAITHFUL, "fp16", "buoyancy"),
                                                (FIXED, "fp32", "open wall"), (FIXED, "fp32", "confinement")])
def test_simulate_is_the_stage_composition(case, storage, extra):
    dims, kw = case
    whole = run_steps(dims, False, extra, storage=storage, **kw)
    assert whole == run_steps(dims, True, extra, storage=storage, **kw)


# ---- 4: off means off ---------------------------------------------------------------------------------------------------------------------------
def run_default(dims, mode, touch):
    f = make(dims, jacobi_iters=12, jacobi_mode=mode)
    assert f.GetAdvectionScheme() == SL
    if touch:
        f.SetAdvectionScheme("maccormack")
        assert f.GetAdvectionScheme() == MC
        f.UpdateFrame(time_step(dims), 0)
        assert f.GetAdvectionScheme() == MC                               # configuration: kept across fx_update_frame
        f.SetAdvectionScheme(MC)                                          # (again: nothing new is allocated)
        f.SetAdvectionScheme("semi-lagrangian")
        assert f.GetAdvectionScheme() == SL
    else:
        f.UpdateFrame(time_step(dims), 0)                                 # (the same parity history)
    dt = time_step(dims)
    for k in range(6):
        f.UpdateFrame(dt, k % 3)
        f.Simulate(k % 3)
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS]
    f.Release()
    return out


@pytest.mark.parametrize("dims,mode", [((70, 70, 5), "fixed"), ((64, 64, 16), "faithful")])
def test_off_means_off(dims, mode):
    assert run_default(dims, mode, False) == run_default(dims, mode, True)


def test_the_scheme_changes_the_step():
    """... and on means on: the same six steps with the scheme set end elsewhere"""
    dims = (32, 32, 32)
    out = []
    for scheme in (SL, MC):
        f = make(dims, jacobi_iters=12)
        f.SetAdvectionScheme(scheme)
        for k in range(6):
            f.UpdateFrame(time_step(dims), k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
        out.append([f.digest(k) for k in ALL_FIELDS])
        f.Release()
    assert out[0][0] != out[1][0] and out[0][2] != out[1][2]


# ---- 5: what the scheme is for, on the device -------------------------------------------------------------------------------------------------
def carry_on_device(q, dims, scheme, steps=mr.CARRY_STEPS):
    """q in all four colour channels, carried `steps` fx_advect calls by the uniform velocity: the alpha channel, all four checked equal"""
    f = make(dims)
    f.SetImpulse(0)
    f.SetAdvectionScheme(scheme)
    f.upload(fx.FIELD_VELOCITY, mr.uniform_velocity(dims))
    f.upload(fx.FIELD_COLOR, np.repeat(q[..., None], 4, axis=-1))
    for k in range(steps):
        f.UpdateFrame(mr.CARRY_DT, k % 3)
        f.Advect()
    f.Synchronize()
    col = f.download(fx.FIELD_COLOR)
    f.Release()
    for i in range(3):
        assert same_bits(col[..., i], col[..., 3])
    return col[..., 3]


def test_a_carried_blob_keeps_its_peak_on_the_device():
    """the 32 x 32 x 8 run of tests/test_maccormack_ref.py through fx_advect, with the step's attenuation (linear, and the limiter is
    scale-invariant: the ratio of the peaks is the model's)"""
    dims = mr.CARRY_DIMS[0]
    q = mr.blob(dims)
    mc, sl = carry_on_device(q, dims, MC), carry_on_device(q, dims, SL)
    want, u0, at = q, mr.uniform_velocity(dims), mr.attenuation(mr.CARRY_DT)
    for _ in range(mr.CARRY_STEPS):
        want = mr.advect_field(want, u0, mr.CARRY_DT) * at
    print("peak %.4f -> semi-Lagrangian %.4f, MacCormack %.4f (ratio %.2f), minimum %.3g" % (q.max(), sl.max(), mc.max(), mc.max() / sl.max(), mc.min()))
    assert same_bits(mc, want)
    assert mc.max() >= 1.5 * sl.max()
    assert mc.min() >= 0


def test_a_step_edge_stays_within_its_bounds_on_the_device():
    dims = mr.CARRY_DIMS[0]
    mc = carry_on_device(mr.edge(dims), dims, MC)
    at = mr.attenuation(mr.CARRY_DT)
    print("edge after %d steps: [%.3g, %.6f], attenuation %.6f" % (mr.CARRY_STEPS, mc.min(), mc.max(), at))
    assert mc.min() >= 0 and mc.max() <= at
    one = carry_on_device(mr.edge(dims), dims, MC, steps=1)
    assert one.min() >= 0 and one.max() <= at and one.max() > 0


# ---- 6: the render ------------------------------------------------------------------------------------------------------------------------------
def rendered_rounds(accel):
    vp = (160, 120)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], (32, 32, 32), jacobi_iters=10)
    f.SetMaxSamples(48, 16)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    f.SetAdvectionScheme(MC)
    view, proj, eye = fx.default_camera(*vp)
    dt = time_step((32, 32, 32))
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


def test_accelerated_render_equals_the_plain_one_after_maccormack_steps():
    cube1, target1 = rendered_rounds(1)
    cube0, target0 = rendered_rounds(0)
    assert cube0[..., 3].max() > 0                                   # the cube map is not empty
    assert np.array_equal(cube1, cube0) and np.array_equal(target1, target0)


# ---- 7: resume ----------------------------------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_identically(tmp_path):
    dims = (32, 32, 32)
    path = str(tmp_path / "maccormack.fxck")

    def steps(f, first, count):
        dt = time_step(dims)
        for k in range(first, first + count):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
    a = make(dims, jacobi_iters=10)
    a.SetAdvectionScheme(MC)
    steps(a, 0, 3)
    a.SaveCheckpoint(path)
    steps(a, 3, 3)
    b = make(dims, jacobi_iters=10)
    b.LoadCheckpoint(path)
    assert b.GetAdvectionScheme() == SL                               # configuration is not stored
    b.SetAdvectionScheme(MC)
    steps(b, 3, 3)
    assert [a.digest(k) for k in ALL_FIELDS] == [b.digest(k) for k in ALL_FIELDS]
    c = make(dims, jacobi_iters=10)                                  # ... and the scheme matters to those steps
    c.LoadCheckpoint(path)
    steps(c, 3, 3)
    assert c.digest(fx.FIELD_VELOCITY) != a.digest(fx.FIELD_VELOCITY)
    for f in (a, b, c):
        f.Release()


# ---- 8: refusals and state codes ----------------------------------------------------------------------------------------------------------------
def test_status_codes():
    lib = capi.load()
    dims = (32, 32, 32)
    f = make(dims)
    got = C.c_uint32(77)
    assert lib.fx_get_advection_scheme(f._ctx, C.byref(got)) == capi.FX_OK and got.value == SL
    assert lib.fx_get_advection_scheme(f._ctx, None) == capi.FX_E_INVALID
    for scheme in (MC, SL):
        for bad in (2, 3, 0x80000000, 0xFFFFFFFF):
            assert lib.fx_set_advection_scheme(f._ctx, scheme) == capi.FX_OK
            assert lib.fx_set_advection_scheme(f._ctx, bad) == capi.FX_E_INVALID
            assert f.GetAdvectionScheme() == scheme                       # the previous setting stays in force
    with pytest.raises(ValueError):
        f.SetAdvectionScheme("bfecc")

    # slab ranks: a lone slab context, and the members of an in-process group
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, dims, slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)

    def slab_refusals(r):
        assert lib.fx_set_advection_scheme(r._ctx, MC) == capi.FX_E_INVALID and lib.fx_set_advection_scheme(r._ctx, SL) == capi.FX_E_INVALID
        assert r.GetAdvectionScheme() == SL                               # (slab ranks may ask)
    for r in ranks:
        slab_refusals(r)
    fx.comm_init_local(ranks)
    ranks[0].UpdateFrame(time_step(dims), 0)                             # (the driver's call: every member's frame)
    for r in ranks:
        slab_refusals(r)
        assert lib.fx_advect(r._ctx, None) == capi.FX_E_INVALID          # the stage call of a rank of a chain, as ever

    ro = fx.Fluid()
    assert ro.Init(64, 64, dims, render_only=True)
    assert lib.fx_set_advection_scheme(ro._ctx, MC) == capi.FX_E_STATE and lib.fx_set_advection_scheme(ro._ctx, SL) == capi.FX_E_STATE
    assert lib.fx_set_advection_scheme(ro._ctx, 9) == capi.FX_E_STATE   # ... whatever else is wrong with the call
    assert lib.fx_get_advection_scheme(ro._ctx, C.byref(got)) == capi.FX_E_STATE
    assert lib.fx_advect(ro._ctx, None) == capi.FX_E_STATE
    for o in [f, ro] + ranks:
        o.Release()
