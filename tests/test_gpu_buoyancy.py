"""Buoyancy on the GPU (fx_set_buoyancy / fx_set_heat_sources / fx_heat, csrc/fx_heat.hip: k_heat).

Against the numpy model tests/buoyancy_ref.py there are two criteria, and no other tolerance in this file:
  * outside every heat source's support the stage equals the model bit for bit, temperature and every VELOCITY1 component;
  * inside, rel-L2 < 1e-6 for the temperature and for the velocity -- the project's figure for exp2 in fp32 against float64
    (tests/test_gpu_emitters.py; the model evaluates the basis in float64, the device in fp32).
Every comparison asserts first that no cell of its inputs has a basis within relative 1e-5 of the threshold e^-4 (the cap on excluded
cells is zero).  Everything else here is bit for bit: the temperature against the colour advection's alpha (the link to the kernels the
oracle pins), fx_simulate against the stage calls, the untouched default, the resume and the two render paths."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import buoyancy_ref as br
import emitter_ref as er
from test_gpu_emitters import SIX

pytestmark = pytest.mark.gpu
f32 = np.float32

SHAPES = br.SHAPES
assert br.SIX == SIX                                                 # the source places are those of tests/test_gpu_emitters.py
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
PRM = br.params(ambient=0.25, density_weight=0.7, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2))


list_a, list_b = br.list_a, br.list_b


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status        # simulation only: no viewport
    return f


def time_step(dims):
    return f32((2.0 if dims[2] > 1 else 1.0) / dims[1])   # Fluid.default_time_step


def rand_state(dims, seed, half=False, cells=1.0):
    """velocity[0] scaled so that |u| dt N has a standard deviation of `cells` cells per axis (about three cells at the tails: some traces
    leave the walls), a VELOCITY1 with -0 entries, a colour in [0, 1) and a temperature around the ambient value"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    dt = time_step(dims)
    vel0 = rng.standard_normal((3, Z, Y, X))
    for a, n in enumerate(dims):
        vel0[a] *= cells / (float(dt) * n)
    vel0 = vel0.astype(f32)
    vel1 = rng.standard_normal((3, Z, Y, X)).astype(f32)
    vel1[:, 0, 0, : min(X, 5)] = f32(-0.0)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    T = (rng.random((Z, Y, X)) * 4 - 1).astype(f32)
    if half:
        vel0, vel1, col = (a.astype(np.float16).astype(f32) for a in (vel0, vel1, col))
    return T, vel0, vel1, col


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.sqrt((b ** 2).sum())
    d = np.sqrt(((a - b) ** 2).sum())
    return d / n if n > 0 else d


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def stage(f, state, prm, sources, dt):
    """one fx_heat on context f from `state`: (temperature, VELOCITY1) behind it"""
    T, vel0, vel1, col = state
    f.SetBuoyancy(**prm)
    f.SetHeatSources(sources)
    f.UpdateFrame(dt, 0)
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_VELOCITY1, vel1); f.upload(fx.FIELD_COLOR, col); f.upload(fx.FIELD_TEMPERATURE, T)
    f.Heat()
    f.Synchronize()
    assert same_bits(f.download(fx.FIELD_VELOCITY), vel0) and same_bits(f.download(fx.FIELD_COLOR), col)      # inputs only
    return f.download(fx.FIELD_TEMPERATURE), f.download(fx.FIELD_VELOCITY1)


# ---- 1: the temperature is advected like the colour ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", SHAPES)
def test_temperature_is_advected_like_the_colour(dims, storage, address):
    """ambient 0 and the advection's own attenuation constant as the cooling: T1 = Ts * atten, the colour advection's alpha operation for
    operation.  The colour advection is held to the oracle by tests/test_gpu_sim.py / tests/test_gpu_stage_matrix.py"""
    _, vel0, _, col = rand_state(dims, 401, half=storage == "fp16")
    f = make(dims, storage=storage, advect_address=address)
    f.SetImpulse(0)
    f.SetBuoyancy(ambient=0.0, cooling=float(f32(0.2)))
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)      # (UpdateFrame flips the parity: the advection reads this colour)
    f.UpdateFrame(time_step(dims), 0)
    f.upload(fx.FIELD_TEMPERATURE, col[..., 3])
    f.Advect()
    f.Heat()
    f.Synchronize()
    T, alpha = f.download(fx.FIELD_TEMPERATURE), f.download(fx.FIELD_COLOR)[..., 3]
    f.Release()
    assert alpha.any() and not same_bits(alpha, col[..., 3])
    if storage == "fp16":
        T = T.astype(np.float16).astype(f32)
    assert same_bits(T, alpha)


# ---- 2: the stage against the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", SHAPES)
def test_stage_matches_the_model(dims, storage, address):
    half = storage == "fp16"
    state = rand_state(dims, 409, half=half)
    T, vel0, vel1, col = state
    dt = time_step(dims)
    A, B = list_a(), list_b()
    assert br.near_threshold(dims, B) == 0                            # the precondition (A is a subset of B): nothing is excluded
    f = make(dims, storage=storage, advect_address=address)

    # list A: bit for bit outside the supports, rel-L2 inside
    gt, gv = stage(f, state, PRM, A, dt)
    wt, wv = br.apply(T, vel0, vel1, col, PRM, A, dt, address, half=half)
    m = br.supports(dims, A)
    assert m.any() and not m.all()
    assert same_bits(gt[~m], wt[~m]) and same_bits(gv[:, ~m], wv[:, ~m])
    et, ev = rel_l2(gt[m], wt[m]), rel_l2(gv[:, m], wv[:, m])
    print("%s %s %s: list A in-support rel-L2 temperature %.3g velocity %.3g (%d cells)" % (dims, storage, address, et, ev, int(m.sum())))
    assert not same_bits(gt, T) and not same_bits(gv, vel1)           # the pass changed something
    assert et < 1e-6 and ev < 1e-6, (et, ev)

    # list B: every cell is inside the fifth source
    gt, gv = stage(f, state, PRM, B, dt)
    wt, wv = br.apply(T, vel0, vel1, col, PRM, B, dt, address, half=half)
    assert br.supports(dims, B).all()
    et, ev = rel_l2(gt, wt), rel_l2(gv, wv)
    print("%s %s %s: list B rel-L2 temperature %.3g velocity %.3g" % (dims, storage, address, et, ev))
    assert et < 1e-6 and ev < 1e-6, (et, ev)

    # no sources: the whole stage bit for bit; with the default `up`, x and z keep their bits (the -0 entries included)
    gt, gv = stage(f, state, PRM, [], dt)
    wt, wv = br.apply(T, vel0, vel1, col, PRM, [], dt, address, half=half)
    assert same_bits(gt, wt) and same_bits(gv, wv) and not same_bits(gv, vel1)
    if dims[2] == 1:
        assert same_bits(gv[2], vel1[2])
    prm = dict(PRM, up=(0.0, 1.0, 0.0))
    gt, gv = stage(f, state, prm, [], dt)
    wt, wv = br.apply(T, vel0, vel1, col, prm, [], dt, address, half=half)
    assert same_bits(gt, wt) and same_bits(gv, wv)
    assert same_bits(gv[0], vel1[0]) and same_bits(gv[2], vel1[2]) and not same_bits(gv[1], vel1[1])
    f.Release()


# ---- 3: obstacles --------------------------------------------------------------------------------------------------------------------------
def masks(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    ball = ((x + .5) / X - .45) ** 2 + ((y + .5) / Y - .55) ** 2 + ((z + .5) / Z - .5) ** 2 <= 0.3 ** 2
    return {"ball": ball.astype(np.uint8), "random": (np.random.default_rng(419).random((Z, Y, X)) < 0.3).astype(np.uint8)}


@pytest.mark.parametrize("kind", ["ball", "random"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(20, 20, 12), (64, 64, 8)])
def test_solid_cells_hold_ambient_and_keep_their_velocity(dims, storage, kind):
    half = storage == "fp16"
    state = rand_state(dims, 421, half=half)
    T, vel0, vel1, col = state
    dt = time_step(dims)
    solid = masks(dims)[kind]
    s = solid != 0
    assert s.any() and not s.all()
    A = list_a()
    assert br.near_threshold(dims, A) == 0
    f = make(dims, storage=storage)
    f.SetObstacles(solid)
    gt, gv = stage(f, state, PRM, A, dt)
    f.Release()
    assert same_bits(gt[s], np.full(int(s.sum()), f32(PRM["ambient"]))) and same_bits(gv[:, s], vel1[:, s])
    wt, wv = br.apply(T, vel0, vel1, col, PRM, A, dt, half=half, solid=solid)
    m = br.supports(dims, A)
    out, ins = ~m & ~s, m & ~s
    assert out.any() and ins.any()
    assert same_bits(gt[out], wt[out]) and same_bits(gv[:, out], wv[:, out]) and not same_bits(gv[:, out], vel1[:, out])
    et, ev = rel_l2(gt[ins], wt[ins]), rel_l2(gv[:, ins], wv[:, ins])
    assert et < 1e-6 and ev < 1e-6, (et, ev)


# ---- 4: fx_simulate is the composition of the stage calls -------------------------------------------------------------------------------
def run_steps(dims, staged, obstacle, **kw):
    _, vel0, _, col = rand_state(dims, 431, half=kw.get("storage") == "fp16", cells=0.3)
    f = make(dims, **kw)
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)
    f.SetImpulse(0)
    f.SetEmitters([er.emitter((0.5, 0.3, 0.5), 0.2, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, 20.0, -3.0), swirl=30.0)])
    f.SetVorticityConfinement(4.0)
    if obstacle:
        f.SetObstacles(masks(dims)["ball"])
    f.SetBuoyancy(**PRM)
    f.SetHeatSources(list_a()[:3])
    dt = time_step(dims)
    for i in range(4):
        f.UpdateFrame(dt, i % 3)
        if staged:
            f.Advect(); f.Emit(); f.Heat(); f.EnforceObstacles(); f.ConfineVorticity()
            f.Divergence(); f.Jacobi(kw["jacobi_iters"]); f.Project()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS], f.download(fx.FIELD_TEMPERATURE)
    f.Release()
    return out


# (fx_set_obstacles refuses FX_JACOBI_FAITHFUL contexts: the faithful case runs with the emitter and the confinement)
@pytest.mark.parametrize("dims,obstacle,kw", [((32, 32, 32), True, dict(jacobi_mode="fixed", jacobi_iters=10)),
                                              ((32, 32, 32), False, dict(jacobi_mode="faithful", jacobi_iters=16)),
                                              ((70, 70, 5), True, dict(storage="fp16", jacobi_iters=10)),
                                              ((36, 36, 1), True, dict(jacobi_iters=10))])
def test_simulate_is_the_stage_composition(dims, obstacle, kw):
    whole, T_whole = run_steps(dims, False, obstacle, **kw)
    parts, T_parts = run_steps(dims, True, obstacle, **kw)
    assert whole == parts and same_bits(T_whole, T_parts)
    assert not same_bits(T_whole, np.full(T_whole.shape, f32(PRM["ambient"])))


# ---- 5: off means off -------------------------------------------------------------------------------------------------------------------------
def run_off(dims, mode, how):
    f = make(dims, jacobi_iters=12, jacobi_mode=mode)
    if how == "detached":
        f.SetBuoyancy(**PRM); f.SetHeatSources(list_a())
        assert f.GetBuoyancy() is not None
        f.SetBuoyancy(None); f.SetHeatSources(None)
        assert f.GetBuoyancy() is None and f.GetHeatSources() == []
    elif how == "sources only":
        f.SetHeatSources(list_b())
    dt = time_step(dims)
    for k in range(6):
        f.UpdateFrame(dt, k % 3)
        f.Simulate(k % 3)
        if how != "never":
            f.Heat()                                                  # buoyancy is off: nothing
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS]
    assert f._lib.fx_field_bytes(f._ctx, fx.FIELD_TEMPERATURE) == 0
    f.Release()
    return out


@pytest.mark.parametrize("dims,mode", [((70, 70, 5), "fixed"), ((64, 64, 16), "faithful")])
def test_off_means_off(dims, mode):
    never = run_off(dims, mode, "never")
    assert never == run_off(dims, mode, "detached") == run_off(dims, mode, "sources only")


# ---- 6: physics, signs only -------------------------------------------------------------------------------------------------------------------
def mean_along_up(up, prm, sources, emitters):
    dims = (24, 24, 24)
    f = make(dims, jacobi_iters=20)
    f.SetImpulse(0)
    f.SetBuoyancy(**dict(prm, up=up))
    f.SetHeatSources(sources)
    f.SetEmitters(emitters)
    dt = time_step(dims)
    for k in range(8):
        f.UpdateFrame(dt, k % 3)
        f.Simulate(k % 3)
    f.Synchronize()
    vel = f.download(fx.FIELD_VELOCITY)
    f.Release()
    m = er.support(dims, er.emitter((0.5, 0.5, 0.5), 0.2))
    assert m.any()
    return float(sum(float(up[a]) * vel[a][m].astype(np.float64).mean() for a in range(3)))


def test_hot_smoke_rises_and_dense_smoke_sinks():
    hot = [br.source((0.5, 0.5, 0.5), 0.2, 40.0)]
    for up in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0)):
        assert mean_along_up(up, br.params(lift=4.0), hot, None) > 0, up
    smoke = [er.emitter((0.5, 0.5, 0.5), 0.2, color_rate=(5.0, 5.0, 5.0, 30.0), force=(0.0, 0.0, 0.0), swirl=0.0)]
    assert mean_along_up((0.0, 1.0, 0.0), br.params(density_weight=6.0), [], smoke) < 0


# ---- 7: resume ----------------------------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_identically(tmp_path):
    dims = (32, 32, 32)
    path = str(tmp_path / "buoyant.fxck")
    prm, src = br.params(ambient=0.1, density_weight=0.5, lift=2.0, cooling=0.3), list_a()[:2]

    def steps(f, first, count):
        dt = time_step(dims)
        for k in range(first, first + count):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
    a = make(dims, jacobi_iters=10)
    a.SetBuoyancy(**prm); a.SetHeatSources(src)
    steps(a, 0, 3)
    a.SaveCheckpoint(path)
    T = a.download(fx.FIELD_TEMPERATURE)
    assert not same_bits(T, np.full(T.shape, f32(0.1)))
    steps(a, 3, 3)
    b = make(dims, jacobi_iters=10)
    b.LoadCheckpoint(path)
    assert b.GetBuoyancy() is None and b.GetHeatSources() == []      # configuration is not stored
    b.SetBuoyancy(**prm); b.SetHeatSources(src)
    b.upload(fx.FIELD_TEMPERATURE, T)
    steps(b, 3, 3)
    assert [a.digest(k) for k in ALL_FIELDS] == [b.digest(k) for k in ALL_FIELDS]      # all six: every one is a function of the restored state by now
    assert same_bits(a.download(fx.FIELD_TEMPERATURE), b.download(fx.FIELD_TEMPERATURE))
    c = make(dims, jacobi_iters=10)                                  # ... and the temperature matters to those steps
    c.LoadCheckpoint(path)
    c.SetBuoyancy(**prm); c.SetHeatSources(src)
    steps(c, 3, 3)
    assert c.digest(fx.FIELD_VELOCITY) != a.digest(fx.FIELD_VELOCITY)
    for f in (a, b, c):
        f.Release()


# ---- 8: the render ----------------------------------------------------------------------------------------------------------------------------
def rendered_rounds(accel):
    vp = (160, 120)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], (32, 32, 32), jacobi_iters=10)
    f.SetMaxSamples(48, 16)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    f.SetBuoyancy(lift=3.0, density_weight=0.5, cooling=0.2)
    f.SetHeatSources([br.source((0.5, 0.1, 0.5), 1 / 16, 40.0)])
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


def test_accelerated_render_equals_the_plain_one_after_buoyant_steps():
    cube1, target1 = rendered_rounds(1)
    cube0, target0 = rendered_rounds(0)
    assert cube0[..., 3].max() > 0                                   # the cube map is not empty
    assert np.array_equal(cube1, cube0) and np.array_equal(target1, target0)


# ---- 9: refusals and state codes ----------------------------------------------------------------------------------------------------------
def c_buoyancy(**kw):
    b = capi.Buoyancy()
    b.struct_size = kw.pop("struct_size", 36)
    b.flags = kw.pop("flags", 0)
    b.ambient, b.density_weight, b.lift, b.cooling = 0.5, 0.25, 2.0, 0.125
    b.up = (0.0, 1.0, 0.0)
    for k, v in kw.items():
        if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], int):      # (index, value) of an array member
            getattr(b, k)[v[0]] = v[1]
        else:
            setattr(b, k, v)
    return b


def c_source(**kw):
    e = capi.HeatSource()
    e.struct_size = kw.pop("struct_size", 28)
    e.flags = kw.pop("flags", 0)
    e.center = (0.5, 0.5, 0.5)
    e.radius = 0.25
    e.rate = 3.0
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(e, k)[v[0]] = v[1]
        else:
            setattr(e, k, v)
    return e


def test_status_codes():
    lib = capi.load()
    dims = (32, 32, 32)
    f = make(dims)
    cells = 32 * 32 * 32
    buf = np.zeros(cells, f32)

    def temperature_calls(ctx):
        return (lib.fx_upload(ctx, fx.FIELD_TEMPERATURE, buf.ctypes.data, buf.nbytes), lib.fx_download(ctx, fx.FIELD_TEMPERATURE, buf.ctypes.data, buf.nbytes),
                lib.fx_field_bytes(ctx, fx.FIELD_TEMPERATURE))
    # off (the default): the field does not exist
    assert f.GetBuoyancy() is None and f.GetHeatSources() == []
    assert temperature_calls(f._ctx) == (capi.FX_E_STATE, capi.FX_E_STATE, 0)
    assert lib.fx_heat(f._ctx, None) == capi.FX_OK

    good = dict(ambient=0.5, density_weight=0.25, lift=2.0, cooling=0.125, up=(0.0, 1.0, 0.0), flags=0)
    assert lib.fx_set_buoyancy(f._ctx, C.byref(c_buoyancy())) == capi.FX_OK and f.GetBuoyancy() == good
    assert temperature_calls(f._ctx) == (capi.FX_OK, capi.FX_OK, 4 * cells)
    T = f.download(fx.FIELD_TEMPERATURE)
    assert T.shape == (32, 32, 32) and not T.any()                   # (the upload above wrote zeros)
    nan, inf = float("nan"), float("inf")
    bad = [c_buoyancy(struct_size=32), c_buoyancy(struct_size=0), c_buoyancy(flags=1), c_buoyancy(flags=0x80000000),
           c_buoyancy(density_weight=-1.0), c_buoyancy(density_weight=-1e-30), c_buoyancy(cooling=-0.5), c_buoyancy(up=(1, 0.0))]
    bad += [c_buoyancy(**{k: v}) for k in ("ambient", "density_weight", "lift", "cooling") for v in (nan, inf, -inf)]
    bad += [c_buoyancy(up=(a, v)) for a in range(3) for v in (nan, inf)]
    for b in bad:
        assert lib.fx_set_buoyancy(f._ctx, C.byref(b)) == capi.FX_E_INVALID
        assert f.GetBuoyancy() == good                               # the previous setting stays in force
    assert lib.fx_set_buoyancy(f._ctx, C.byref(c_buoyancy(lift=-3.0, ambient=-2.0, up=(1, -1.0)))) == capi.FX_OK      # a negative lift, ambient or up is legal
    assert f.GetBuoyancy() == dict(good, lift=-3.0, ambient=-2.0, up=(0.0, -1.0, 0.0))
    assert not f.download(fx.FIELD_TEMPERATURE).any()                # a later call keeps the field (it is not refilled with the new ambient)
    on = C.c_int(5)
    assert lib.fx_get_buoyancy(f._ctx, None, C.byref(on)) == capi.FX_OK and on.value == 1
    assert lib.fx_get_buoyancy(f._ctx, None, None) == capi.FX_OK
    # the first call fills the field with the ambient value
    f.SetBuoyancy(None)
    assert f.GetBuoyancy() is None and temperature_calls(f._ctx) == (capi.FX_E_STATE, capi.FX_E_STATE, 0)
    f.SetBuoyancy(ambient=1.5)
    assert same_bits(f.download(fx.FIELD_TEMPERATURE), np.full((32, 32, 32), f32(1.5)))
    assert lib.fx_upload(f._ctx, fx.FIELD_TEMPERATURE, buf.ctypes.data, buf.nbytes - 4) == capi.FX_E_INVALID
    out = (C.c_uint64 * 2)()
    assert lib.fx_field_digest(f._ctx, fx.FIELD_TEMPERATURE, 0, 0, out) != capi.FX_OK      # not a digested field

    # heat sources
    src = [br.source((0.25, 0.5, 0.75), 0.125, -6.0)]
    f.SetHeatSources(src)
    kept = [dict(src[0], flags=0)]
    assert f.GetHeatSources() == kept

    def one(e, count=1):
        arr = (capi.HeatSource * 17)()
        for k in range(17):
            arr[k] = e
        return lib.fx_set_heat_sources(f._ctx, arr, count)
    bad = [c_source(struct_size=24), c_source(struct_size=0), c_source(flags=1), c_source(flags=0x80000000), c_source(radius=0.0),
           c_source(radius=-0.1), c_source(radius=nan), c_source(radius=inf), c_source(rate=nan), c_source(rate=-inf)]
    bad += [c_source(center=(a, v)) for a in range(3) for v in (nan, inf)]
    for e in bad:
        assert one(e) == capi.FX_E_INVALID
        assert f.GetHeatSources() == kept
    assert one(c_source(), 17) == capi.FX_E_INVALID and f.GetHeatSources() == kept
    assert lib.fx_set_heat_sources(f._ctx, None, 1) == capi.FX_E_INVALID and f.GetHeatSources() == kept
    n = C.c_uint32(99)
    assert lib.fx_get_heat_sources(f._ctx, None, 0, None) == capi.FX_E_INVALID
    assert lib.fx_get_heat_sources(f._ctx, None, 0, C.byref(n)) == capi.FX_OK and n.value == 1
    assert one(c_source(), 16) == capi.FX_OK and len(f.GetHeatSources()) == 16
    assert one(c_source(center=(1, 40.0), rate=-1.0), 2) == capi.FX_OK      # a centre outside the volume and a cold source are allowed
    f.SetBuoyancy(None)
    assert len(f.GetHeatSources()) == 2                              # the list may stand while buoyancy is off
    assert lib.fx_set_heat_sources(f._ctx, None, 0) == capi.FX_OK and f.GetHeatSources() == []

    # slab ranks: a lone slab context, and the members of an in-process group
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, dims, slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    bu, arr = c_buoyancy(), (capi.HeatSource * 1)(c_source())

    def slab_refusals(r):
        assert lib.fx_set_buoyancy(r._ctx, C.byref(bu)) == capi.FX_E_INVALID and lib.fx_set_buoyancy(r._ctx, None) == capi.FX_E_INVALID
        assert lib.fx_set_heat_sources(r._ctx, arr, 1) == capi.FX_E_INVALID and lib.fx_heat(r._ctx, None) == capi.FX_E_INVALID
        assert r.GetBuoyancy() is None and r.GetHeatSources() == []
        assert temperature_calls(r._ctx)[2] == 0
    for r in ranks:
        slab_refusals(r)
    fx.comm_init_local(ranks)
    for r in ranks:
        slab_refusals(r)

    ro = fx.Fluid()
    assert ro.Init(64, 64, dims, render_only=True)
    assert lib.fx_set_buoyancy(ro._ctx, C.byref(bu)) == capi.FX_E_STATE and lib.fx_set_buoyancy(ro._ctx, None) == capi.FX_E_STATE
    assert lib.fx_get_buoyancy(ro._ctx, None, C.byref(on)) == capi.FX_E_STATE
    assert lib.fx_set_heat_sources(ro._ctx, arr, 1) == capi.FX_E_STATE and lib.fx_set_heat_sources(ro._ctx, None, 0) == capi.FX_E_STATE
    assert lib.fx_get_heat_sources(ro._ctx, None, 0, C.byref(n)) == capi.FX_E_STATE
    assert lib.fx_heat(ro._ctx, None) == capi.FX_E_STATE
    # ... whatever else is wrong with the call
    assert lib.fx_set_buoyancy(ro._ctx, C.byref(c_buoyancy(struct_size=3))) == capi.FX_E_STATE and lib.fx_set_heat_sources(ro._ctx, arr, 17) == capi.FX_E_STATE
    assert temperature_calls(ro._ctx) == (capi.FX_E_STATE, capi.FX_E_STATE, 0)
    for o in [f, ro] + ranks:
        o.Release()


def test_configuration_survives_update_frame_and_is_not_digested():
    dims = (32, 32, 32)
    f = make(dims)
    before = [f.digest(k) for k in ALL_FIELDS]
    f.SetBuoyancy(**PRM); f.SetHeatSources(list_a())
    f.UpdateFrame(f32(0.05), 0)
    assert f.GetBuoyancy() == dict({k: float(f32(v)) for k, v in PRM.items() if k != "up"}, up=tuple(float(f32(v)) for v in PRM["up"]), flags=0)
    assert len(f.GetHeatSources()) == 5
    assert sorted(before) == sorted(f.digest(k) for k in ALL_FIELDS)
    f.Release()
