"""Solid obstacles on the GPU (fx_set_obstacles / fx_get_obstacles / fx_enforce_obstacles, csrc/fx_obstacle.hip).

Everything here is bit for bit -- the stages against the C++ reference tests/obstacle_ref/ (tests/test_obstacle_ref.py anchors it to the oracle),
an all-fluid mask against no mask, the wide sweep against the scalar one, fx_simulate against the stage calls, detach, the accelerated render
against the plain one, a checkpoint resume -- with one exception: the rollout against the reference's whole step, whose advection is the
oracle's.  The device's advection is held to the oracle's at rel-L2 1e-6 per step and bit for bit only away from the impulse ball (its exp2
is the device's own; tests/test_gpu_sim.py), so that comparison uses the project's rollout criterion, rel-L2 < 1e-4 (test_gpu_sim.py TOL),
over its 4 steps, while the same test feeds the DEVICE's advected fields through the reference's enforce, divergence, sweeps and projection
and compares those bit for bit.

Shapes (X = Y, Z): the smallest at which each kernel can go wrong -- (20, 5) scalar with a row shorter than a tile, (150, 6) scalar 3-D with
X % 4 != 0, (36, 1) and (150, 1) 2-D, (64, 8) the wide sweep, (68, 5) with a partial wave, (256, 6) one wave per row, (320, 4) wave seams
inside a row."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import test_obstacle_ref as ob
from test_obstacle_ref import RefSim, ball_mask, plate_mask, random_mask, ref_divergence, ref_enforce, ref_jacobi, ref_project, ref_codes

pytestmark = pytest.mark.gpu
f32 = np.float32

SCALAR = [(20, 20, 5), (150, 150, 6), (36, 36, 1), (150, 150, 1)]
V4 = [(64, 64, 8), (68, 68, 5), (256, 256, 6), (320, 320, 4)]
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
TOL = 1e-4          # tests/test_gpu_sim.py: fields within 1e-4 rel-L2 of the reference replay


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status        # simulation only: no viewport
    return f


def masks(dims):
    X, Y, Z = dims
    one = np.zeros((Z, Y, X), np.uint8)
    one[Z // 2, Y // 3, (2 * X) // 3] = 1
    return {"random": random_mask(dims), "ball": ball_mask(dims), "single": one, "solid": np.ones((Z, Y, X), np.uint8),
            "fluid": np.zeros((Z, Y, X), np.uint8)}


def rand_state(dims, seed, half=False, scale=0.5):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vel = (rng.standard_normal((3, Z, Y, X)) * scale).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    if half:
        vel, col = vel.astype(np.float16).astype(f32), col.astype(np.float16).astype(f32)
    return vel, col, p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_all(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.sqrt((b ** 2).sum())
    d = np.sqrt(((a - b) ** 2).sum())
    return d / n if n > 0 else d


# ---- 1: the stages against the reference ------------------------------------------------------------------------------------------------
def stages(f, vel, col, p, sweeps=5):
    """uploads the state, runs enforce, divergence, `sweeps` sweeps and the projection -> (velocity1, colour, b, pressure, velocity)"""
    f.UpdateFrame(f32(f.default_time_step()), 0)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col); f.upload(fx.FIELD_PRESSURE, p)
    f.EnforceObstacles()
    v1, c1 = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.Divergence()
    b = f.download(fx.FIELD_DIVERGENCE)
    f.Jacobi(sweeps)
    q = f.download(fx.FIELD_PRESSURE)
    f.Project()
    return v1, c1, b, q, f.download(fx.FIELD_VELOCITY)


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", SCALAR + V4)
def test_stages_match_the_reference_bit_for_bit(dims, storage):
    half = storage == "fp16"
    vel, col, p = rand_state(dims, 301, half)
    f = make(dims, storage=storage, jacobi_iters=5)
    for name, m in masks(dims).items():
        f.SetObstacles(m)
        got_mask, cells = f.GetObstacles()
        assert np.array_equal(got_mask, m) and cells == int(m.sum()), name
        v1, c1, b, q, out = stages(f, vel, col, p)
        wv, wc = ref_enforce(vel, col, m)
        assert same_bits(v1, wv) and same_bits(c1, wc), name
        wb = ref_divergence(wv, m)
        assert same_bits(b, wb), name
        wq = ref_jacobi(p, wb, m, 5)
        assert same_bits(q, wq), name
        assert same_bits(out, ref_project(wv, wq, m, half)), name
        if name in ("random", "ball"):                                # the mask took part in every stage
            none = np.zeros_like(m)
            assert not same_bits(b, ref_divergence(vel, none)) and not same_bits(q, ref_jacobi(p, wb, none, 5))
    f.Release()


def test_the_mask_may_be_device_memory():
    import torch
    dims = (64, 64, 8)
    m = random_mask(dims, seed=5)
    vel, col, p = rand_state(dims, 303)
    a, b = make(dims, jacobi_iters=5), make(dims, jacobi_iters=5)
    a.SetObstacles(m)
    b.SetObstacles(torch.from_numpy(m.astype(np.int32) * 7).to("cuda"))      # any non-zero value is solid
    assert np.array_equal(b.GetObstacles()[0], m) and b.GetObstacles()[1] == a.GetObstacles()[1] == int(m.sum())
    assert same_all(stages(a, vel, col, p), stages(b, vel, col, p))
    a.Release(); b.Release()


# ---- 2: an all-fluid mask is no mask ------------------------------------------------------------------------------------------------------
EMITTER = [{"center": (0.3, 0.6, 0.4), "radius": 0.11, "color_rate": (1.0, 3.0, 3.0, 2.0), "force": (-20.0, 30.0, 5.0), "swirl": 60.0}]


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(64, 64, 8), (150, 150, 6)])
def test_an_all_fluid_mask_is_no_mask(dims, storage, extras):
    X, Y, Z = dims
    vel, col, p = rand_state(dims, 307, storage == "fp16", scale=0.2)
    a, b = make(dims, storage=storage, jacobi_iters=10), make(dims, storage=storage, jacobi_iters=10)
    b.SetObstacles(np.zeros((Z, Y, X), np.uint8))
    assert b.GetObstacles()[1] == 0
    assert same_all(stages(a, vel, col, p), stages(b, vel, col, p))
    for f in (a, b):
        f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
        if extras:
            f.SetVorticityConfinement(4.0); f.SetEmitters(EMITTER)
        dt = f32(f.default_time_step())
        for k in range(6):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
    assert [a.digest(k) for k in ALL_FIELDS] == [b.digest(k) for k in ALL_FIELDS]
    a.Release(); b.Release()


# ---- 3: the wide sweep is the scalar sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", V4)
def test_the_wide_sweep_is_the_scalar_sweep(dims, knob):
    m = random_mask(dims, seed=17)
    _, _, p = rand_state(dims, 311)
    b = np.random.default_rng(313).standard_normal(p.shape).astype(f32)

    def sweeps():
        f = make(dims, jacobi_iters=7)
        f.SetObstacles(m)
        f.upload(fx.FIELD_PRESSURE, p); f.upload(fx.FIELD_DIVERGENCE, b)
        f.Jacobi(7)
        out = f.download(fx.FIELD_PRESSURE)
        f.Release()
        return out
    wide = sweeps()
    knob("OBSTACLE_V4", "0")                                          # (a lab switch: the contexts from here on run on the lab build)
    scalar = sweeps()
    want = ref_jacobi(p, b, m, 7)
    assert same_bits(wide, want) and same_bits(scalar, want)


# ---- 4: whole steps ---------------------------------------------------------------------------------------------------------------------------
def run_steps(dims, staged, mask, extras, steps=4, seed=337, **kw):
    """from a random state (on the thin grids here the built-in impulse reaches few cells or none: (64, 64, 8) has no cell centre within its radius)"""
    vel, col, _ = rand_state(dims, seed, kw.get("storage") == "fp16", scale=0.2)
    f = make(dims, **kw)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetObstacles(mask)
    if extras:
        f.SetVorticityConfinement(4.0); f.SetEmitters(EMITTER)
    dt = f32(f.default_time_step())
    for i in range(steps):
        f.UpdateFrame(dt, i % 3)
        if staged:
            f.Advect(); f.Emit(); f.EnforceObstacles(); f.ConfineVorticity()
            f.Divergence(); f.Jacobi(kw["jacobi_iters"]); f.Project()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    out = [f.download(k) for k in (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE)]
    f.Release()
    return out


def low_ball(dims):
    """a ball in the lower half of the box, in the way of the plume"""
    return ball_mask(dims, center=(0.5, 0.3, 0.5), radius=0.12)


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(64, 64, 8), (150, 150, 6), (36, 36, 1)])
def test_simulate_is_the_stage_composition(dims, storage, extras):
    m = low_ball(dims)
    kw = dict(storage=storage, jacobi_iters=10)
    whole = run_steps(dims, False, m, extras, **kw)
    assert same_all(whole, run_steps(dims, True, m, extras, **kw))
    assert not same_all(whole, run_steps(dims, False, None, extras, **kw))           # (and the obstacle took part)
    solid = m.astype(bool)
    assert not bits(whole[0])[:, solid].any() and not bits(whole[1])[solid].any()


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(64, 64, 8), (20, 20, 5), (36, 36, 1)])
def test_simulate_is_the_reference_step(dims, storage):
    X, Y, Z = dims
    half = storage == "fp16"
    m = low_ball(dims)
    assert m.any() and not m.all()
    vel, col, _ = rand_state(dims, 341, half, scale=0.2)
    r = RefSim(X, Y, Z, m, iters=10, half=half)
    r.s.vel[0][...] = vel; r.s.col[0][...] = col
    f = make(dims, storage=storage, jacobi_iters=10)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetObstacles(m)
    dt = f32(f.default_time_step())
    for k in range(4):
        r.step()
        f.UpdateFrame(dt, k % 3)
        if k < 3:
            f.Simulate(k % 3)
    # the last step by stages: the device's own advected fields through the reference's enforce, divergence, sweeps and projection, bit for bit
    p0 = f.download(fx.FIELD_PRESSURE)
    f.Advect()
    av, ac = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.EnforceObstacles(); f.Divergence(); f.Jacobi(10); f.Project()
    f.Synchronize()
    gv, gc, gp = f.download(fx.FIELD_VELOCITY), f.download(fx.FIELD_COLOR), f.download(fx.FIELD_PRESSURE)
    wv, wc = ref_enforce(av, ac, m)
    wq = ref_jacobi(p0, ref_divergence(wv, m), m, 10)
    assert same_bits(gc, wc) and same_bits(gp, wq) and same_bits(gv, ref_project(wv, wq, m, half))
    # ... and the whole rollout against the reference's, whose advection is the oracle's
    ev, ec, ep = rel_l2(gv, r.velocity), rel_l2(gc, r.color), rel_l2(gp, r.pressure)
    print("%s %s: rel-L2 velocity %.3g colour %.3g pressure %.3g" % (dims, storage, ev, ec, ep))
    assert r.color.max() > 0 and ev < TOL and ec < TOL and ep < TOL, (ev, ec, ep)
    f.Release()


# ---- 5: the seal ------------------------------------------------------------------------------------------------------------------------------
def test_a_plate_seals_the_far_half():
    """the plate and step count of tests/test_obstacle_ref.py::test_a_plate_seals_the_far_half, on the device"""
    X, Y, Z = dims = ob.SEAL_DIMS
    m = plate_mask(dims)
    far = slice(Y // 2 + 2, Y)
    runs = []
    for mask in (m, None):
        f = make(dims, jacobi_iters=ob.SEAL_ITERS)
        f.SetObstacles(mask)
        dt = f32(f.default_time_step())
        for k in range(ob.SEAL_STEPS):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
        runs.append((f.download(fx.FIELD_VELOCITY), f.download(fx.FIELD_COLOR)))
        f.Release()
    (pv, pc), (cv, cc) = runs
    assert cc[:, far].max() > 0 and np.abs(cv[:, :, far]).max() > 0                  # the control has smoke there
    assert not pv[:, :, far].any() and not pc[:, far].any()
    assert pc[:, :Y // 2].max() > 0
    solid = m.astype(bool)
    assert not bits(pv)[:, solid].any() and not bits(pc)[solid].any()                # +0, bit for bit
    beside = ~solid & ((ref_codes(m) & 0x0c) != 0)                                   # the fluid cells on either face of the plate
    assert beside.sum() == 2 * X * Z and not pv[1][beside].any()                     # no flow into or out of it
    assert pv[0][beside].any() and pv[2][beside].any()                               # ... but along it (free slip)


def test_normal_velocity_vanishes_beside_a_ball():
    dims = (64, 64, 8)
    m = low_ball(dims)
    v = run_steps(dims, False, m, True, steps=5, jacobi_iters=10)[0]
    code, fluid = ref_codes(m), ~m.astype(bool)
    for a in range(3):
        beside = fluid & ((code & (3 << (2 * a))) != 0)
        assert beside.any() and not v[a][beside].any()
        assert v[a][fluid & ~beside].any()


# ---- 6: detach ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(64, 64, 8), (36, 36, 1)])
def test_detach_returns_to_the_plain_kernels(dims):
    vel, col, _ = rand_state(dims, 317, scale=0.2)
    a, b = make(dims, jacobi_iters=10), make(dims, jacobi_iters=10)
    b.SetObstacles(low_ball(dims))
    b.SetObstacles(None)
    assert b.GetObstacles()[1] == 0 and not b.GetObstacles()[0].any()
    for f in (a, b):
        f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
        dt = f32(f.default_time_step())
        for k in range(3):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
    assert [a.digest(k) for k in ALL_FIELDS] == [b.digest(k) for k in ALL_FIELDS]
    # set again: the spare volume is reused, and the mask is in force again
    b.SetObstacles(low_ball(dims))
    b.UpdateFrame(f32(b.default_time_step()), 0); b.Simulate(0)
    a.UpdateFrame(f32(a.default_time_step()), 0); a.Simulate(0)
    assert a.digest(fx.FIELD_VELOCITY) != b.digest(fx.FIELD_VELOCITY)
    a.Release(); b.Release()


# ---- 7: the render's alpha side volume ------------------------------------------------------------------------------------------------
def rendered_rounds(accel):
    vp = (160, 120)
    dims = (32, 32, 32)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], dims, jacobi_iters=10)
    f.SetMaxSamples(48, 16)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    f.SetObstacles(ball_mask(dims, center=(0.5, 0.22, 0.5), radius=0.1))           # in the plume, right above the built-in impulse
    view, proj, eye = fx.default_camera(*vp)
    dt = f32(f.default_time_step())
    for k in range(4):                                               # from the second step on the advection writes the alpha volume
        f.UpdateFrame(dt, k % 3, view, proj, eye)
        f.Simulate(k % 3)
        f.ClearRenderTarget()
        f.Render(k % 3, fx.Fluid.OPTIMIZED)
        f.RenderCube(k % 3)
    f.Synchronize()
    out = f.download(fx.FIELD_CUBEMAP), f.download(fx.FIELD_TARGET), f.download(fx.FIELD_COLOR)
    f.Release()
    return out


def test_the_accelerated_render_sees_the_enforced_colour():
    cube1, target1, col1 = rendered_rounds(1)
    cube0, target0, col0 = rendered_rounds(0)
    assert cube0[..., 3].max() > 0 and same_bits(col1, col0)
    solid = ball_mask((32, 32, 32), center=(0.5, 0.22, 0.5), radius=0.1).astype(bool)
    assert not bits(col0)[solid].any() and col0[~solid].max() > 0
    assert np.array_equal(cube1, cube0) and np.array_equal(target1, target0)


# ---- 8: status codes --------------------------------------------------------------------------------------------------------------------------
def test_status_codes():
    lib = capi.load()
    dims = (32, 32, 8)
    n = 32 * 32 * 8
    m = random_mask(dims, seed=23)
    f = make(dims, jacobi_iters=6)
    f.SetObstacles(m)
    ptr = m.ctypes.data

    def in_force():
        got, cells = f.GetObstacles()
        return np.array_equal(got, m) and cells == int(m.sum())
    assert in_force()
    other = np.ones_like(m)
    for bytes_, flags in ((n - 1, 0), (n + 1, 0), (0, 0), (n, 2), (n, 0x80000000), (n, 3)):
        assert lib.fx_set_obstacles(f._ctx, None, other.ctypes.data, bytes_, flags) == capi.FX_E_INVALID
        assert in_force()                                            # the previous mask stays in force
    assert lib.fx_set_obstacles(f._ctx, None, None, 0, 2) == capi.FX_E_INVALID and in_force()
    assert lib.fx_set_obstacles(None, None, ptr, n, 0) == capi.FX_E_INVALID
    assert lib.fx_get_obstacles(None, None, 0, None) == capi.FX_E_INVALID and lib.fx_enforce_obstacles(None, None) == capi.FX_E_INVALID
    cells = C.c_uint64(0)
    out = np.empty(n, np.uint8)
    assert lib.fx_get_obstacles(f._ctx, out.ctypes.data, n - 1, C.byref(cells)) == capi.FX_E_INVALID
    assert lib.fx_get_obstacles(f._ctx, None, 0, C.byref(cells)) == capi.FX_OK and cells.value == int(m.sum())       # the count alone
    assert lib.fx_get_obstacles(f._ctx, out.ctypes.data, n, None) == capi.FX_OK and np.array_equal(out.reshape(m.shape), m)
    assert lib.fx_get_obstacles(f._ctx, None, 0, None) == capi.FX_OK
    # timing: one sweep per launch with a mask
    f.timing_enable(True)
    f.UpdateFrame(f32(f.default_time_step()), 0)
    f.Simulate(0); f.Jacobi(9)
    f.Synchronize()
    t = f.timing_read()
    assert t.jacobi_launches == t.jacobi_sweeps == 6 + 9
    # NULL ignores `bytes`
    assert lib.fx_set_obstacles(f._ctx, None, None, 12345, 0) == capi.FX_OK and f.GetObstacles()[1] == 0
    # nothing to do: no obstacles, or dt = 0
    vel, col, _ = rand_state(dims, 331)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
    f.EnforceObstacles()
    assert same_bits(f.download(fx.FIELD_VELOCITY1), vel) and same_bits(f.download(fx.FIELD_COLOR), col)
    f.SetObstacles(m)
    f.UpdateFrame(0.0, 1)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
    f.EnforceObstacles()
    assert same_bits(f.download(fx.FIELD_VELOCITY1), vel) and same_bits(f.download(fx.FIELD_COLOR), col)
    # configuration: kept across UpdateFrame, not digested
    before = sorted(f.digest(k) for k in ALL_FIELDS)
    f.SetObstacles(other)
    f.UpdateFrame(f32(0.05), 2)
    assert f.GetObstacles()[1] == n and before == sorted(f.digest(k) for k in ALL_FIELDS)

    # faithful contexts
    fa = make(dims, jacobi_iters=16, jacobi_mode="faithful")
    assert lib.fx_set_obstacles(fa._ctx, None, ptr, n, 0) == capi.FX_E_INVALID and fa.GetObstacles()[1] == 0
    # slab ranks: a lone slab context, and the members of an in-process group
    ranks = []
    big = np.zeros((32, 32, 32), np.uint8)
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    for r in ranks:
        assert lib.fx_set_obstacles(r._ctx, None, big.ctypes.data, big.size, 0) == capi.FX_E_INVALID
        assert lib.fx_set_obstacles(r._ctx, None, big.ctypes.data, 32 * 32 * 12, 0) == capi.FX_E_INVALID
    fx.comm_init_local(ranks)
    for r in ranks:
        assert lib.fx_set_obstacles(r._ctx, None, big.ctypes.data, big.size, 0) == capi.FX_E_INVALID
        assert lib.fx_enforce_obstacles(r._ctx, None) == capi.FX_E_INVALID
        assert lib.fx_get_obstacles(r._ctx, None, 0, C.byref(cells)) == capi.FX_OK and cells.value == 0
    ro = fx.Fluid()
    assert ro.Init(64, 64, dims, render_only=True)
    assert lib.fx_set_obstacles(ro._ctx, None, ptr, n, 0) == capi.FX_E_STATE and lib.fx_set_obstacles(ro._ctx, None, None, 0, 0) == capi.FX_E_STATE
    assert lib.fx_set_obstacles(ro._ctx, None, ptr, n + 1, 9) == capi.FX_E_STATE             # ... whatever else is wrong with the call
    assert lib.fx_get_obstacles(ro._ctx, None, 0, C.byref(cells)) == capi.FX_E_STATE and lib.fx_enforce_obstacles(ro._ctx, None) == capi.FX_E_STATE
    with pytest.raises(fx.FluidxError):
        fa.SetObstacles(m)
    for o in [f, fa, ro] + ranks:
        o.Release()


# ---- 9: checkpoints ---------------------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_resume_continues_bit_identically(tmp_path):
    dims = (64, 64, 8)
    m = low_ball(dims)
    path = str(tmp_path / "obstacles.fxck")

    def steps(f, first, count):
        dt = f32(f.default_time_step())
        for k in range(first, first + count):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
    vel, col, _ = rand_state(dims, 347, scale=0.2)
    a = make(dims, jacobi_iters=10)
    a.upload(fx.FIELD_VELOCITY, vel); a.upload(fx.FIELD_COLOR, col)
    a.SetObstacles(m)
    steps(a, 0, 4)
    a.SaveCheckpoint(path)
    steps(a, 4, 3)
    b = make(dims, jacobi_iters=10)
    b.LoadCheckpoint(path)
    assert b.GetObstacles()[1] == 0                                  # configuration is not stored
    b.SetObstacles(m)
    steps(b, 4, 3)
    keep = (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE)
    assert [a.digest(k) for k in keep] == [b.digest(k) for k in keep]
    c = make(dims, jacobi_iters=10)                                  # ... and the mask matters to those steps
    c.LoadCheckpoint(path)
    steps(c, 4, 3)
    assert c.digest(fx.FIELD_VELOCITY) != a.digest(fx.FIELD_VELOCITY)
    c.Release()
    a.Release(); b.Release()
