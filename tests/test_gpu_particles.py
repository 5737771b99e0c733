"""Tracer particles and point queries on the GPU (fx_set_particles / fx_move_particles / fx_sample_velocity ..., csrc/fx_particles.hip).

Every comparison with the numpy model tests/particle_ref.py is bit for bit, every record: the rule has no transcendental.  Shapes (X = Y, Z):
(20, 12) rows that are no multiple of a wave, (70, 5) thin z, (36, 1) 2-D, (256, 6) a wide row; both storages; 1, 257 and 4099 records -- a
single one, one past a workgroup, a ragged tail.  The positions always carry the model's edge set: the walls, -0, the outermost cell
centres, a centre and a face inside, places beyond the box, +-inf, NaN and 1e30."""
import ctypes as C
import functools

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import particle_ref as pr

pytestmark = pytest.mark.gpu
f32 = np.float32

SHAPES, COUNTS = pr.SHAPES, pr.COUNTS
STORAGES = ["fp32", "fp16"]
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
DRIFT = (0.03, -0.4, 0.02)


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status        # simulation only: no viewport
    return f


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def velocity(dims, half):
    """one random velocity per shape and storage, about 1.5 cells per step, shared by the tests (never written to)"""
    v = pr.velocity(dims, 601, cells=1.5, half=half)
    v.setflags(write=False)
    return v


def uniform(dims, cells, signs=(1, 1, 1)):
    """the same velocity everywhere: `cells` cells per step along every axis, towards the walls `signs` names"""
    dt = float(pr.time_step(dims))
    v = np.empty((3, dims[2], dims[1], dims[0]), f32)
    for a, n in enumerate(dims):
        v[a] = signs[a] * cells / (dt * n)
    return v.astype(np.float16).astype(f32)                      # (representable in either storage)


def loaded(dims, storage, vel, **kw):
    f = make(dims, storage=storage, **kw)
    f.upload(fx.FIELD_VELOCITY, vel)
    f.UpdateFrame(pr.time_step(dims), 0)
    return f


# ---- 1: the point query ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES)
def test_sample_velocity_matches_the_model_bit_for_bit(dims, storage):
    vel = velocity(dims, storage == "fp16")
    f = loaded(dims, storage, vel)
    for n in COUNTS:
        pts = pr.points(dims, n, 611 + n)
        got = f.SampleVelocity(pts)
        assert same_bits(got, pr.sample(vel, pts)), n
        four = np.concatenate([pts, np.full((n, 1), np.nan, f32)], axis=1)          # w is not looked at
        assert same_bits(f.SampleVelocity(four), got), n
    edge = pr.edge_points(dims)                                                       # the wild points land where the clamp says
    wild = f.SampleVelocity(edge)
    with np.errstate(invalid="ignore"):
        assert same_bits(wild, f.SampleVelocity(pr.c01(edge))) and np.isfinite(wild).all()
    assert f.SampleVelocity(np.zeros((0, 4), f32)).shape == (0, 3)
    f.Release()


# ---- 2: the stage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["euler", "midpoint"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES)
def test_move_particles_matches_the_model_bit_for_bit(dims, storage, scheme):
    vel = velocity(dims, storage == "fp16")
    dt = pr.time_step(dims)
    lifetime = 0.5 + float(dt)                                                        # the older half of the records dies
    f = loaded(dims, storage, vel)
    f.SetParticleParams(scheme, DRIFT, lifetime)
    prm = pr.params(scheme=pr.MIDPOINT if scheme == "midpoint" else pr.EULER, drift=DRIFT, lifetime=lifetime)
    for n in COUNTS:
        rec = pr.records(dims, n, 621 + n)
        f.SetParticles(rec)
        assert same_bits(f.GetParticles(), rec)
        f.MoveParticles()
        got, want = f.GetParticles(), pr.move(rec, vel, dt, prm)
        assert same_bits(got, want), n
        with np.errstate(invalid="ignore"):
            dead_in = ~(rec[:, 3] >= 0)
        assert same_bits(got[dead_in], rec[dead_in])                                 # a dead record keeps every bit
        if n > 1:
            assert dead_in.any() and (got[~dead_in, 3] == -1).any() and (got[~dead_in, 3] > 0).any()
            assert not same_bits(got[~dead_in, :3], rec[~dead_in, :3])
        f.MoveParticles()                                                            # a second step, from the device's own records
        assert same_bits(f.GetParticles(), pr.move(want, vel, dt, prm)), n
    f.Release()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", [(20, 20, 12), (36, 36, 1)])
def test_wide_offset_kernels_match_the_model(dims, storage, knob):
    """WIDE_OFFSETS = 1 (a lab switch: the context runs on the lab build) makes the launchers take the WIDE = true instantiations of both
    kernels, which otherwise serve grids of 2^28 cells and more: 64-bit offsets are executed here, not driven beyond 2^32"""
    knob("WIDE_OFFSETS", "1")
    vel = velocity(dims, storage == "fp16")
    dt = pr.time_step(dims)
    f = loaded(dims, storage, vel)
    f.SetObstacles(pr.box_mask(dims))
    f.SetOpenWalls(pr.X_HI | pr.Y_LO)
    rec = pr.records(dims, 4099, 625)
    assert same_bits(f.SampleVelocity(rec), pr.sample(vel, rec))
    for scheme in ("euler", "midpoint"):
        f.SetParticleParams(scheme, DRIFT, 0.5 + float(dt))
        f.SetParticles(rec)
        f.MoveParticles()
        prm = pr.params(scheme=pr.MIDPOINT if scheme == "midpoint" else pr.EULER, drift=DRIFT, lifetime=0.5 + float(dt))
        assert same_bits(f.GetParticles(), pr.move(rec, vel, dt, prm, pr.X_HI | pr.Y_LO, pr.box_mask(dims))), scheme
    f.Release()


# ---- 3: walls -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES)
def test_a_closed_wall_holds_and_an_open_one_lets_go(dims, storage):
    n, dt, is3d = 4099, pr.time_step(dims), dims[2] > 1
    rec = pr.records(dims, n, 631)
    with np.errstate(invalid="ignore"):
        live = rec[:, 3] >= 0
        tame = live & (np.abs(rec[:, :3]) <= 2).all(axis=1)                          # (an infinite or huge start stays on its own side)
    # two box widths and more per step towards x+, y-, z+: all faces closed, every live record ends on those walls
    far = uniform(dims, 2.0 * max(dims), (1, -1, 1))
    f = loaded(dims, storage, far)
    for scheme in ("euler", "midpoint"):
        f.SetParticleParams(scheme)
        f.SetParticles(rec)
        f.MoveParticles()
        got = f.GetParticles()
        assert same_bits(got, pr.move(rec, far, dt, pr.params(scheme=pr.MIDPOINT if scheme == "midpoint" else pr.EULER)))
        assert tame.sum() > n // 2 and (got[tame, 0] == 1).all() and (got[tame, 1] == 0).all() and (not is3d or (got[tame, 2] == 1).all())
        assert (got[live, 3] >= 0).all()
    # three cells per step with x+ and y- open: exactly the model's records die
    near = uniform(dims, 3.0, (1, -1, 1))
    f.upload(fx.FIELD_VELOCITY, near)
    f.SetOpenWalls(pr.X_HI | pr.Y_LO)
    f.SetParticles(rec)
    f.MoveParticles()
    got, want = f.GetParticles(), pr.move(rec, near, dt, faces=pr.X_HI | pr.Y_LO)
    assert same_bits(got, want)
    died = live & (got[:, 3] == -1)
    assert died.any() and (live & ~died).any()
    closed = pr.move(rec, near, dt)
    assert same_bits(got[:, :3], closed[:, :3]) and not same_bits(got[:, 3], closed[:, 3])     # the walls decide who lives, not where
    f.Release()


# ---- 4: obstacles ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES)
def test_particles_do_not_enter_a_solid(dims, storage):
    n, dt = 4099, pr.time_step(dims)
    vel = velocity(dims, storage == "fp16")
    solid = pr.box_mask(dims)
    rec = pr.records(dims, n, 641)
    f = loaded(dims, storage, vel)
    f.SetObstacles(solid)
    want = pr.move(rec, vel, dt, solid=solid)
    free = pr.move(rec, vel, dt)
    with np.errstate(invalid="ignore"):
        live = rec[:, 3] >= 0
    stopped = live & (bits(want[:, :3]) != bits(free[:, :3])).any(axis=1)
    assert stopped.any() and same_bits(want[stopped, :3], rec[stopped, :3]) and (live & ~stopped).any()
    for bodies in ((), [dict(box_lo=(0.2, 0.2, 0.0), box_hi=(0.8, 0.8, 1.0), linear=(0.5, 0.0, 0.0), angular=(0.0, 0.0, 1.0))]):
        f.SetObstacleBodies(bodies)                                                  # a moving solid stops them the same way
        f.SetParticles(rec)
        f.MoveParticles()
        assert same_bits(f.GetParticles(), want), len(bodies)
    f.SetObstacles(None)
    f.SetParticles(rec)
    f.MoveParticles()
    assert same_bits(f.GetParticles(), free)
    f.Release()


# ---- 5, 6, 7: the step ----------------------------------------------------------------------------------------------------------------------
ITERS = 8


def run_steps(dims, storage, mode, steps=3):
    """mode: "whole" = fx_simulate with a set, "staged" = the stage calls and MoveParticles behind them, "never" = no set at all, "freed" = a
    set that was freed again before the first step -> (the six fields, the particles or None)"""
    half = storage == "fp16"
    vel = pr.velocity(dims, 651, cells=0.6, half=half)
    col = np.random.default_rng(653).random((dims[2], dims[1], dims[0], 4)).astype(f32)
    col = col.astype(np.float16).astype(f32) if half else col
    f = make(dims, storage=storage, jacobi_iters=ITERS)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetObstacles(pr.box_mask(dims))
    f.SetOpenWalls(pr.Y_HI | pr.X_LO)
    if mode != "never":
        f.SetParticles(pr.records(dims, 4099, 655))
        f.SetParticleParams("midpoint", DRIFT, 0.7)
    if mode == "freed":
        f.SetParticles(None)
        assert f.ParticlesDevice() == (0, 0) and f.GetParticles().shape == (0, 4)
    dt = pr.time_step(dims)
    for i in range(steps):
        f.UpdateFrame(dt, i % 3)
        if mode == "staged":
            f.Advect(); f.OpenInflow(); f.EnforceObstacles()
            f.Divergence(); f.Jacobi(ITERS); f.Project()
            f.MoveParticles()
        else:
            f.Simulate(i % 3)
    if mode in ("never", "freed"):
        f.MoveParticles()                                                            # nothing
    f.Synchronize()
    fields = [f.download(k) for k in ALL_FIELDS]
    digests = [f.digest(k) for k in ALL_FIELDS]
    part = f.GetParticles() if mode in ("whole", "staged") else None
    f.Release()
    return fields, digests, part


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", [(20, 20, 12), (36, 36, 1)])
def test_simulate_moves_the_particles_and_nothing_else(dims, storage):
    whole, dw, pw = run_steps(dims, storage, "whole")
    staged, ds, ps = run_steps(dims, storage, "staged")
    never, dn, _ = run_steps(dims, storage, "never")
    freed, df, _ = run_steps(dims, storage, "freed")
    # 5: fx_simulate with a set = the stage calls followed by MoveParticles
    assert same_bits(pw, ps) and dw == ds
    rec = pr.records(dims, 4099, 655)
    with np.errstate(invalid="ignore"):
        live = rec[:, 3] >= 0
    assert not same_bits(pw[live, :3], rec[live, :3]) and same_bits(pw[~live], rec[~live])
    # 6: particles are passive -- all six fields, bit for bit, with and without a set
    for a, b in zip(whole, never):
        assert same_bits(a, b)
    assert dw == dn
    # 7: a set that was freed is a set that never was
    for a, b in zip(freed, never):
        assert same_bits(a, b)
    assert df == dn


# ---- 8: the device path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_pointer_serves_the_point_query(storage):
    import torch
    dims, n = (20, 20, 12), 4099
    vel = velocity(dims, storage == "fp16")
    f = loaded(dims, storage, vel)
    rec = pr.records(dims, n, 661)
    f.SetParticles(rec)
    ptr, count = f.ParticlesDevice()
    assert ptr != 0 and ptr % 16 == 0 and count == n
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fp = C.POINTER(C.c_float)
    capi.check(capi.load().fx_sample_velocity(f._ctx, None, C.cast(ptr, fp), n, C.cast(out.data_ptr(), fp), capi.PARTICLES_DEVICE), "device query")
    f.Synchronize()
    torch.cuda.synchronize()
    host = f.SampleVelocity(rec)
    assert same_bits(out.cpu().numpy(), host) and same_bits(host, pr.sample(vel, rec))
    # ... and a device tensor replaces the set, and moves like the host copy
    t = torch.from_numpy(rec).to("cuda")
    f.SetParticles(t)
    assert same_bits(f.GetParticles(), rec)
    f.MoveParticles()
    assert same_bits(f.GetParticles(), pr.move(rec, vel, pr.time_step(dims)))
    lib = capi.load()
    assert lib.fx_sample_velocity(f._ctx, None, C.cast(ptr + 4, fp), 1, C.cast(out.data_ptr(), fp), capi.PARTICLES_DEVICE) == capi.FX_E_INVALID   # misaligned
    f.Release()


# ---- 9: the calls ---------------------------------------------------------------------------------------------------------------------------
def test_status_codes_and_round_trips():
    lib = capi.load()
    dims = (20, 20, 12)
    f = loaded(dims, "fp32", velocity(dims, False))
    fp = C.POINTER(C.c_float)
    n, p = C.c_uint32(99), C.c_void_p(5)
    default = dict(scheme="midpoint", drift=(0.0, 0.0, 0.0), lifetime=0.0, flags=0)
    # the defaults
    assert f.GetParticleParams() == default and f.ParticlesDevice() == (0, 0) and f.GetParticles().shape == (0, 4)
    assert lib.fx_get_particles(f._ctx, None, 0, C.byref(n)) == capi.FX_OK and n.value == 0
    assert lib.fx_move_particles(f._ctx, None) == capi.FX_OK
    # round trips
    rec = pr.records(dims, 257, 671)
    f.SetParticles(rec)
    ptr, count = f.ParticlesDevice()
    assert count == 257 and ptr and same_bits(f.GetParticles(), rec)
    part = np.zeros((10, 4), f32)
    assert lib.fx_get_particles(f._ctx, part.ctypes.data_as(fp), 10, C.byref(n)) == capi.FX_OK and n.value == 257 and same_bits(part, rec[:10])
    assert lib.fx_get_particles(f._ctx, None, 0, C.byref(n)) == capi.FX_OK and n.value == 257
    assert lib.fx_particles_device(f._ctx, None, None) == capi.FX_OK
    f.SetParticleParams("euler", (0.5, -0.25, 0.125), 3.0)
    mine = dict(scheme="euler", drift=(0.5, -0.25, 0.125), lifetime=3.0, flags=0)
    assert f.GetParticleParams() == mine
    # refused, the previous state staying in force
    r4 = rec.ctypes.data_as(fp)
    assert lib.fx_set_particles(f._ctx, None, None, 3, 0) == capi.FX_E_INVALID                       # a count with no pointer
    assert lib.fx_set_particles(f._ctx, None, r4, capi.MAX_PARTICLES + 1, 0) == capi.FX_E_INVALID
    assert lib.fx_set_particles(f._ctx, None, r4, 4, 2) == capi.FX_E_INVALID and lib.fx_set_particles(f._ctx, None, r4, 4, 0x80000001) == capi.FX_E_INVALID
    assert f.ParticlesDevice() == (ptr, 257) and same_bits(f.GetParticles(), rec)
    assert lib.fx_get_particles(f._ctx, None, 4, C.byref(n)) == capi.FX_E_INVALID and lib.fx_get_particles(f._ctx, r4, 4, None) == capi.FX_E_INVALID
    bad = []
    for change in (dict(struct_size=24), dict(struct_size=32), dict(flags=1), dict(scheme=2), dict(scheme=0xFFFFFFFF), dict(lifetime=-1.0),
                   dict(lifetime=float("inf")), dict(lifetime=float("nan"))):
        q = capi.ParticleParams(28, 0, capi.PARTICLE_MIDPOINT, (C.c_float * 3)(0, 0, 0), 0.0)
        for k, v in change.items():
            setattr(q, k, v)
        bad.append(q)
    for a in range(3):
        for v in (float("nan"), float("inf"), -float("inf")):
            q = capi.ParticleParams(28, 0, capi.PARTICLE_EULER, (C.c_float * 3)(0, 0, 0), 0.0)
            q.drift[a] = v
            bad.append(q)
    for q in bad:
        assert lib.fx_set_particle_params(f._ctx, C.byref(q)) == capi.FX_E_INVALID and f.GetParticleParams() == mine
    assert lib.fx_get_particle_params(f._ctx, None) == capi.FX_E_INVALID
    out3 = np.zeros((4, 3), f32)
    o3 = out3.ctypes.data_as(fp)
    assert lib.fx_sample_velocity(f._ctx, None, r4, 4, o3, 2) == capi.FX_E_INVALID
    assert lib.fx_sample_velocity(f._ctx, None, None, 4, o3, 0) == capi.FX_E_INVALID and lib.fx_sample_velocity(f._ctx, None, r4, 4, None, 0) == capi.FX_E_INVALID
    assert lib.fx_sample_velocity(f._ctx, None, r4, capi.MAX_PARTICLES + 1, o3, 0) == capi.FX_E_INVALID
    assert lib.fx_sample_velocity(f._ctx, None, None, 0, None, 0) == capi.FX_OK and lib.fx_sample_velocity(f._ctx, None, None, 0, None, capi.PARTICLES_DEVICE) == capi.FX_OK
    assert not out3.any()
    # caller data: kept across UpdateFrame, not digested; dt = 0 moves nothing
    f.UpdateFrame(f32(0.0), 1)
    f.MoveParticles()
    f.Simulate(1)
    assert same_bits(f.GetParticles(), rec) and f.GetParticleParams() == mine
    before = [f.digest(k) for k in ALL_FIELDS]
    f.SetParticles(rec[:5])
    assert before == [f.digest(k) for k in ALL_FIELDS] and f.ParticlesDevice()[1] == 5
    f.SetParticleParams(None)
    assert f.GetParticleParams() == default
    f.SetParticles(np.zeros((0, 4), f32))
    assert f.ParticlesDevice() == (0, 0)
    # slab ranks: the setters refuse, the getters report the empty default
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    for grouped in (False, True):
        if grouped:
            fx.comm_init_local(ranks)
        for r in ranks:
            q = capi.ParticleParams(28, 0, capi.PARTICLE_EULER, (C.c_float * 3)(0, 0, 0), 0.0)
            assert lib.fx_set_particles(r._ctx, None, r4, 4, 0) == capi.FX_E_INVALID and lib.fx_set_particles(r._ctx, None, None, 0, 0) == capi.FX_E_INVALID
            assert lib.fx_set_particle_params(r._ctx, C.byref(q)) == capi.FX_E_INVALID and lib.fx_move_particles(r._ctx, None) == capi.FX_E_INVALID
            assert lib.fx_sample_velocity(r._ctx, None, r4, 4, o3, 0) == capi.FX_E_INVALID
            assert r.GetParticleParams() == default and r.ParticlesDevice() == (0, 0) and r.GetParticles().shape == (0, 4)
    # a render-only context: FX_E_STATE, whatever else is wrong with the call
    ro = fx.Fluid()
    assert ro.Init(64, 64, (32, 32, 8), render_only=True)
    q = capi.ParticleParams(28, 0, capi.PARTICLE_EULER, (C.c_float * 3)(0, 0, 0), 0.0)
    assert lib.fx_set_particles(ro._ctx, None, r4, 4, 0) == capi.FX_E_STATE and lib.fx_set_particles(ro._ctx, None, None, 3, 7) == capi.FX_E_STATE
    assert lib.fx_get_particles(ro._ctx, None, 0, C.byref(n)) == capi.FX_E_STATE and lib.fx_particles_device(ro._ctx, C.byref(p), C.byref(n)) == capi.FX_E_STATE
    assert lib.fx_set_particle_params(ro._ctx, C.byref(q)) == capi.FX_E_STATE and lib.fx_get_particle_params(ro._ctx, C.byref(q)) == capi.FX_E_STATE
    assert lib.fx_move_particles(ro._ctx, None) == capi.FX_E_STATE and lib.fx_sample_velocity(ro._ctx, None, r4, 4, o3, 0) == capi.FX_E_STATE
    for o in [f, ro] + ranks:
        o.Release()
