"""The particle spawners on the GPU (fx_set_particle_spawners / fx_spawn_particles / fx_particle_spawn_info, csrc/fx_particle_spawn.hip)
against the numpy model tests/particle_spawn_ref.py: every record and the whole info struct bit for bit.

Shapes: 12 x 12 x 8 in both storages and 12 x 12 x 1 (fx_create takes X = Y alone, so the rows are the odd extent here); pools of 2500 records -- three workgroups of 1024, the last one partial -- and one of
2^21 + 1500, at which the scan of the workgroup counts takes its reduce / block sums / apply path."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import particle_ref as pr
import particle_sort_ref as ps
import particle_spawn_ref as sr
import particle_trail_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
GRIDS = [((12, 12, 8), "fp32"), ((12, 12, 8), "fp16"), ((12, 12, 1), "fp32")]
POOL = 2500
# a box that reaches over the -x and the +y wall, so that the clamp acts, and a ball
BOX = sr.spawner(shape=sr.BOX, seed=11, center=(0.1, 0.8, 0.5), half_extent=(0.2, 0.3, 0.25), rate=900.0, age_spread=0.3)
BALL = sr.spawner(shape=sr.BALL, seed=0xdeadbeef, center=(0.6, 0.4, 0.5), half_extent=(0.3, 0.2, 0.4), rate=500.0, age_spread=0.0)
ITERS = 8


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status
    return f


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def pool(dims, n, seed, dead_share=0.5):
    """n records, a share of them dead and scattered: by a negative age, a NaN age with a payload, or -inf in turn; every seventh dead record
    holds NaN payloads as its position; some live records have the age -0.0"""
    rng = np.random.default_rng(seed)
    rec = pr.records(dims, n, seed, dead_every=n + 1)                      # all live, the edge points first
    dead = np.flatnonzero(rng.random(n) < dead_share)
    kinds = np.array([0xbf800000, 0x7fc01234, 0xff800000, 0xffc00001], np.uint32).view(f32)
    rec[dead, 3] = kinds[np.arange(len(dead)) % 4]
    rec[dead[::7], :3] = np.array([0x7fc0beef, 0xffc00002, 0x7f800001], np.uint32).view(f32)
    live = np.setdiff1d(np.arange(n), dead)
    rec[live[::9], 3] = f32(-0.0)
    return rec


def run_alone(f, sp, st, rec, dt, dims, steps, solid=None, tag=""):
    """`steps` runs of the stage alone, each held to the model: the records and the info struct"""
    for k in range(steps):
        f.SpawnParticles()
        f.Synchronize()
        rec = sr.step(rec, sp, st, dt, dims, solid=solid)
        assert same_bits(f.GetParticles(), rec), (tag, k)
        assert f.ParticleSpawnInfo() == sr.info(st), (tag, k)
    return rec


# ---- 1: the stage alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,storage", GRIDS)
def test_the_stage_alone_is_the_models(dims, storage):
    dt = pr.time_step(dims)
    sp = [BOX, BALL]
    f = make(dims, storage=storage)
    f.UpdateFrame(dt, 0)
    rec = pool(dims, POOL, 5)
    f.SetParticles(rec)
    f.SetParticleSpawners(sp)
    got = f.GetParticleSpawners()
    assert [g["shape"] for g in got] == ["box", "ball"] and [g["seed"] for g in got] == [11, 0xdeadbeef]
    assert f.ParticleSpawnInfo() == sr.info(sr.new_state(2))
    st = sr.new_state(2)
    out = run_alone(f, sp, st, rec, dt, dims, 4, tag=storage)
    assert st["born"] == sum(st["serial"]) > 400 and st["dropped"] == 0 and st["blocked"] == 0 and min(st["serial"]) > 150
    with np.errstate(invalid="ignore"):
        was_live = rec[:, 3] >= 0
    assert same_bits(out[was_live], rec[was_live])                         # no live record changes a bit, -0.0 ages included
    born = ~was_live & (out[:, 3] >= 0)
    assert int(born.sum()) == st["born"]
    assert (out[born, 0] == 0).any() and (out[born, 1] == 1).any() and not np.signbit(out[born, :3]).any()      # the clamp acted
    if dims[2] == 1:
        assert set(np.unique(out[born, 2])) == {f32(0.5)}                  # a 2-D grid draws no z
    f.Release()


# ---- 2: overflow ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,storage", [GRIDS[0], GRIDS[2]])
def test_births_beyond_the_dead_slots_are_dropped(dims, storage):
    dt = pr.time_step(dims)
    sp = [sr.spawner(BOX, rate=1200.0), sr.spawner(BALL, rate=900.0)]
    f = make(dims, storage=storage)
    f.UpdateFrame(dt, 0)
    rec = pool(dims, POOL, 7, dead_share=0.04)
    with np.errstate(invalid="ignore"):
        D = int((~(rec[:, 3] >= 0)).sum())
    f.SetParticles(rec)
    f.SetParticleSpawners(sp)
    st = sr.new_state(2)
    out = run_alone(f, sp, st, rec, dt, dims, 1, tag="first")
    n = sum(st["serial"])
    assert D < n and (st["born"], st["dropped"]) == (D, n - D)
    with np.errstate(invalid="ignore"):
        assert (out[:, 3] >= 0).all()
    out = run_alone(f, sp, st, out, dt, dims, 1, tag="full")               # no slot at all: everything dropped, the serials advance
    assert st["born"] == D
    # some records die (the caller's upload of the same count: the serials stay) and the next step goes on with the serials the model has
    out[3::5, 3] = -1
    f.SetParticles(out)
    assert f.ParticleSpawnInfo() == sr.info(st)
    out = run_alone(f, sp, st, out, dt, dims, 2, tag="reused")
    assert st["born"] > D and st["dropped"] > n - D
    f.Release()


# ---- 3: solids ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,storage", [GRIDS[1], GRIDS[2]])
def test_a_birth_inside_a_solid_is_blocked(dims, storage):
    dt = pr.time_step(dims)
    sp = [sr.spawner(shape=sr.BOX, seed=21, center=(0.5, 0.5, 0.5), half_extent=(0.4, 0.3, 0.3), rate=1500.0, age_spread=0.1), BALL]
    solid = np.zeros(dims[::-1], np.uint8)
    solid[:, :, dims[0] // 2:] = 1                                         # half the box
    f = make(dims, storage=storage)
    f.UpdateFrame(dt, 0)
    f.SetObstacles(solid)
    rec = pool(dims, POOL, 9, dead_share=0.8)
    st = sr.new_state(2)
    for bodies in ((), [dict(box_lo=(0.2, 0.2, 0.0), box_hi=(0.8, 0.8, 1.0), linear=(0.5, 0.0, 0.0), angular=(0.0, 0.0, 1.0))]):
        f.SetObstacleBodies(bodies)                                        # resting and moving solids: the same code bit
        f.SetParticles(rec)
        f.SetParticleSpawners(sp)
        st = sr.new_state(2)
        out = run_alone(f, sp, st, rec, dt, dims, 2, solid=solid, tag=len(bodies))
        assert st["blocked"] > 100 and st["born"] > 100 and st["dropped"] == 0
        with np.errstate(invalid="ignore"):
            still_dead = ~(out[:, 3] >= 0)
        assert same_bits(out[still_dead], rec[still_dead])                 # blocked slots stay dead with their bits kept
        with np.errstate(invalid="ignore"):
            born = ~(rec[:, 3] >= 0) & ~still_dead
        assert (np.minimum((out[born, 0] * f32(dims[0])).astype(np.int64), dims[0] - 1) < dims[0] // 2).all()
    f.Release()


# ---- 4: inside fx_simulate ------------------------------------------------------------------------------------------------------------------
TRAIL = tr.trail(rate=3.0, tint=(0.25, -0.5, 0.125, 0.7))
PRM = pr.params(scheme=pr.MIDPOINT, drift=(0.03, -0.4, 0.02), lifetime=0.5)


def run_steps(dims, storage, mode, spawners=True, trail=True, steps=6):
    """mode "whole": fx_simulate; "staged": the stage calls in the step's order, each particle stage held to the composed model
    -> (digests of the six fields, the particles, the info)"""
    half = storage == "fp16"
    sp = [BOX, BALL]
    vel = pr.velocity(dims, 751, cells=0.6, half=half)
    col = np.random.default_rng(753).random((dims[2], dims[1], dims[0], 4)).astype(f32)
    col = col.astype(np.float16).astype(f32) if half else col
    f = make(dims, storage=storage, jacobi_iters=ITERS)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetParticleSort(True, 2)
    rec = pool(dims, POOL, 13, dead_share=0.3)
    with np.errstate(invalid="ignore"):
        rec[:, 3] = np.where(rec[:, 3] >= 0, np.abs(rec[:, 3]) * f32(0.6), rec[:, 3])  # ages below 0.6: some die in every step
    f.SetParticles(rec)
    f.SetParticleParams("midpoint", PRM["drift"], PRM["lifetime"])
    if trail:
        f.SetParticleTrail(TRAIL["rate"], TRAIL["tint"], TRAIL["heat"])
    if spawners:
        f.SetParticleSpawners(sp)
    st = sr.new_state(2)
    dt = pr.time_step(dims)
    reused = 0
    for i in range(steps):
        f.UpdateFrame(dt, i % 3)
        if mode == "whole":
            f.Simulate(i % 3)
            continue
        f.Advect(); f.OpenInflow(); f.Emit(); f.Heat()
        before = f.download(fx.FIELD_COLOR)
        f.DepositParticles()
        assert same_bits(f.download(fx.FIELD_COLOR), tr.apply(tr.density(rec, dims), before, dt, TRAIL, half=half)[0]), i
        f.EnforceObstacles(); f.ConfineVorticity()
        f.Divergence(); f.Jacobi(ITERS); f.Project()
        v = f.download(fx.FIELD_VELOCITY)                                   # the velocity in front of the move, as the device holds it
        f.MoveParticles()                                                  # the sort if due, the move, the births
        if i % 2 == 0:
            rec = ps.sort(rec, dims)[0]
        moved = pr.move(rec, v, dt, PRM)
        with np.errstate(invalid="ignore"):
            reused += int(((rec[:, 3] >= 0) & ~(moved[:, 3] >= 0)).sum())   # died in this move: slots the births of this step may take
        rec = sr.step(moved, sp, st, dt, dims)
        assert same_bits(f.GetParticles(), rec), i
        assert f.ParticleSpawnInfo() == sr.info(st), i
    if mode == "staged":
        assert reused > 200 and st["born"] > 600 and st["born"] + st["dropped"] == sum(st["serial"])     # records died, slots were taken
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS], f.GetParticles(), f.ParticleSpawnInfo()
    f.Release()
    return out


@pytest.mark.parametrize("dims,storage", [GRIDS[0], ((12, 12, 1), "fp16")])
def test_simulate_spawns_behind_the_move(dims, storage):
    staged, ps_, is_ = run_steps(dims, storage, "staged")
    whole, pw, iw = run_steps(dims, storage, "whole")
    assert whole == staged and same_bits(pw, ps_) and iw == is_
    # the trail off: no field knows whether spawners exist
    with_, p1, i1 = run_steps(dims, storage, "whole", spawners=True, trail=False)
    without, p0, i0 = run_steps(dims, storage, "whole", spawners=False, trail=False)
    assert with_ == without and not same_bits(p1, p0)
    assert i1["born"] > 600 and i0 == sr.info(sr.new_state(0))
    assert with_[2] != whole[2]                                            # ... and with a trail the births do reach the colour


# ---- 5: a large pool ------------------------------------------------------------------------------------------------------------------------
def test_a_large_pool_takes_the_scans_block_sums():
    dims = (12, 12, 8)
    n = (1 << 21) + 1500                                                   # 2050 workgroup counts: two scan tiles
    dt = pr.time_step(dims)
    rng = np.random.default_rng(31)
    rec = np.empty((n, 4), f32)
    rec[:, :3] = rng.random((n, 3), dtype=f32)
    rec[:, 3] = 1.0
    early = rng.choice(1 << 21, 20, replace=False)
    late = n - 1 - rng.choice(3000, 400, replace=False)                    # the last four workgroups, both sides of the tile edge
    rec[early, 3] = -1
    rec[late, 3] = np.nan
    sp = [sr.spawner(BOX, rate=540.0), sr.spawner(BALL, rate=360.0)]       # 90 + 60 births per step
    f = make(dims)
    f.UpdateFrame(dt, 0)
    f.SetParticles(rec)
    f.SetParticleSpawners(sp)
    st = sr.new_state(2)
    out = run_alone(f, sp, st, rec, dt, dims, 2, tag="large")
    assert st["born"] == 300 and st["dropped"] == 0
    with np.errstate(invalid="ignore"):
        assert (out[early, 3] >= 0).all() and int((out[late, 3] >= 0).sum()) == 280
        assert (out[late[late >= 1 << 21], 3] >= 0).any() and (out[late[late < 1 << 21], 3] >= 0).any()
    run_alone(f, sp, st, out, dt, dims, 1, tag="dropping")                 # 120 slots left for 150 births
    assert st["born"] == 420 and st["dropped"] == 30
    f.Release()


# ---- 6: capture -----------------------------------------------------------------------------------------------------------------------------
SPAWN_LAUNCHES = 4          # k_spawn_count, the one-tile scan, k_spawn_tick, k_spawn_place


def graph_nodes(f, frame):
    """the launches one fx_simulate enqueues: the step captured on a stream of its own (never replayed), its graph's nodes counted"""
    hip = capi.load()                                                      # the HIP runtime the library itself is linked against
    vp = C.c_void_p
    hip.hipStreamCreate.restype, hip.hipStreamCreate.argtypes = C.c_int, [C.POINTER(vp)]
    hip.hipStreamDestroy.restype, hip.hipStreamDestroy.argtypes = C.c_int, [vp]
    hip.hipStreamBeginCapture.restype, hip.hipStreamBeginCapture.argtypes = C.c_int, [vp, C.c_int]
    hip.hipStreamEndCapture.restype, hip.hipStreamEndCapture.argtypes = C.c_int, [vp, C.POINTER(vp)]
    hip.hipGraphGetNodes.restype, hip.hipGraphGetNodes.argtypes = C.c_int, [vp, vp, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.restype, hip.hipGraphDestroy.argtypes = C.c_int, [vp]
    s, g, n = vp(None), vp(None), C.c_size_t(0)
    f.Synchronize()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0                            # 2: hipStreamCaptureModeRelaxed
    rc = f._lib.fx_simulate(f._ctx, s, frame)
    end = hip.hipStreamEndCapture(s, C.byref(g))
    assert rc == capi.FX_OK and end == 0 and g.value
    assert hip.hipGraphGetNodes(g, None, C.byref(n)) == 0
    assert hip.hipGraphDestroy(g) == 0 and hip.hipStreamDestroy(s) == 0
    return int(n.value)


def test_a_step_with_spawners_captures_and_costs_four_launches():
    dims = (12, 12, 8)
    f = make(dims, jacobi_iters=ITERS)
    f.upload(fx.FIELD_VELOCITY, pr.velocity(dims, 751, cells=0.6))
    f.SetParticles(pool(dims, POOL, 17))
    dt = pr.time_step(dims)
    f.UpdateFrame(dt, 0); f.Simulate(0)
    f.UpdateFrame(dt, 1)
    off = graph_nodes(f, 1)
    f.SetParticleSpawners([BOX, BALL])
    f.UpdateFrame(dt, 2)
    on = graph_nodes(f, 2)
    assert f.ParticleSpawnInfo() == sr.info(sr.new_state(2))                # captured, never run: nothing ticked
    f.SetParticleSpawners(None)
    f.UpdateFrame(dt, 0)
    again = graph_nodes(f, 0)
    f.SetParticles(None)
    f.SetParticleSpawners([BOX])
    f.UpdateFrame(dt, 1)
    no_set = graph_nodes(f, 1)
    f.Release()
    assert on == off + SPAWN_LAUNCHES and again == off and no_set == off - 1, (off, on, again, no_set)   # (no set: the move goes, nothing is born)


# ---- 7: refusals and round trips ------------------------------------------------------------------------------------------------------------
def c_spawner(**change):
    q = capi.ParticleSpawner(48, 0, capi.SPAWN_BALL, 5, (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.1, 0.1, 0.1), 10.0, 0.5)
    for k, v in change.items():
        setattr(q, k, (C.c_float * 3)(*v) if k in ("center", "half_extent") else v)
    return q


def test_status_codes_and_round_trips():
    lib = capi.load()
    dims = (12, 12, 8)
    dt = pr.time_step(dims)
    f = make(dims)
    f.UpdateFrame(dt, 0)
    empty = sr.info(sr.new_state(0))
    # the default: off
    assert f.GetParticleSpawners() == [] and f.ParticleSpawnInfo() == empty
    assert lib.fx_spawn_particles(f._ctx, None) == capi.FX_E_STATE
    f.SetParticleSpawners(None); f.SetParticleSpawners([])
    assert lib.fx_spawn_particles(f._ctx, None) == capi.FX_E_STATE
    # spawners without a set: FX_OK, nothing done, the state does not tick
    sp = [BOX, BALL]
    f.SetParticleSpawners(sp)
    mine = f.GetParticleSpawners()
    assert len(mine) == 2 and mine[1]["center"] == tuple(float(f32(v)) for v in BALL["center"]) and mine[0]["rate"] == 900.0
    f.SpawnParticles(); f.MoveParticles(); f.Simulate(0)
    assert f.ParticleSpawnInfo() == sr.info(sr.new_state(2))
    # a pool: the set that is only ever spawned into
    f.SetParticlePool(300)
    start = f.GetParticles()
    assert start.shape == (300, 4) and not start[:, :3].any() and (start[:, 3] == -1).all()
    st = sr.new_state(2)
    rec = run_alone(f, sp, st, start, dt, dims, 1, tag="pool")
    assert st["born"] == 233
    # dt = 0: nothing, the state does not tick
    f.UpdateFrame(f32(0.0), 1)
    f.SpawnParticles(); f.Simulate(1)
    assert same_bits(f.GetParticles(), rec) and f.ParticleSpawnInfo() == sr.info(st)
    f.UpdateFrame(dt, 2)
    # refused, the previous spawners and their state staying in force
    nan, inf = float("nan"), float("inf")
    for change in (dict(struct_size=44), dict(struct_size=52), dict(flags=1), dict(flags=0x80000000), dict(shape=2), dict(shape=0xffffffff),
                   dict(rate=-1e-30), dict(rate=nan), dict(rate=inf), dict(age_spread=-1.0), dict(age_spread=nan), dict(age_spread=inf),
                   dict(center=(0.5, nan, 0.5)), dict(center=(inf, 0.5, 0.5)), dict(half_extent=(0.1, 0.1, -1e-30)), dict(half_extent=(nan, 0.1, 0.1)),
                   dict(half_extent=(0.1, inf, 0.1))):
        arr = (capi.ParticleSpawner * 2)(c_spawner(), c_spawner(**change))
        assert lib.fx_set_particle_spawners(f._ctx, arr, 2) == capi.FX_E_INVALID, change
        assert f.GetParticleSpawners() == mine and f.ParticleSpawnInfo() == sr.info(st), change
    big = (capi.ParticleSpawner * 17)(*[c_spawner() for _ in range(17)])
    assert lib.fx_set_particle_spawners(f._ctx, big, 17) == capi.FX_E_INVALID
    assert lib.fx_set_particle_spawners(f._ctx, None, 1) == capi.FX_E_INVALID
    n = C.c_uint32(0)
    assert lib.fx_get_particle_spawners(f._ctx, big, 17, None) == capi.FX_E_INVALID
    assert lib.fx_get_particle_spawners(f._ctx, None, 1, C.byref(n)) == capi.FX_E_INVALID
    assert lib.fx_get_particle_spawners(f._ctx, None, 0, C.byref(n)) == capi.FX_OK and n.value == 2
    assert lib.fx_particle_spawn_info(f._ctx, None, None) == capi.FX_E_INVALID
    assert f.GetParticleSpawners() == mine and f.ParticleSpawnInfo() == sr.info(st)
    # accepted: sixteen spawners, rate 0, half extents 0
    f.SetParticleSpawners([sr.spawner(rate=0.0, half_extent=(0.0, 0.0, 0.0), seed=k) for k in range(16)])
    assert len(f.GetParticleSpawners()) == 16 and f.ParticleSpawnInfo() == sr.info(sr.new_state(16))      # a new list: the state starts again
    f.SpawnParticles()
    assert same_bits(f.GetParticles(), rec) and f.ParticleSpawnInfo() == sr.info(sr.new_state(16))
    # fx_set_particles with another count keeps the serials and the counters
    f.SetParticleSpawners(sp)
    st = sr.new_state(2)
    rec = run_alone(f, sp, st, rec, dt, dims, 1, tag="before")
    assert st["dropped"] > 0
    grown = pool(dims, 1500, 41)
    f.SetParticles(grown)
    assert f.ParticleSpawnInfo() == sr.info(st) and f.GetParticleSpawners() == mine
    run_alone(f, sp, st, grown, dt, dims, 2, tag="resized")
    # kept across UpdateFrame, not digested
    before = [f.digest(k) for k in ALL_FIELDS]
    f.UpdateFrame(dt, 1)
    f.SpawnParticles()
    assert f.GetParticleSpawners() == mine and before == [f.digest(k) for k in ALL_FIELDS]
    # slab ranks: the setter and the stage refuse, the getter and the info call report the empty default
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    one = (capi.ParticleSpawner * 1)(c_spawner())
    for r in ranks:
        assert lib.fx_set_particle_spawners(r._ctx, one, 1) == capi.FX_E_INVALID and lib.fx_set_particle_spawners(r._ctx, None, 0) == capi.FX_E_INVALID
        assert lib.fx_spawn_particles(r._ctx, None) == capi.FX_E_INVALID
        assert r.GetParticleSpawners() == [] and r.ParticleSpawnInfo() == empty
    # a render-only context: FX_E_STATE, whatever else is wrong with the call
    ro = fx.Fluid()
    assert ro.Init(64, 64, (32, 32, 8), render_only=True)
    info = capi.ParticleSpawnInfo()
    assert lib.fx_set_particle_spawners(ro._ctx, one, 1) == capi.FX_E_STATE and lib.fx_set_particle_spawners(ro._ctx, None, 17) == capi.FX_E_STATE
    assert lib.fx_get_particle_spawners(ro._ctx, None, 0, C.byref(n)) == capi.FX_E_STATE and lib.fx_spawn_particles(ro._ctx, None) == capi.FX_E_STATE
    assert lib.fx_particle_spawn_info(ro._ctx, None, C.byref(info)) == capi.FX_E_STATE
    # Release() with the block allocated is clean; NULL is the default again
    g = make(dims)
    g.SetParticlePool(100)
    g.SetParticleSpawners(sp)
    f.SetParticleSpawners(None)
    assert f.GetParticleSpawners() == [] and f.ParticleSpawnInfo() == empty and lib.fx_spawn_particles(f._ctx, None) == capi.FX_E_STATE
    for o in [f, ro, g] + ranks:
        o.Release()


# ---- 8: the C++ wrapper ---------------------------------------------------------------------------------------------------------------------
CXX = r'''
#include "Fluid.hpp"
#include <cstdio>
using namespace fluidx;
int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	const XMUINT3 grid = { 12, 12, 8 };
	Fluid::Options opt;
	opt.storage = FX_STORAGE_FP32; opt.jacobiIters = 4; opt.jacobiMode = FX_JACOBI_FIXED;
	Fluid fluid;
	if (!fluid.Init(nullptr, 0, 0, grid, opt)) return 3;
	if (fluid.SpawnParticles() || fluid.LastStatus() != FX_E_STATE) return 4;                         // off by default
	struct fx_particle_spawn_info info = {};
	info.born = 5;
	if (!fluid.ParticleSpawnInfo(info) || info.struct_size != 160 || info.born != 0) return 5;
	fx_particle_spawner sp[2] = {
		{ (uint32_t)sizeof(fx_particle_spawner), 0u, FX_SPAWN_BOX, 11u, { 0.1f, 0.8f, 0.5f }, { 0.2f, 0.3f, 0.25f }, 900.0f, 0.3f },
		{ (uint32_t)sizeof(fx_particle_spawner), 0u, FX_SPAWN_BALL, 0xdeadbeefu, { 0.6f, 0.4f, 0.5f }, { 0.3f, 0.2f, 0.4f }, 500.0f, 0.0f } };
	if (fluid.SetParticleSpawners(sp, 17) || fluid.LastStatus() != FX_E_INVALID) return 6;
	if (!fluid.SetParticlePool(300) || !fluid.SetParticleSpawners(sp, 2)) return 7;
	fx_particle_spawner got[FX_MAX_PARTICLE_SPAWNERS];
	uint32_t n = 0;
	if (!fluid.GetParticleSpawners(got, FX_MAX_PARTICLE_SPAWNERS, n) || n != 2 || got[1].seed != 0xdeadbeefu || got[0].rate != 900.0f) return 8;
	const XMFLOAT4X4 m = {};
	const XMFLOAT3 eye = {};
	fluid.UpdateFrame(1.0f / 6.0f, 0, m, m, eye);
	if (fluid.LastStatus() != FX_OK) return 9;
	if (!fluid.SpawnParticles() || !fluid.SpawnParticles()) return 10;
	if (!fluid.ParticleSpawnInfo(info)) return 11;
	std::vector<float> rec;
	if (!fluid.GetParticles(rec) || rec.size() != 1200) return 12;
	if (!fluid.SetParticleSpawners(nullptr, 0) || !fluid.GetParticleSpawners(got, 0, n) || n != 0) return 13;
	FILE* f = std::fopen(argv[1], "wb");
	if (!f || std::fwrite(rec.data(), 4, rec.size(), f) != rec.size() || std::fwrite(&info, sizeof info, 1, f) != 1) return 14;
	return std::fclose(f) ? 15 : 0;
}
'''


def test_the_cxx_wrapper_spawns(tmp_path):
    from fluidx12_amd import build as fxbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cc)
    libdir = os.path.dirname(fxbuild.ensure_built())
    dims = (12, 12, 8)
    src, exe, out = tmp_path / "spawn.cpp", str(tmp_path / "spawn"), str(tmp_path / "out.bin")
    src.write_text(CXX)
    subprocess.run([cc, "-std=c++17", "-O1", "-I", os.path.join(root, "fluidx12_amd", "csrc"), str(src), "-o", exe, "-L" + libdir, "-lfluidx_hip",
                    "-Wl,-rpath," + libdir], check=True, timeout=300)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)             # a fresh child process, under its own time limit
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(out, np.uint8)
    rec = raw[:4800].view(f32).reshape(300, 4)
    info = capi.ParticleSpawnInfo.from_buffer_copy(raw[4800:].tobytes())
    st = sr.new_state(2)
    want = np.zeros((300, 4), f32)
    want[:, 3] = -1
    for _ in range(2):
        want = sr.step(want, [BOX, BALL], st, f32(1.0) / f32(6.0), dims)
    assert same_bits(rec, want)
    assert dict(born=info.born, dropped=info.dropped, blocked=info.blocked, serial=list(info.serial)) == sr.info(st) and st["dropped"] > 0
