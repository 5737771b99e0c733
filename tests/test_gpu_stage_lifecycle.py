"""The optional stages' setters over their whole life: set, clear, set with another size, set for good -- then the step must be the one a fresh
context takes that received the final configuration once.  The per-stage files set each feature once on a fresh context; this file holds the
paths behind that: a buffer freed after a step has used it, a scratch that grows (the voxeliser's, the sort's inside fx_set_particles), a pyramid
replaced by one of another depth, and a refused call behind all of it, which must leave what is in force.

Context P is churned, context Q is fresh.  Both then get the same uploaded velocity, colour, pressure and temperature and the same particle
set, take three fx_simulate steps, and agree in every bit of velocity, colour, pressure, temperature, the particle records, the sort's order
and fx_particle_sort_info.  No tolerance anywhere: one device, one library, the same launches.

P takes one step between every feature's first setting and its second, with all the first settings in force, so that what is freed has been
used.  That step leaves nothing behind that the uploads do not level: the two velocity, colour, pressure and temperature buffers are each
written whole before they are read (a solid cell's pressure is written as 0), the step's parity and buffer indices only choose which buffer
an upload lands in, and the sort's counters start again with the final fx_set_particles.

Grid (32, 32, 8), both storages, jacobi_iters 8.  Case "jacobi": everything, under the plain solver.  Case "multigrid": no obstacles and no
open walls (the solver refuses them); the solver itself goes multigrid with 2 levels -> Jacobi -> multigrid with as many as the grid allows."""
import ctypes as C
import functools

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import buoyancy_ref as br
import emitter_ref as er
import moving_obstacle_ref as mor
import particle_ref as pr
import step_ref as sr
import voxelize_ref as vr

pytestmark = pytest.mark.gpu
f32 = np.float32
DIMS, ITERS, STEPS = (32, 32, 8), 8, 3
CASES = [(case, storage) for case in ("jacobi", "multigrid") for storage in ("fp32", "fp16")]
INVALID, STATE = capi.FX_E_INVALID, capi.FX_E_STATE


@functools.lru_cache(maxsize=None)
def initial(storage):
    """what both contexts are given behind their configuration: seeded, fp16-representable where the storage is; shared, never written"""
    half = storage == "fp16"
    X, Y, Z = DIMS
    rng = np.random.default_rng(9100)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    col = col.astype(np.float16).astype(f32) if half else col
    out = dict(vel=pr.velocity(DIMS, 9101, cells=0.6, half=half), col=col, p=rng.standard_normal((Z, Y, X)).astype(f32),
               temp=rng.random((Z, Y, X)).astype(f32), rec=pr.records(DIMS, 3000, 9102))
    for a in out.values():
        a.setflags(write=False)
    return out


def other_mask():
    """not particle_ref.box_mask: a slab against the x_lo wall and a single cell"""
    X, Y, Z = DIMS
    m = np.zeros((Z, Y, X), np.uint8)
    m[1:Z - 2, Y // 2:Y // 2 + 5, 0:7] = 1
    m[Z - 1, 3, X - 2] = 1
    return m


def features(case):
    """name -> the feature's settings in the order P makes them, as calls on a Fluid; the last one is the final configuration, all Q gets"""
    emit = [er.emitter(br.SIX[k][0], br.SIX[k][1]) for k in (0, 1, 3)]
    buoy = [br.params(ambient=0.5, density_weight=0.2, lift=0.8, cooling=0.1), sr.BUOY]
    sort = lambda on, every: (lambda f: f.SetParticleSort(on, every))
    out = {
        "emitters": [lambda f: f.SetEmitters(emit), lambda f: f.SetEmitters(None), lambda f: f.SetEmitters(emit[1:2])],
        "heat sources": [lambda f: f.SetHeatSources(br.list_b()), lambda f: f.SetHeatSources(None), lambda f: f.SetHeatSources(br.list_a())],
        "buoyancy": [lambda f: f.SetBuoyancy(**buoy[0]), lambda f: f.SetBuoyancy(None), lambda f: f.SetBuoyancy(**buoy[1])],
        "advection": [lambda f: f.SetAdvectionScheme("maccormack"), lambda f: f.SetAdvectionScheme("semi-lagrangian"),
                      lambda f: f.SetAdvectionScheme("maccormack")],
        # the scratch is allocated for 1000 records, resized to none and to 3000 inside fx_set_particles, freed, and allocated again for 3000;
        # the set itself comes last, with the fields (`level`)
        "particles": [lambda f: (f.SetParticles(pr.records(DIMS, 1000, 9110)), sort(True, 1)(f)), lambda f: f.SetParticles(None),
                      lambda f: f.SetParticles(pr.records(DIMS, 3000, 9111)), sort(False, 0), sort(True, 2)],
        "trail": [lambda f: f.SetParticleTrail(1.0, (0.5, 0.5, 0.5, 0.5), 1.0), lambda f: f.SetParticleTrail(None),
                  lambda f: f.SetParticleTrail(sr.TRAIL["rate"], sr.TRAIL["tint"], sr.TRAIL["heat"])],
    }
    if case == "multigrid":
        mg = lambda levels: (lambda f: f.SetPressureSolver("multigrid", max_levels=levels))
        out["solver"] = [mg(2), lambda f: f.SetPressureSolver("jacobi"), mg(0)]
        return out
    box = lambda lo, hi: mor.body(lo, hi, linear=(0.05, -0.02, 0.01), angular=(0.0, 0.3, -0.2))
    bodies = [box((0.0, 0.0, 0.0), (0.5, 1.0, 1.0)), box((0.5, 0.0, 0.0), (1.0, 1.0, 1.0))]
    small = vr.box_mesh((0.3, 0.3, 0.2), (0.6, 0.7, 0.8))                       # 12 triangles, then 528: the voxeliser's work buffer grows
    large = vr.uv_sphere((0.55, 0.45, 0.5), (0.2, 0.25, 0.35))
    out["obstacles"] = [lambda f: f.SetObstacles(pr.box_mask(DIMS)), lambda f: f.SetObstacles(None), lambda f: f.SetObstacles(other_mask()),
                        lambda f: f.SetObstacleMeshes([(small[0], small[1], None)]), lambda f: f.SetObstacleMeshes([(large[0], large[1], None)])]
    out["bodies"] = [lambda f: f.SetObstacleBodies(bodies), lambda f: f.SetObstacleBodies(None), lambda f: f.SetObstacleBodies(bodies[1:])]
    out["open walls"] = [lambda f: f.SetOpenWalls(capi.WALL_X_LO | capi.WALL_Y_HI), lambda f: f.SetOpenWalls(0), lambda f: f.SetOpenWalls(capi.WALL_Y_HI)]
    return out


def refusals(f, case):
    """one refused call per setter -> [(what, status, the status it has to be)]"""
    lib, ctx = f._lib, f._ctx
    n = DIMS[0] * DIMS[1] * DIMS[2]
    bad = lambda T, count=1: (T * count)()                                       # zeroed records: struct_size 0
    too_short = np.zeros(n - 1, np.uint8)
    rec = np.zeros((1, 4), f32)
    ps = lambda kind: capi.PressureSolver(kind, 0, 2, 2, 2, 16, 0, 0.8)
    mg = case == "multigrid"
    return [
        ("fx_set_emitters: struct_size", lib.fx_set_emitters(ctx, bad(capi.Emitter), 1), INVALID),
        ("fx_set_emitters: count", lib.fx_set_emitters(ctx, bad(capi.Emitter, capi.MAX_EMITTERS + 1), capi.MAX_EMITTERS + 1), INVALID),
        ("fx_set_heat_sources: count", lib.fx_set_heat_sources(ctx, bad(capi.HeatSource, capi.MAX_HEAT_SOURCES + 1), capi.MAX_HEAT_SOURCES + 1), INVALID),
        ("fx_set_obstacle_bodies: struct_size", lib.fx_set_obstacle_bodies(ctx, bad(capi.ObstacleBody), 1), INVALID),
        ("fx_set_obstacle_bodies: count", lib.fx_set_obstacle_bodies(ctx, bad(capi.ObstacleBody, capi.MAX_OBSTACLE_BODIES + 1), capi.MAX_OBSTACLE_BODIES + 1), INVALID),
        # (under multigrid the solver's refusal comes first)
        ("fx_set_obstacles: bytes", lib.fx_set_obstacles(ctx, None, too_short.ctypes.data, too_short.size, 0), STATE if mg else INVALID),
        ("fx_set_obstacle_meshes: struct_size", lib.fx_set_obstacle_meshes(ctx, None, bad(capi.ObstacleMesh), 1, None), INVALID),
        ("fx_set_obstacle_meshes: count", lib.fx_set_obstacle_meshes(ctx, None, bad(capi.ObstacleMesh, capi.MAX_OBSTACLE_MESHES + 1), capi.MAX_OBSTACLE_MESHES + 1, None), INVALID),
        ("fx_set_open_walls", lib.fx_set_open_walls(ctx, capi.WALL_Y_HI if mg else 0x40), STATE if mg else INVALID),
        ("fx_set_buoyancy: struct_size", lib.fx_set_buoyancy(ctx, bad(capi.Buoyancy)), INVALID),
        ("fx_set_advection_scheme", lib.fx_set_advection_scheme(ctx, 7), INVALID),
        ("fx_set_pressure_solver: kind", lib.fx_set_pressure_solver(ctx, C.byref(ps(9))), INVALID),
        ("fx_set_pressure_solver: cycles", lib.fx_set_pressure_solver(ctx, C.byref(capi.PressureSolver(capi.PRESSURE_MULTIGRID, 0, 0, 2, 2, 16, 0, 0.8))), INVALID),
        ("fx_set_particles: count", lib.fx_set_particles(ctx, None, rec.ctypes.data_as(C.POINTER(C.c_float)), capi.MAX_PARTICLES + 1, 0), INVALID),
        ("fx_set_particles: flags", lib.fx_set_particles(ctx, None, rec.ctypes.data_as(C.POINTER(C.c_float)), 1, 0x2), INVALID),
        ("fx_set_particle_params: struct_size", lib.fx_set_particle_params(ctx, bad(capi.ParticleParams)), INVALID),
        ("fx_set_particle_sort: struct_size", lib.fx_set_particle_sort(ctx, bad(capi.ParticleSort)), INVALID),
        ("fx_set_particle_trail: struct_size", lib.fx_set_particle_trail(ctx, bad(capi.ParticleTrail)), INVALID),
    ] + ([] if mg else [("fx_set_pressure_solver: multigrid beside obstacles", lib.fx_set_pressure_solver(ctx, C.byref(ps(capi.PRESSURE_MULTIGRID))), STATE)])


def create(storage):
    f = fx.Fluid()
    assert f.Init(0, 0, DIMS, storage=storage, jacobi_iters=ITERS), f.last_status
    f.SetVorticityConfinement(4.0)
    f.SetParticleParams("midpoint", sr.DRIFT, sr.LIFETIME)
    return f


def level(f, s0):
    f.upload(fx.FIELD_VELOCITY, s0["vel"]); f.upload(fx.FIELD_COLOR, s0["col"]); f.upload(fx.FIELD_PRESSURE, s0["p"])
    f.upload(fx.FIELD_TEMPERATURE, s0["temp"])
    f.SetParticles(s0["rec"])


def run(f, dt):
    for i in range(STEPS):
        f.UpdateFrame(dt, i % 3)
        f.Simulate(i % 3)
    f.Synchronize()
    return dict(VELOCITY=f.download(fx.FIELD_VELOCITY), COLOR=f.download(fx.FIELD_COLOR), PRESSURE=f.download(fx.FIELD_PRESSURE),
                TEMPERATURE=f.download(fx.FIELD_TEMPERATURE), PARTICLES=f.GetParticles(), ORDER=f.ParticleOrder(),
                SORT_INFO=np.array(f.ParticleSortInfo(), np.uint32))


@pytest.mark.parametrize("case,storage", CASES)
def test_a_churned_context_steps_like_a_fresh_one(case, storage):
    feats = features(case)
    dt = pr.time_step(DIMS)
    s0 = initial(storage)
    P, Q = create(storage), create(storage)
    for calls in feats.values():
        calls[0](P)
    P.UpdateFrame(dt, 0)
    P.Simulate(0)
    P.Synchronize()
    for calls in feats.values():
        for call in calls[1:]:
            call(P)
    for calls in feats.values():
        calls[-1](Q)
    refused = refusals(P, case)
    wrong = [(what, got, want) for what, got, want in refused if got != want]
    assert not wrong, wrong
    level(P, s0); level(Q, s0)
    got, want = run(P, dt), run(Q, dt)
    assert got["SORT_INFO"][1] == 2                                              # every 2: the first and the third run of the stage sorted
    P.Release(); Q.Release()
    diff = sr.first_difference(got, want)
    assert diff is None, "first difference in %s at %s: churned %r, fresh %r (%d elements differ)" % diff
