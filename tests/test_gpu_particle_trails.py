"""The particle trail on the GPU (fx_set_particle_trail / fx_deposit_particles / fx_particle_density, csrc/fx_particle_trail.hip) against the
numpy model tests/particle_trail_ref.py: the accumulator volume as uint64 words, colour, temperature and the render's side volume bit for bit.

Shapes: particle_ref.SHAPES -- rows that are no multiple of a wave, thin z, 2-D, a wide row --, both storages, counts 1, 257 and 4099: a wave
edge and a workgroup edge inside the runs the scatter merges."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import buoyancy_ref as br
import emitter_ref as er
import particle_ref as pr
import particle_trail_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
SHAPES, COUNTS, STORAGES = tr.SHAPES, tr.COUNTS, ("fp32", "fp16")
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
TRAIL = tr.trail(rate=3.0, tint=(0.25, -0.5, 0.125, 0.7), heat=-2.5)
BUOY = dict(ambient=0.25, density_weight=0.7, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2))
ITERS = 8


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status
    return f


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def set_trail(f, t=TRAIL):
    f.SetParticleTrail(t["rate"], t["tint"], t["heat"])


def live_count(rec):
    return int(tr.live_of(rec).sum())


# ---- 1, 2: the scatter against the model ----------------------------------------------------------------------------------------------------
def check_density(f, rec, dims, tag):
    f.SetParticles(rec)
    want = tr.density(rec, dims)
    got = f.ParticleDensity()
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), tag
    return want


@pytest.mark.parametrize("dims", SHAPES)
def test_the_density_is_the_models_volume(dims):
    f = make(dims)
    set_trail(f)
    assert not f.ParticleDensity().any()                                   # no set: zeros
    for name in tr.ARRANGEMENTS:
        for n in COUNTS:
            rec = tr.arrangement(name, dims, n, seed=n % 89)
            want = check_density(f, rec, dims, (name, n))
            assert int(want.sum()) == live_count(rec) << 24
            if name == "one_cell" and n == 4099:                          # the 64-bit carry and the conversion's rounding are exercised
                assert int(want.max()) > 1 << 32 and int(want.max()) & 0xFFFF
            if name == "dead5" and n > 5:
                assert 0 < live_count(rec) < n
    # 2: a second call returns the same volume, not twice it
    rec = tr.arrangement("random", dims, 4099, seed=7)
    want = check_density(f, rec, dims, "first")
    assert np.array_equal(f.ParticleDensity(), want) and np.array_equal(f.ParticleDensity(), want)
    f.Release()


# ---- 3: the lab switch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(20, 20, 12), (36, 36, 1)])
def test_unmerged_adds_give_the_same_volume(dims, knob):
    """TRAIL_MERGE = 0 (a lab switch: the context runs on the lab build): every lane adds its own eight weights"""
    knob("TRAIL_MERGE", "0")
    f = make(dims)
    set_trail(f)
    for name in tr.ARRANGEMENTS:
        check_density(f, tr.arrangement(name, dims, 4099, seed=3), dims, name)
    f.Release()


@pytest.mark.parametrize("dims", [(20, 20, 12), (36, 36, 1)])
def test_wide_offset_kernels_match_the_model(dims, knob):
    """WIDE_OFFSETS = 1 (a lab switch) makes the launchers take the WIDE = true instantiations, which otherwise serve grids of 2^28 cells and
    more: 64-bit offsets are executed here, not driven beyond 2^32"""
    knob("WIDE_OFFSETS", "1")
    f = make(dims, storage="fp16")
    set_trail(f)
    rec = tr.arrangement("sorted", dims, 4099, seed=3)
    check_density(f, rec, dims, "wide")
    dt = pr.time_step(dims)
    col, _ = tr.fields(dims, 31, True)
    f.UpdateFrame(dt, 0)
    f.upload(fx.FIELD_COLOR, col)
    f.DepositParticles()
    f.Synchronize()
    assert same_bits(f.download(fx.FIELD_COLOR), tr.apply(tr.density(rec, dims), col, dt, TRAIL, half=True)[0])
    f.Release()


# ---- 4: the deposit against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES)
def test_the_deposit_is_the_models(dims, storage):
    half = storage == "fp16"
    dt = pr.time_step(dims)
    col, temp = tr.fields(dims, 17, half)
    f = make(dims, storage=storage)
    f.UpdateFrame(dt, 0)
    set_trail(f)
    for n in COUNTS:
        rec = np.concatenate([tr.arrangement("dead5", dims, n, seed=n % 89), tr.arrangement("one_cell", dims, n, seed=5)])
        rec[:n, :3] *= f32(0.5)                                            # (the random ones in one octant, so that cells stay untouched on every grid)
        acc = tr.density(rec, dims)
        untouched = acc == 0
        assert (untouched & np.signbit(col[..., 3])).any()                 # -0 stands in cells no particle touches
        f.SetParticles(rec)
        # buoyancy off: the colour alone
        f.SetBuoyancy(None)
        f.upload(fx.FIELD_COLOR, col)
        f.DepositParticles()
        f.Synchronize()
        want, _ = tr.apply(acc, col, dt, TRAIL, half=half)
        got = f.download(fx.FIELD_COLOR)
        assert same_bits(got, want), n
        assert same_bits(got[untouched], col[untouched]) and not same_bits(got[~untouched], col[~untouched])
        # buoyancy on: the temperature too; heat = 0 leaves it alone
        f.SetBuoyancy(**br.params(**BUOY))
        for t in (TRAIL, tr.trail(rate=3.0, tint=TRAIL["tint"])):
            set_trail(f, t)
            f.upload(fx.FIELD_COLOR, col); f.upload(fx.FIELD_TEMPERATURE, temp)
            f.DepositParticles()
            f.Synchronize()
            want, wtemp = tr.apply(acc, col, dt, t, temp=temp, half=half)
            assert same_bits(f.download(fx.FIELD_COLOR), want) and same_bits(f.download(fx.FIELD_TEMPERATURE), wtemp), (n, t["heat"])
            assert same_bits(wtemp, temp) == (t["heat"] == 0)
        set_trail(f)
        # the accumulator is all zero behind a deposit
        assert np.array_equal(f.ParticleDensity(), acc)
    f.Release()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", [(20, 20, 12), (36, 36, 1), (70, 70, 5)])
def test_solid_cells_take_nothing_and_keep_nothing(dims, storage):
    half = storage == "fp16"
    dt = pr.time_step(dims)
    col, temp = tr.fields(dims, 19, half)
    solid = pr.box_mask(dims)
    f = make(dims, storage=storage)
    f.UpdateFrame(dt, 0)
    set_trail(f)
    f.SetBuoyancy(**br.params(**BUOY))
    f.SetObstacles(solid)
    rec = tr.arrangement("random", dims, 4099, seed=23)
    acc = tr.density(rec, dims)
    inside = (solid != 0) & (acc != 0)
    assert inside.any() and ((solid == 0) & (acc != 0)).any()
    for bodies in ((), [dict(box_lo=(0.2, 0.2, 0.0), box_hi=(0.8, 0.8, 1.0), linear=(0.5, 0.0, 0.0), angular=(0.0, 0.0, 1.0))]):
        f.SetObstacleBodies(bodies)
        f.SetParticles(rec)
        f.upload(fx.FIELD_COLOR, col); f.upload(fx.FIELD_TEMPERATURE, temp)
        f.DepositParticles()
        f.Synchronize()
        want, wtemp = tr.apply(acc, col, dt, TRAIL, temp=temp, solid=solid, half=half)
        got, gtemp = f.download(fx.FIELD_COLOR), f.download(fx.FIELD_TEMPERATURE)
        assert same_bits(got, want) and same_bits(gtemp, wtemp), len(bodies)
        assert same_bits(got[inside], col[inside]) and same_bits(gtemp[inside], temp[inside])
        assert np.array_equal(f.ParticleDensity(), acc)                    # no remnant from the solid cells
    f.Release()


# ---- 5: what is deposited is what was asked for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(20, 20, 12), (256, 256, 6)])
def test_the_alpha_sum_is_the_amount_deposited(dims):
    dt = pr.time_step(dims)
    rec = tr.arrangement("dead5", dims, 4099, seed=29)
    t = tr.trail(rate=2.0, tint=(0.0, 0.0, 0.0, 0.75))
    f = make(dims)
    f.UpdateFrame(dt, 0)
    set_trail(f, t)
    f.SetParticles(rec)
    f.upload(fx.FIELD_COLOR, np.zeros(dims[::-1] + (4,), f32))
    f.DepositParticles()
    f.Synchronize()
    got = f.download(fx.FIELD_COLOR)
    want = live_count(rec) * (float(f32(2.0) * dt) * 0.75)
    err = abs(got[..., 3].astype(np.float64).sum() / want - 1)
    print("alpha sum: relative error %.3g" % err)
    assert err < 1e-6 and not got[..., :3].any()
    f.Release()


# ---- 6, 7: the step -------------------------------------------------------------------------------------------------------------------------
BODY = dict(box_lo=(0.2, 0.2, 0.0), box_hi=(0.8, 0.8, 1.0), linear=(0.5, 0.0, 0.0), angular=(0.0, 0.0, 1.0))


def run_steps(dims, storage, mode, steps=3, timing=False):
    """mode: "whole" = fx_simulate with a trail, "staged" = the stage calls in the step's order, "never" = no trail ever, "freed" = a trail set
    and switched off again before the first step -> (digests of the six fields and the temperature's bytes, the particles, launch counts)"""
    half = storage == "fp16"
    vel = pr.velocity(dims, 651, cells=0.6, half=half)
    col = np.random.default_rng(653).random((dims[2], dims[1], dims[0], 4)).astype(f32)
    col = col.astype(np.float16).astype(f32) if half else col
    f = make(dims, storage=storage, jacobi_iters=ITERS)
    if timing:
        f.timing_enable(True)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetAdvectionScheme("maccormack")
    f.SetEmitters([er.emitter((0.5, 0.3, 0.5), 0.2, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, 20.0, -3.0), swirl=30.0)])
    f.SetBuoyancy(**br.params(**BUOY))
    f.SetObstacles(pr.box_mask(dims))
    f.SetObstacleBodies([BODY])
    f.SetParticleSort(True, 2)
    f.SetParticles(pr.records(dims, 4099, 655))
    f.SetParticleParams("midpoint", (0.03, -0.4, 0.02), 0.7)
    if mode != "never":
        set_trail(f)
    if mode == "freed":
        f.SetParticleTrail(None)
        assert f.GetParticleTrail() == dict(rate=0.0, tint=(0.0, 0.0, 0.0, 0.0), heat=0.0, flags=0)
    dt = pr.time_step(dims)
    for i in range(steps):
        f.UpdateFrame(dt, i % 3)
        if mode == "staged":
            f.Advect(); f.OpenInflow(); f.Emit(); f.Heat(); f.DepositParticles(); f.EnforceObstacles(); f.ConfineVorticity()
            f.Divergence(); f.Jacobi(ITERS); f.Project()
            f.MoveParticles()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    digests = [f.digest(k) for k in ALL_FIELDS] + [f.download(fx.FIELD_TEMPERATURE).tobytes()]
    part = f.GetParticles()
    counts = None
    if timing:
        t = f.timing_read()
        counts = {k: getattr(t, k) for k, _ in capi.Timing._fields_ if not k.endswith("_ms")}
    f.Release()
    return digests, part, counts


@pytest.mark.parametrize("dims,storage", [((20, 20, 12), "fp32"), ((36, 36, 1), "fp16")])
def test_simulate_is_the_stage_calls_in_order_and_off_is_the_parent(dims, storage):
    whole, pw, _ = run_steps(dims, storage, "whole")
    staged, ps_, _ = run_steps(dims, storage, "staged")
    never, pn, _ = run_steps(dims, storage, "never")
    freed, pf, _ = run_steps(dims, storage, "freed")
    # 6: fx_simulate = the stage calls, the deposit between the buoyancy pass and the enforce pass
    assert whole == staged and same_bits(pw, ps_)
    # 7: never set = set then NULL, fields and particles; and the trail does change the fields
    assert never == freed and same_bits(pn, pf)
    assert whole[2] != never[2] and whole[6] != never[6]


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


def test_a_trail_costs_two_launches_and_off_costs_none():
    dims = (20, 20, 12)
    # fx_timing's launch counts: never set = set then NULL
    dn, pn, never = run_steps(dims, "fp32", "never", steps=6, timing=True)
    df, pf, freed = run_steps(dims, "fp32", "freed", steps=6, timing=True)
    _, _, whole = run_steps(dims, "fp32", "whole", steps=6, timing=True)
    assert dn == df and same_bits(pn, pf)                                  # the fields and the particle buffer after six steps
    assert never == freed and never["steps"] == 6 and never["jacobi_launches"] > 0
    assert whole == never                                                  # (fx_timing counts the solver's launches: the trail adds none there)
    # every launch of the step, counted in a captured step (captured, never replayed): a trail set = exactly two more
    f = make(dims, jacobi_iters=ITERS)
    f.upload(fx.FIELD_VELOCITY, pr.velocity(dims, 651, cells=0.6))
    f.SetBuoyancy(**br.params(**BUOY))
    f.SetParticles(pr.records(dims, 4099, 655))
    dt = pr.time_step(dims)
    f.UpdateFrame(dt, 0); f.Simulate(0)
    f.UpdateFrame(dt, 1)
    off = graph_nodes(f, 1)
    set_trail(f)
    f.UpdateFrame(dt, 2)
    on = graph_nodes(f, 2)
    f.SetParticleTrail(None)
    f.UpdateFrame(dt, 0)
    again = graph_nodes(f, 0)
    f.SetParticles(None)
    set_trail(f)
    f.UpdateFrame(dt, 1)
    no_set = graph_nodes(f, 1)
    f.Release()
    assert on == off + 2 and again == off and no_set == off - 1, (off, on, again, no_set)      # (no set: the move goes too, the trail adds nothing)


def rendered_rounds(accel):
    vp = (160, 120)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], (32, 32, 32), jacobi_iters=10)
    f.SetMaxSamples(48, 16)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    f.SetImpulse(0)
    rng = np.random.default_rng(77)
    rec = np.zeros((4099, 4), f32)
    rec[:, :3] = (0.5, 0.8, 0.45) + 0.08 * rng.standard_normal((4099, 3))  # high in the volume: the only smoke there is the trail's
    f.SetParticles(rec)
    f.SetParticleTrail(400.0, (0.9, 0.6, 0.3, 1.0))
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


def test_the_trail_reaches_the_accelerated_render():
    cube1, target1 = rendered_rounds(1)
    cube0, target0 = rendered_rounds(0)
    assert cube0[..., 3].max() > 0                                   # the cube map is not empty
    assert np.array_equal(cube1, cube0) and np.array_equal(target1, target0)


# ---- 8: status codes and round trips --------------------------------------------------------------------------------------------------------
def test_status_codes_and_round_trips():
    lib = capi.load()
    dims = (20, 20, 12)
    cells = dims[0] * dims[1] * dims[2]
    f = make(dims)
    off = dict(rate=0.0, tint=(0.0, 0.0, 0.0, 0.0), heat=0.0, flags=0)
    vol = np.full(cells, 77, np.uint64)
    ptr = vol.ctypes.data_as(C.POINTER(C.c_uint64))
    # the default: off -- the stage and the inspection call are FX_E_STATE, the getter reports it
    assert f.GetParticleTrail() == off
    assert lib.fx_deposit_particles(f._ctx, None) == capi.FX_E_STATE
    assert lib.fx_particle_density(f._ctx, None, ptr, vol.nbytes) == capi.FX_E_STATE and (vol == 77).all()
    rec = tr.arrangement("random", dims, 257, seed=23)
    f.SetParticles(rec)
    assert lib.fx_deposit_particles(f._ctx, None) == capi.FX_E_STATE
    # round trips
    set_trail(f)
    mine = dict(rate=3.0, tint=(0.25, -0.5, 0.125, 0.7), heat=-2.5, flags=0)
    got = f.GetParticleTrail()
    assert got == dict(mine, tint=tuple(float(f32(v)) for v in mine["tint"]))
    mine = got
    want = tr.density(rec, dims)
    assert np.array_equal(f.ParticleDensity(), want)
    # refused, the previous state staying in force
    nan, inf = float("nan"), float("inf")
    for change in (dict(struct_size=28), dict(struct_size=36), dict(flags=1), dict(flags=0x80000000), dict(rate=-1e-30), dict(rate=nan), dict(rate=inf),
                   dict(heat=nan), dict(heat=-inf), dict(tint=(0, nan, 0, 0)), dict(tint=(0, 0, 0, inf)), dict(tint=(-inf, 0, 0, 0))):
        q = capi.ParticleTrail(32, 0, 1.0, (C.c_float * 4)(1, 1, 1, 1), 1.0)
        for k, v in change.items():
            setattr(q, k, (C.c_float * 4)(*v) if k == "tint" else v)
        assert lib.fx_set_particle_trail(f._ctx, C.byref(q)) == capi.FX_E_INVALID and f.GetParticleTrail() == mine, change
    assert lib.fx_get_particle_trail(f._ctx, None) == capi.FX_E_INVALID
    for bytes_ in (0, vol.nbytes - 8, vol.nbytes + 8, cells * 4):
        assert lib.fx_particle_density(f._ctx, None, ptr, bytes_) == capi.FX_E_INVALID and (vol == 77).all()
    assert lib.fx_particle_density(f._ctx, None, None, vol.nbytes) == capi.FX_E_INVALID
    assert np.array_equal(f.ParticleDensity(), want)
    # accepted: rate 0, a negative heat, a negative tint
    f.SetParticleTrail(0.0, (-1.0, 0.0, 0.0, 0.0), -3.0)
    assert f.GetParticleTrail()["rate"] == 0.0 and f.GetParticleTrail()["heat"] == -3.0
    set_trail(f)
    # configuration on the emitters' terms: kept across UpdateFrame, not digested; dt = 0 deposits nothing
    f.UpdateFrame(f32(0.0), 1)
    f.Simulate(1)
    before = [f.digest(k) for k in ALL_FIELDS]
    f.DepositParticles()
    assert f.GetParticleTrail() == mine and before == [f.digest(k) for k in ALL_FIELDS]
    # no set: FX_OK and nothing done, the density is zeros
    f.SetParticles(None)
    f.UpdateFrame(pr.time_step(dims), 2)
    before = [f.digest(k) for k in ALL_FIELDS]
    f.DepositParticles()
    assert before == [f.digest(k) for k in ALL_FIELDS] and not f.ParticleDensity().any()
    # NULL is the default again
    f.SetParticleTrail(None)
    assert f.GetParticleTrail() == off and lib.fx_deposit_particles(f._ctx, None) == capi.FX_E_STATE
    assert lib.fx_particle_density(f._ctx, None, ptr, vol.nbytes) == capi.FX_E_STATE and (vol == 77).all()
    # slab ranks: the setter and the stages refuse, the getter reports the default
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    big = np.zeros(32 * 32 * 32, np.uint64)
    for r in ranks:
        q = capi.ParticleTrail(32, 0, 1.0, (C.c_float * 4)(1, 1, 1, 1), 1.0)
        assert lib.fx_set_particle_trail(r._ctx, C.byref(q)) == capi.FX_E_INVALID and lib.fx_set_particle_trail(r._ctx, None) == capi.FX_E_INVALID
        assert lib.fx_deposit_particles(r._ctx, None) == capi.FX_E_INVALID
        assert lib.fx_particle_density(r._ctx, None, big.ctypes.data_as(C.POINTER(C.c_uint64)), big.nbytes) == capi.FX_E_INVALID
        assert r.GetParticleTrail() == off
    # a render-only context: FX_E_STATE, whatever else is wrong with the call
    ro = fx.Fluid()
    assert ro.Init(64, 64, (32, 32, 8), render_only=True)
    q = capi.ParticleTrail(32, 0, 1.0, (C.c_float * 4)(1, 1, 1, 1), 1.0)
    assert lib.fx_set_particle_trail(ro._ctx, C.byref(q)) == capi.FX_E_STATE and lib.fx_get_particle_trail(ro._ctx, C.byref(q)) == capi.FX_E_STATE
    assert lib.fx_deposit_particles(ro._ctx, None) == capi.FX_E_STATE and lib.fx_particle_density(ro._ctx, None, ptr, 8) == capi.FX_E_STATE
    assert q.rate == 1.0 and (vol == 77).all()
    # Release() with the accumulator allocated is clean
    g = make(dims)
    set_trail(g)
    g.SetParticles(rec)
    for o in [f, ro, g] + ranks:
        o.Release()


# ---- 9: the C++ wrapper -------------------------------------------------------------------------------------------------------------------
CXX = r'''
#include "Fluid.hpp"
#include <cstdio>
using namespace fluidx;
int main(int argc, char** argv)
{
	if (argc < 3) return 2;
	const XMUINT3 grid = { 20, 20, 12 };
	Fluid::Options opt;
	opt.storage = FX_STORAGE_FP32; opt.jacobiIters = 4; opt.jacobiMode = FX_JACOBI_FIXED;
	Fluid fluid;
	if (!fluid.Init(nullptr, 0, 0, grid, opt)) return 3;
	std::vector<float> rec;
	FILE* in = std::fopen(argv[1], "rb");
	if (!in) return 4;
	float r[4];
	while (std::fread(r, sizeof r, 1, in) == 1) rec.insert(rec.end(), r, r + 4);
	std::fclose(in);
	std::vector<uint64_t> vol((size_t)20 * 20 * 12, 5u);
	if (fluid.DepositParticles() || fluid.LastStatus() != FX_E_STATE) return 5;                       // off by default
	if (fluid.ParticleDensity(vol.data(), vol.size() * 8) || fluid.LastStatus() != FX_E_STATE || vol[0] != 5u) return 6;
	const float tint[4] = { 0.25f, -0.5f, 0.125f, 0.7f };
	if (!fluid.SetParticles(rec) || !fluid.SetParticleTrail(3.0f, tint, -2.5f)) return 7;
	fx_particle_trail t = {};
	if (!fluid.GetParticleTrail(t) || t.struct_size != 32 || t.rate != 3.0f || t.tint[3] != 0.7f || t.heat != -2.5f) return 8;
	if (fluid.ParticleDensity(vol.data(), 8) || fluid.LastStatus() != FX_E_INVALID) return 9;
	if (!fluid.DepositParticles()) return 10;                                                           // (dt = 0 so far: nothing)
	if (!fluid.ParticleDensity(vol.data(), vol.size() * 8)) return 11;
	if (!fluid.SetParticleTrail(nullptr) || !fluid.GetParticleTrail(t) || t.rate != 0.0f || t.heat != 0.0f) return 12;
	FILE* f = std::fopen(argv[2], "wb");
	if (!f || std::fwrite(vol.data(), 8, vol.size(), f) != vol.size()) return 13;
	return std::fclose(f) ? 14 : 0;
}
'''


def test_the_cxx_wrapper_deposits(tmp_path):
    from fluidx12_amd import build as fxbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cc)
    libdir = os.path.dirname(fxbuild.ensure_built())
    dims = (20, 20, 12)
    rec = tr.arrangement("dead5", dims, 4099, seed=41)
    src, exe, inp, out = tmp_path / "trail.cpp", str(tmp_path / "trail"), str(tmp_path / "rec.bin"), str(tmp_path / "vol.bin")
    src.write_text(CXX)
    rec.tofile(inp)
    subprocess.run([cc, "-std=c++17", "-O1", "-I", os.path.join(root, "fluidx12_amd", "csrc"), str(src), "-o", exe, "-L" + libdir, "-lfluidx_hip",
                    "-Wl,-rpath," + libdir], check=True, timeout=300)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)        # a fresh child process, under its own time limit
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert np.array_equal(np.fromfile(out, np.uint64).reshape(dims[::-1]), tr.density(rec, dims))
