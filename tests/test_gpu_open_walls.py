"""Open walls on the GPU (fx_set_open_walls / fx_get_open_walls / fx_open_inflow, csrc/fx_open.hip; the faces argument of k_heat).

Everything here is bit for bit against the numpy model tests/open_ref.py (tests/test_open_ref.py anchors it to the obstacle reference and to
buoyancy_ref) -- the sweeps and the projection, with and without a mask; the inflow pass; the buoyancy pass with a ghost at ambient;
fx_simulate against the stage calls; faces = 0 against a context that never heard of the call; the accelerated render against the plain one
-- with one exception: the plume, which holds the device to the two inequalities of the CPU test (the smoke leaves through an open lid and
piles up under a closed one).

Shapes (X = Y, Z), the obstacle suite's: (20, 5) scalar with a row shorter than a tile, (150, 6) scalar 3-D with X % 4 != 0, (36, 1) and
(150, 1) 2-D, (64, 8) the wide sweep, (68, 5) with a partial wave, (256, 6) one wave per row, (320, 4) wave seams inside a row."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import buoyancy_ref as br
import emitter_ref as er
import open_ref as orf
import test_obstacle_ref as ob
from test_obstacle_ref import random_mask, ref_divergence, ref_enforce

pytestmark = pytest.mark.gpu
f32 = np.float32

SCALAR = [(20, 20, 5), (150, 150, 6), (36, 36, 1), (150, 150, 1)]
V4 = [(64, 64, 8), (68, 68, 5), (256, 256, 6), (320, 320, 4)]
INFLOW = [(20, 20, 5), (150, 150, 6), (36, 36, 1), (320, 320, 4)]
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status        # simulation only: no viewport
    return f


def time_step(dims):
    return f32((2.0 if dims[2] > 1 else 1.0) / dims[1])   # Fluid.default_time_step


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def rand_state(dims, seed, half=False, scale=0.5):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vel = (rng.standard_normal((3, Z, Y, X)) * scale).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    if half:
        vel, col = vel.astype(np.float16).astype(f32), col.astype(np.float16).astype(f32)
    return vel, col, p


def trace_state(dims, seed, half=False, cells=1.2):
    """a VELOCITY whose back-traces move `cells` cells (standard deviation) along every axis -- at a face some leave by less than a cell,
    some by more --, a colour in [0, 1) and a temperature around the ambient value"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    dt = time_step(dims)
    vel0 = rng.standard_normal((3, Z, Y, X))
    for a, n in enumerate(dims):
        vel0[a] *= cells / (float(dt) * n)
    vel0 = vel0.astype(f32)
    vel1 = rng.standard_normal((3, Z, Y, X)).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    T = (rng.random((Z, Y, X)) * 4 - 1).astype(f32)
    if half:
        vel0, vel1, col = (a.astype(np.float16).astype(f32) for a in (vel0, vel1, col))
    return T, vel0, vel1, col


# ---- 1: the sweeps and the projection against the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", SCALAR + V4)
def test_stages_match_the_model_bit_for_bit(dims, storage):
    """Jacobi(5) and Project() the way tests/test_gpu_obstacles.py `stages` runs them.  The divergence is the obstacle suite's (unchanged)."""
    half = storage == "fp16"
    vel, col, p = rand_state(dims, 501, half)
    f = make(dims, storage=storage, jacobi_iters=5)
    f.UpdateFrame(time_step(dims), 0)
    for name, m in (("none", None), ("random", random_mask(dims))):
        f.SetObstacles(m)
        f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col)
        f.EnforceObstacles()
        f.Divergence()
        b = f.download(fx.FIELD_DIVERGENCE)
        wv = ref_enforce(vel, col, m)[0] if m is not None else vel
        wb = ref_divergence(wv, m if m is not None else np.zeros(p.shape, np.uint8))
        assert same_bits(b, wb), name
        closed_q = orf.ref_jacobi(p, wb, m, 0, 5)
        closed_out = orf.ref_project(wv, closed_q, m, 0, half)
        for faces in orf.face_sets(dims):
            f.SetOpenWalls(faces)
            assert f.GetOpenWalls() == faces
            f.upload(fx.FIELD_PRESSURE, p)
            f.Jacobi(5)
            q = f.download(fx.FIELD_PRESSURE)
            f.Project()
            out = f.download(fx.FIELD_VELOCITY)
            wq = orf.ref_jacobi(p, wb, m, faces, 5)
            assert same_bits(q, wq), (name, faces)
            assert same_bits(out, orf.ref_project(wv, wq, m, faces, half)), (name, faces)
            assert not same_bits(q, closed_q) and not same_bits(out, closed_out), (name, faces)       # the rule took part
        f.SetOpenWalls(0)
        f.upload(fx.FIELD_PRESSURE, p)
        f.Jacobi(5)
        assert same_bits(f.download(fx.FIELD_PRESSURE), closed_q), name
    f.Release()


@pytest.mark.parametrize("dims", V4)
def test_the_wide_sweep_is_the_scalar_sweep(dims, knob):
    """every legal face open, with and without a mask: seven sweeps as built (the wide kernel), then on the lab build with the scalar one"""
    faces = orf.legal_faces(dims)
    masks = [None, random_mask(dims, seed=17)]
    _, _, p = rand_state(dims, 311)
    b = np.random.default_rng(313).standard_normal(p.shape).astype(f32)

    def sweeps(m):
        f = make(dims, jacobi_iters=7)
        f.SetObstacles(m)
        f.SetOpenWalls(faces)
        f.upload(fx.FIELD_PRESSURE, p); f.upload(fx.FIELD_DIVERGENCE, b)
        f.Jacobi(7)
        out = f.download(fx.FIELD_PRESSURE)
        f.Release()
        return out
    wide = [sweeps(m) for m in masks]
    knob("OBSTACLE_V4", "0")                                          # (a lab switch: the contexts from here on run on the lab build)
    scalar = [sweeps(m) for m in masks]
    for m, w, s in zip(masks, wide, scalar):
        want = orf.ref_jacobi(p, b, m, faces, 7)
        assert same_bits(w, want) and same_bits(s, want), m is not None


# ---- 2: the inflow pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", INFLOW)
def test_inflow_matches_the_model_bit_for_bit(dims, storage, address):
    half = storage == "fp16"
    _, vel0, vel1, col = trace_state(dims, 503, half)
    dt = time_step(dims)
    f = make(dims, storage=storage, advect_address=address)
    f.UpdateFrame(dt, 0)
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_VELOCITY1, vel1)
    for faces in orf.face_sets(dims):
        f.SetOpenWalls(faces)
        f.upload(fx.FIELD_COLOR, col)
        f.OpenInflow()
        got = f.download(fx.FIELD_COLOR)
        w = orf.inflow_weights(vel0, dt, faces)
        assert (w == 0).any() and ((w > 0) & (w < 1)).any() and (w == 1).any(), faces      # traces that leave by more than a cell, by less, not at all
        assert same_bits(got, orf.ref_inflow(col, vel0, dt, faces, half)), faces
        assert same_bits(got[w == 1], col[w == 1])
    assert same_bits(f.download(fx.FIELD_VELOCITY), vel0) and same_bits(f.download(fx.FIELD_VELOCITY1), vel1)      # the colour only
    # nothing to do: all walls closed, or dt = 0
    f.SetOpenWalls(0)
    f.upload(fx.FIELD_COLOR, col)
    f.OpenInflow()
    assert same_bits(f.download(fx.FIELD_COLOR), col)
    f.SetOpenWalls(orf.legal_faces(dims))
    f.UpdateFrame(0.0, 1)
    f.upload(fx.FIELD_COLOR, col)
    f.OpenInflow()
    assert same_bits(f.download(fx.FIELD_COLOR), col)
    f.Release()


def rendered_rounds(accel, faces):
    vp = (160, 120)
    dims = (32, 32, 32)
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], dims, jacobi_iters=10)
    f.SetMaxSamples(48, 16)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    f.SetOpenWalls(faces)
    # smoke right under the lid, pushed down: the back-traces of the top layers leave through the face
    f.SetEmitters([er.emitter((0.5, 0.93, 0.5), 0.15, color_rate=(8.0, 16.0, 40.0, 40.0), force=(0.0, -40.0, 0.0), swirl=0.0)])
    view, proj, eye = fx.default_camera(*vp)
    dt = f32(f.default_time_step())
    for k in range(5):                                               # from the second step on the advection writes the alpha volume
        f.UpdateFrame(dt, k % 3, view, proj, eye)
        f.Simulate(k % 3)
        f.ClearRenderTarget()
        f.Render(k % 3, fx.Fluid.OPTIMIZED)
        f.RenderCube(k % 3)
    f.Synchronize()
    out = f.download(fx.FIELD_CUBEMAP), f.download(fx.FIELD_TARGET), f.download(fx.FIELD_COLOR)
    f.Release()
    return out


def test_the_accelerated_render_sees_the_scaled_colour():
    cube1, target1, col1 = rendered_rounds(1, orf.Y_HI)
    cube0, target0, col0 = rendered_rounds(0, orf.Y_HI)
    assert cube0[..., 3].max() > 0 and same_bits(col1, col0)
    assert np.array_equal(cube1, cube0) and np.array_equal(target1, target0)
    assert not same_bits(col0, rendered_rounds(0, 0)[2])              # ... and the pass had smoke to scale


# ---- 3: the buoyancy pass with a ghost at ambient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(20, 20, 5), (36, 36, 1)])
def test_heat_with_open_faces_matches_the_model_bit_for_bit(dims, storage, address):
    """no heat sources: no transcendental, so no cell is excluded"""
    half = storage == "fp16"
    T, vel0, vel1, col = trace_state(dims, 509, half)
    dt = time_step(dims)
    prm = br.params(ambient=0.25, density_weight=0.5, lift=2.0, cooling=0.3, up=(0.2, 1.0, -0.1))
    solid = random_mask(dims, seed=7, p=0.1)
    f = make(dims, storage=storage, advect_address=address)
    f.SetBuoyancy(**prm)
    f.UpdateFrame(dt, 0)
    for mask in (None, solid):
        f.SetObstacles(mask)
        for faces in orf.face_sets(dims) + [0]:
            f.SetOpenWalls(faces)
            f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_VELOCITY1, vel1); f.upload(fx.FIELD_COLOR, col); f.upload(fx.FIELD_TEMPERATURE, T)
            f.Heat()
            gT, gv = f.download(fx.FIELD_TEMPERATURE), f.download(fx.FIELD_VELOCITY1)
            wT, wv = orf.heat_apply(T, vel0, vel1, col, prm, [], dt, address, half=half, solid=mask, faces=faces)
            assert same_bits(gT, wT) and same_bits(gv, wv), (faces, mask is not None)
            if faces:
                assert not same_bits(gT, br.apply(T, vel0, vel1, col, prm, [], dt, address, half=half, solid=mask)[0]), faces
    f.Release()


# ---- 4: fx_simulate is the composition of the stage calls -------------------------------------------------------------------------------
PRM = br.params(ambient=0.1, density_weight=0.4, lift=3.0, cooling=0.2, up=(0.1, 1.0, -0.2))
EMITTER = [er.emitter((0.4, 0.8, 0.5), 0.25, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, 40.0, -3.0), swirl=30.0)]


def run_steps(dims, staged, faces, steps=3, **kw):
    _, vel0, _, col = trace_state(dims, 521, half=kw.get("storage") == "fp16", cells=0.6)
    f = make(dims, **kw)
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)
    f.SetEmitters(EMITTER)
    f.SetObstacles(ob.ball_mask(dims, center=(0.5, 0.3, 0.5), radius=0.12))
    f.SetBuoyancy(**PRM)
    f.SetHeatSources(br.list_a()[:3])
    if faces is not None:
        f.SetOpenWalls(faces)
    dt = time_step(dims)
    for i in range(steps):
        f.UpdateFrame(dt, i % 3)
        if staged:
            f.Advect(); f.OpenInflow(); f.Emit(); f.Heat(); f.EnforceObstacles()
            f.Divergence(); f.Jacobi(kw["jacobi_iters"]); f.Project()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS], f.download(fx.FIELD_TEMPERATURE)
    f.Release()
    return out


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(64, 64, 8), (150, 150, 6)])
def test_simulate_is_the_stage_composition(dims, storage):
    kw = dict(storage=storage, jacobi_iters=10)
    faces = orf.Y_HI | orf.X_LO | orf.Z_HI
    whole, T_whole = run_steps(dims, False, faces, **kw)
    parts, T_parts = run_steps(dims, True, faces, **kw)
    assert whole == parts and same_bits(T_whole, T_parts)
    closed, T_closed = run_steps(dims, False, None, **kw)            # (and the open walls took part, in every field they reach)
    for k in (0, 2, 4):
        assert whole[k] != closed[k], k
    assert not same_bits(T_whole, T_closed)


# ---- 5: the setter --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(64, 64, 8), (36, 36, 1)])
def test_closing_the_walls_again_is_never_having_opened_them(dims):
    _, vel0, _, col = trace_state(dims, 523, cells=0.6)
    a, b = make(dims, jacobi_iters=10), make(dims, jacobi_iters=10)
    b.SetOpenWalls(orf.legal_faces(dims))
    b.SetOpenWalls(0)
    assert b.GetOpenWalls() == 0 and a.GetOpenWalls() == 0
    for f in (a, b):
        f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)
        dt = time_step(dims)
        for k in range(3):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.OpenInflow()                                               # nothing
        f.Synchronize()
    assert [a.digest(k) for k in ALL_FIELDS] == [b.digest(k) for k in ALL_FIELDS]
    b.SetOpenWalls(orf.Y_HI)                                         # set again: in force again
    for f in (a, b):
        f.UpdateFrame(time_step(dims), 0); f.Simulate(0)
    assert a.digest(fx.FIELD_VELOCITY) != b.digest(fx.FIELD_VELOCITY)
    a.Release(); b.Release()


def test_status_codes():
    lib = capi.load()
    dims = (32, 32, 8)
    f = make(dims, jacobi_iters=6)
    got = C.c_uint32(99)
    assert lib.fx_get_open_walls(f._ctx, C.byref(got)) == capi.FX_OK and got.value == 0                 # the default
    for faces in list(range(0x40)) + [0x15]:
        assert lib.fx_set_open_walls(f._ctx, faces) == capi.FX_OK
        assert lib.fx_get_open_walls(f._ctx, C.byref(got)) == capi.FX_OK and got.value == faces        # round trip
    for bad in (0x40, 0x80, 0x55, 0x100, 0x80000000, 0xFFFFFFFF):
        assert lib.fx_set_open_walls(f._ctx, bad) == capi.FX_E_INVALID and f.GetOpenWalls() == 0x15    # the previous setting stays in force
    assert lib.fx_get_open_walls(f._ctx, None) == capi.FX_E_INVALID
    assert lib.fx_set_open_walls(None, 1) == capi.FX_E_INVALID and lib.fx_open_inflow(None, None) == capi.FX_E_INVALID
    # timing: one sweep per launch with a face open, with or without a mask
    f.SetOpenWalls(orf.Y_HI)
    for mask in (None, random_mask(dims, seed=23)):
        f.SetObstacles(mask)
        f.timing_enable(True)
        f.timing_read(True)
        f.UpdateFrame(time_step(dims), 0)
        f.Simulate(0); f.Jacobi(9)
        f.Synchronize()
        t = f.timing_read()
        assert t.jacobi_launches == t.jacobi_sweeps == 6 + 9
        f.timing_enable(False)
    # configuration: kept across UpdateFrame, not digested
    before = sorted(f.digest(k) for k in ALL_FIELDS)
    f.SetOpenWalls(orf.X_LO | orf.Z_HI)
    f.UpdateFrame(f32(0.05), 2)
    assert f.GetOpenWalls() == (orf.X_LO | orf.Z_HI) and before == sorted(f.digest(k) for k in ALL_FIELDS)
    # a z bit on a 2-D grid
    flat = make((36, 36, 1))
    flat.SetOpenWalls(orf.X_HI | orf.Y_LO)
    for bad in (orf.Z_LO, orf.Z_HI, orf.ALL_3D, orf.Z_LO | orf.X_LO):
        assert lib.fx_set_open_walls(flat._ctx, bad) == capi.FX_E_INVALID and flat.GetOpenWalls() == (orf.X_HI | orf.Y_LO)
    flat.SetOpenWalls(orf.ALL_2D)
    # faithful contexts
    fa = make(dims, jacobi_iters=16, jacobi_mode="faithful")
    assert lib.fx_set_open_walls(fa._ctx, orf.Y_HI) == capi.FX_E_INVALID and fa.GetOpenWalls() == 0
    assert lib.fx_set_open_walls(fa._ctx, 0x40) == capi.FX_E_INVALID
    with pytest.raises(fx.FluidxError):
        fa.SetOpenWalls(orf.Y_HI)
    # slab ranks: a lone slab context, and the members of an in-process group
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    for r in ranks:
        assert lib.fx_set_open_walls(r._ctx, orf.Y_HI) == capi.FX_E_INVALID and r.GetOpenWalls() == 0
    fx.comm_init_local(ranks)
    for r in ranks:
        assert lib.fx_set_open_walls(r._ctx, orf.Y_HI) == capi.FX_E_INVALID and r.GetOpenWalls() == 0
        assert lib.fx_open_inflow(r._ctx, None) == capi.FX_E_INVALID
    ro = fx.Fluid()
    assert ro.Init(64, 64, dims, render_only=True)
    assert lib.fx_set_open_walls(ro._ctx, orf.Y_HI) == capi.FX_E_STATE and lib.fx_set_open_walls(ro._ctx, 0) == capi.FX_E_STATE
    assert lib.fx_set_open_walls(ro._ctx, 0x40) == capi.FX_E_STATE               # ... whatever else is wrong with the call
    assert lib.fx_get_open_walls(ro._ctx, C.byref(got)) == capi.FX_E_STATE and lib.fx_open_inflow(ro._ctx, None) == capi.FX_E_STATE
    for o in [f, flat, fa, ro] + ranks:
        o.Release()


# ---- 6: the plume -----------------------------------------------------------------------------------------------------------------------------
def test_the_smoke_leaves_through_an_open_lid():
    """the settings of tests/test_open_ref.py::test_the_smoke_leaves_through_an_open_lid on the device: 32^3 fp32, dt = 1/60, 40 sweeps, the
    built-in impulse on for 120 steps and off for 120 more; Y+ open against a closed box"""
    import test_open_ref as cpu
    sums = {}
    for name, faces in (("open", orf.Y_HI), ("closed", 0)):
        f = make(cpu.PLUME_DIMS, jacobi_iters=cpu.PLUME_ITERS)
        f.SetOpenWalls(faces)
        dt = f32(cpu.PLUME_DT)
        for k in range(cpu.PLUME_STEPS):
            if k == cpu.PLUME_ON:
                f.SetImpulse(0)
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
            if k + 1 in (cpu.PLUME_ON, cpu.PLUME_STEPS):
                sums[name, k + 1] = float(f.download(fx.FIELD_COLOR)[..., 3].astype(np.float64).sum())
        f.Release()
    o120, o240, c120, c240 = sums["open", 120], sums["open", 240], sums["closed", 120], sums["closed", 240]
    print("sum alpha  open: step 120 %.3f  step 240 %.3f   closed: step 120 %.3f  step 240 %.3f" % (o120, o240, c120, c240))
    assert o240 < 0.25 * o120
    assert c240 > 10 * o240
