"""Moving obstacles on the GPU (fx_set_obstacle_bodies / fx_get_obstacle_bodies, csrc/fx_obstacle.hip).

Every comparison is bit for bit against the numpy model tests/moving_obstacle_ref.py (tests/test_moving_obstacle_ref.py anchors it to the
resting obstacles' reference): the three stages that see the bodies and the sweeps between them, with closed walls and with two open ones;
fx_simulate against the stage calls and against the model's step; bodies that hold no solid cell and an empty list against a context that
never heard of the call; bodies that stand still against the empty list; a ball that is voxelised anew every frame.  The model's step starts behind the stages the bodies do not touch
(advection, inflow, emitters, buoyancy, confinement): those run on the device, and what they leave is what the model continues from.

Shapes (X = Y, Z): (20, 5) a row shorter than a tile, (36, 1) 2-D, (68, 5) X % 64 != 0 with the wide sweep, (64, 8) the wide sweep on full
waves, (150, 6) scalar sweeps with X % 4 != 0 and three tiles a row."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import build as fxbuild
from fluidx12_amd import capi

import buoyancy_ref as br
import emitter_ref as er
import moving_obstacle_ref as mv
import open_ref as orf
from test_obstacle_ref import ball_mask, ref_codes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

GRIDS = [(20, 20, 5), (36, 36, 1), (68, 68, 5), (64, 64, 8), (150, 150, 6)]
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
OPEN = orf.Y_HI | orf.X_LO


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


def cells_box(dims, x, y, z):
    """the box that holds exactly the cells x[0]..x[1], y[0]..y[1], z[0]..z[1]: its bounds are cell bounds, the centres lie strictly inside"""
    X, Y, Z = dims
    return (x[0] / X, y[0] / Y, z[0] / Z), ((x[1] + 1.0) / X, (y[1] + 1.0) / Y, (z[1] + 1.0) / Z)


def scene(dims):
    """-> (mask, bodies): every case of the rules in one grid, in the corner every grid has (16 x 20 cells) and at the far walls
      A  touches the walls x = 0 and (3-D) z = 0, z = Z - 1: the clamped neighbour of its outer cells is the cell itself; it translates
      B, C  one fluid cell apart (x = 11) with different velocities: that cell's u_x is their mean; C rotates about all three axes
      D  its box overlaps C's and comes later in the list: the shared cells are C's
      E  in the far corner, against x = X - 1 and y = Y - 1, across the last tile's tail; it translates
      two solid cells in no box: they rest
      grids of 36 cells and more: a ball that spins about a pivot off its centre"""
    X, Y, Z = dims
    m = np.zeros((Z, Y, X), np.uint8)
    zs = (1, Z - 2) if Z > 2 else (0, Z - 1)
    zsl = slice(zs[0], zs[1] + 1)
    bodies = []
    m[:, 3:8, 0:3] = 1
    bodies.append(mv.body(*cells_box(dims, (0, 2), (3, 7), (0, Z - 1)), linear=(0.3, -0.2, 0.1)))
    m[zsl, 10:14, 8:11] = 1
    bodies.append(mv.body(*cells_box(dims, (8, 10), (10, 13), zs), linear=(-0.4, 0.25, 0.0)))
    m[zsl, 10:14, 12:15] = 1
    bodies.append(mv.body(*cells_box(dims, (12, 14), (10, 13), zs), linear=(0.1, 0.0, -0.2), angular=(1.5, -2.5, 6.0)))
    m[zsl, 12:16, 15:17] = 1
    bodies.append(mv.body(*cells_box(dims, (13, 16), (10, 15), zs), linear=(0.0, 0.6, 0.3)))
    m[zsl, Y - 6:Y, X - 2:X] = 1
    bodies.append(mv.body(*cells_box(dims, (X - 2, X - 1), (Y - 6, Y - 1), zs), linear=(-0.5, -0.35, 0.15)))
    m[zsl, 1:3, X - 4:X - 2] = 1
    if X >= 36:
        ball = ball_mask(dims, center=(0.7, 0.6, 0.5), radius=0.12)
        m |= ball
        bodies.append(mv.body((0.57, 0.47, 0.0), (0.83, 0.73, 1.0), linear=(0.05, 0.0, 0.0), angular=(-3.0, 2.0, 5.0), pivot=(0.66, 0.62, 0.45)))
    who = mv.body_of((Z, Y, X), bodies)
    solid = m.astype(bool)
    assert (solid & (who < 0)).sum() == 4 * (zs[1] - zs[0] + 1)                 # the resting cells
    assert all((solid & (who == k)).any() for k in range(len(bodies)))          # every body holds solid cells
    return m, bodies


def bodies_equal(got, want):
    keys = ("box_lo", "box_hi", "linear", "angular", "pivot")
    return len(got) == len(want) and all(tuple(f32(v) for v in g[k]) == tuple(f32(v) for v in w[k]) for g, w in zip(got, want) for k in keys)


# ---- 1: the stages against the model, closed walls and two open ones ----------------------------------------------------------------------
@pytest.mark.parametrize("faces", [0, OPEN], ids=["closed", "open"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", GRIDS)
def test_stages_match_the_model_bit_for_bit(dims, storage, faces):
    half = storage == "fp16"
    vel, col, p = rand_state(dims, 601, half)
    m, bodies = scene(dims)
    f = make(dims, storage=storage, jacobi_iters=5)
    f.SetObstacleBodies(bodies)                                      # before the mask: the order does not matter
    f.SetObstacles(m)
    f.SetOpenWalls(faces)
    assert bodies_equal(f.GetObstacleBodies(), bodies)
    f.UpdateFrame(time_step(dims), 0)
    f.upload(fx.FIELD_VELOCITY1, vel); f.upload(fx.FIELD_COLOR, col); f.upload(fx.FIELD_PRESSURE, p)
    f.EnforceObstacles()
    v1, c1 = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.Divergence()
    b = f.download(fx.FIELD_DIVERGENCE)
    f.Jacobi(5)
    q = f.download(fx.FIELD_PRESSURE)
    f.Project()
    out = f.download(fx.FIELD_VELOCITY)
    f.Release()
    wv, wc = mv.ref_enforce(vel, col, m, bodies, half)
    assert same_bits(v1, wv) and same_bits(c1, wc), "enforce"
    wb = mv.ref_divergence(wv, m, bodies)
    assert same_bits(b, wb), "divergence"
    wq = mv.ref_jacobi(p, wb, m, faces, 5)
    assert same_bits(q, wq), "relaxation"
    assert same_bits(out, mv.ref_project(wv, wq, m, bodies, faces, half)), "projection"
    # the bodies took part in each of the three
    rv, _ = mv.ref_enforce(vel, col, m, [], half)
    assert not same_bits(v1, rv) and not same_bits(b, mv.ref_divergence(wv, m, [])) and not same_bits(out, mv.ref_project(wv, wq, m, [], faces, half))
    # ... and the cases of the scene are in it: a fluid cell between two solids, a solid cell that is its own clamped neighbour
    code = ref_codes(m)
    assert ((code & 0x43) == 0x03).any() and (code[:, :, 0] & 0x41 == 0x41).any()


# ---- 2: whole steps ---------------------------------------------------------------------------------------------------------------------------
PRM = br.params(ambient=0.1, density_weight=0.4, lift=3.0, cooling=0.2, up=(0.1, 1.0, -0.2))
EMITTER = [er.emitter((0.4, 0.8, 0.5), 0.25, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, 40.0, -3.0), swirl=30.0)]


def configure(f, extras, faces):
    f.SetOpenWalls(faces)
    if extras:
        f.SetEmitters(EMITTER)
        f.SetBuoyancy(**PRM)
        f.SetHeatSources(br.list_a()[:3])
        f.SetVorticityConfinement(4.0)


def steps_against_the_model(dims, storage, frames, extras=False, faces=0, iters=8, state=None, impulse=True):
    """`frames` = [(mask, bodies)] per step.  Context a runs fx_simulate; context b runs the stage calls, and behind each of its stages
    that sees the bodies the model's result, computed from what b's previous stages left, is compared bit for bit.  Both end in the same
    fields.  -> a's final velocity"""
    half = storage == "fp16"
    a, b = make(dims, storage=storage, jacobi_iters=iters), make(dims, storage=storage, jacobi_iters=iters)
    for f in (a, b):
        configure(f, extras, faces)
        f.SetImpulse(1 if impulse else 0)
        if state is not None:
            f.upload(fx.FIELD_VELOCITY, state[0]); f.upload(fx.FIELD_COLOR, state[1])
    dt = time_step(dims)
    for k, (mask, bodies) in enumerate(frames):
        for f in (a, b):
            f.SetObstacles(mask)
            f.SetObstacleBodies(bodies)
            f.UpdateFrame(dt, k % 3)
        a.Simulate(k % 3)
        p0 = b.download(fx.FIELD_PRESSURE)
        b.Advect(); b.OpenInflow(); b.Emit(); b.Heat()
        av, ac = b.download(fx.FIELD_VELOCITY1), b.download(fx.FIELD_COLOR)
        b.EnforceObstacles()
        wv, wc = mv.ref_enforce(av, ac, mask, bodies, half)
        assert same_bits(b.download(fx.FIELD_VELOCITY1), wv) and same_bits(b.download(fx.FIELD_COLOR), wc), ("enforce", k)
        b.ConfineVorticity()
        cv = b.download(fx.FIELD_VELOCITY1)                            # (the confinement is not the model's: it continues from the device's)
        assert extras or same_bits(cv, wv)
        b.Divergence()
        wb = mv.ref_divergence(cv, mask, bodies)
        assert same_bits(b.download(fx.FIELD_DIVERGENCE), wb), ("divergence", k)
        b.Jacobi(iters)
        wq = mv.ref_jacobi(p0, wb, mask, faces, iters)
        assert same_bits(b.download(fx.FIELD_PRESSURE), wq), ("relaxation", k)
        b.Project()
        assert same_bits(b.download(fx.FIELD_VELOCITY), mv.ref_project(cv, wq, mask, bodies, faces, half)), ("projection", k)
    a.Synchronize(); b.Synchronize()
    keep = (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
    assert [a.digest(k) for k in keep] == [b.digest(k) for k in keep]
    out = a.download(fx.FIELD_VELOCITY)
    a.Release(); b.Release()
    return out


@pytest.mark.parametrize("variant", ["plain", "extras", "open"])
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(64, 64, 8), (36, 36, 1)])
def test_simulate_is_the_stage_composition_and_the_model_s_step(dims, storage, variant):
    m, bodies = scene(dims)
    vel, col, _ = rand_state(dims, 607, storage == "fp16", scale=0.2)
    out = steps_against_the_model(dims, storage, [(m, bodies)] * 3, extras=variant == "extras", faces=OPEN if variant == "open" else 0, state=(vel, col))
    solid = m.astype(bool)
    w = mv.wall_velocity(m.shape, bodies)
    if storage == "fp16":
        w = w.astype(np.float16).astype(f32)
    assert same_bits(out[:, solid], w[:, solid])                       # the solids carry their velocity into the next advection


# ---- 3: equivalence -----------------------------------------------------------------------------------------------------------------------------
def run_plain(dims, storage, mask, bodies, call=True, steps=3, timing=False, faces=0):
    vel, col, _ = rand_state(dims, 613, storage == "fp16", scale=0.2)
    f = make(dims, storage=storage, jacobi_iters=8)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetObstacles(mask)
    f.SetOpenWalls(faces)
    if call:
        f.SetObstacleBodies(bodies)
    f.timing_enable(True)
    dt = time_step(dims)
    for k in range(steps):
        f.UpdateFrame(dt, k % 3)
        f.Simulate(k % 3)
    f.Synchronize()
    t = f.timing_read()
    out = [f.digest(k) for k in ALL_FIELDS], (t.steps, t.jacobi_launches, t.jacobi_sweeps, t.jacobi_main_launches, t.jacobi_main_sweeps)
    f.Release()
    return out


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(64, 64, 8), (36, 36, 1)])
def test_at_rest_the_context_runs_what_it_ran_before(dims, storage):
    X, Y, Z = dims
    m, bodies = scene(dims)
    never = run_plain(dims, storage, m, None, call=False)
    # bodies whose boxes hold cells, none of them solid: the moving kernels run and give the resting bits
    fluid_only = [mv.body(*cells_box(dims, (20, 30), (0, 8), (0, Z - 1)), linear=(3.0, -2.0, 1.0), angular=(0.5, -4.0, 7.0)),
                  mv.body((2.0, 2.0, 2.0), (3.0, 3.0, 3.0), linear=(9.0, 9.0, 9.0))]
    who = mv.body_of(m.shape, fluid_only)
    assert (who == 0).any() and not m[who >= 0].any()
    assert run_plain(dims, storage, m, fluid_only)[0] == never[0]
    # an empty list: the launches of a context that never called, in bits and in count
    assert run_plain(dims, storage, m, []) == never
    # ... also after a list was in force, and with no mask at all the list is idle
    f_bits = run_plain(dims, storage, m, bodies)[0]
    assert f_bits != never[0]
    assert run_plain(dims, storage, None, bodies) == run_plain(dims, storage, None, None, call=False)
    vel, col, _ = rand_state(dims, 613, storage == "fp16", scale=0.2)
    f = make(dims, storage=storage, jacobi_iters=8)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetObstacles(m)
    f.SetObstacleBodies(bodies)
    f.SetObstacleBodies([])
    assert f.GetObstacleBodies() == []
    f.timing_enable(True)
    for k in range(3):
        f.UpdateFrame(time_step(dims), k % 3)
        f.Simulate(k % 3)
    f.Synchronize()
    t = f.timing_read()
    assert ([f.digest(k) for k in ALL_FIELDS], (t.steps, t.jacobi_launches, t.jacobi_sweeps, t.jacobi_main_launches, t.jacobi_main_sweeps)) == never
    f.Release()


@pytest.mark.parametrize("dims,storage,faces", [(d, s, 0) for d in [(20, 20, 5), (36, 36, 1), (64, 64, 8)] for s in ("fp32", "fp16")]
                         + [((64, 64, 8), s, OPEN) for s in ("fp32", "fp16")])
def test_bodies_that_stand_still_give_the_resting_bits(dims, storage, faces):
    """What lets one kernel body serve the resting and the moving solids: the scene's bodies, boxes and pivots kept, with linear = angular =
    +0 run the MOV = 1 kernels over every solid cell and must leave all six fields as the empty list (MOV = 0) leaves them, bit for bit.
    r = pos - pivot takes both signs along x and y over the solid cells the bodies hold; fmaf(-0, r, +0) is +0 either way."""
    m, bodies = scene(dims)
    still = [mv.body(b["box_lo"], b["box_hi"], pivot=b["pivot"]) for b in bodies]
    assert all(b["linear"] == (0.0, 0.0, 0.0) and b["angular"] == (0.0, 0.0, 0.0) and not np.signbit(b["linear"] + b["angular"]).any() for b in still)
    who, pos = mv.body_of(m.shape, still), mv.cell_centres(m.shape)
    for a in range(2):
        r = np.concatenate([pos[a][(who == k) & m.astype(bool)] - f32(b["pivot"][a]) for k, b in enumerate(still)])
        assert (r < 0).any() and (r > 0).any(), a
    assert run_plain(dims, storage, m, still, faces=faces)[0] == run_plain(dims, storage, m, [], faces=faces)[0]


# ---- 4: a moving mask -----------------------------------------------------------------------------------------------------------------------
def ball_frames(dims, frames=5, radius=0.15, moving=True):
    """a ball stepped one cell a frame along +x, voxelised anew each frame, under one body whose box encloses it"""
    dt = float(time_step(dims))
    v = 1.0 / (dims[0] * dt)                                          # texture units per unit time: a cell per step
    out = []
    for k in range(frames):
        c = (0.3 + k * v * dt, 0.5, 0.5)
        mask = ball_mask(dims, center=c, radius=radius)
        box = mv.body([x - radius - 0.01 for x in c], [x + radius + 0.01 for x in c], linear=(v, 0.0, 0.0))
        out.append((mask, [box] if moving else []))
    return out, v


@pytest.mark.parametrize("dims", [(64, 64, 8), (36, 36, 1)])
def test_a_ball_stepped_along_x_pushes_the_air_ahead_of_it(dims):
    """from a state at rest with the impulse off: five frames against the model, then the sign of the flow in front of the ball"""
    frames, v = ball_frames(dims)
    out = steps_against_the_model(dims, "fp32", frames, impulse=False)
    last = frames[-1][0]
    code = ref_codes(last)
    ahead = (code & 0x41) == 0x01                                     # fluid cells whose x-1 neighbour is solid: the shell in front
    assert ahead.sum() >= 5
    mean = float(out[0][ahead].astype(np.float64).mean())
    print("%s: mean u_x ahead of the ball %.6g (the ball's %.6g) over %d cells" % (dims, mean, v, int(ahead.sum())))
    assert mean > 0
    assert (out[0][ahead] == f32(v)).all()                            # free slip against a moving wall: exactly the wall's (the damping is 1 there)
    resting, _ = ball_frames(dims, moving=False)
    rest = steps_against_the_model(dims, "fp32", resting, impulse=False)
    assert not rest[0][ahead].any() and not rest.any()                # a resting ball from rest: exactly 0


# ---- 5: status codes --------------------------------------------------------------------------------------------------------------------------
def c_bodies(bodies):
    arr = (capi.ObstacleBody * max(len(bodies), 1))()
    for k, b in enumerate(bodies):
        arr[k].struct_size, arr[k].flags = C.sizeof(capi.ObstacleBody), 0
        for key in ("box_lo", "box_hi", "linear", "angular", "pivot"):
            setattr(arr[k], key, (C.c_float * 3)(*b[key]))
    return arr


def test_status_codes():
    lib = capi.load()
    dims = (32, 32, 8)
    _, bodies = scene(dims)
    f = make(dims, jacobi_iters=6)
    assert f.GetObstacleBodies() == []                               # the default
    f.SetObstacleBodies(bodies)                                      # no mask in force: legal

    def in_force():
        return bodies_equal(f.GetObstacleBodies(), bodies)
    assert in_force()
    other = [mv.body((0.1, 0.1, 0.1), (0.2, 0.2, 0.2), linear=(1.0, 1.0, 1.0))]
    good = c_bodies(other)
    many = c_bodies(other * 17)
    assert lib.fx_set_obstacle_bodies(f._ctx, many, 17) == capi.FX_E_INVALID and in_force()
    assert lib.fx_set_obstacle_bodies(f._ctx, None, 1) == capi.FX_E_INVALID and in_force()
    for size in (0, 64, 67, 72):
        bad = c_bodies(other); bad[0].struct_size = size
        assert lib.fx_set_obstacle_bodies(f._ctx, bad, 1) == capi.FX_E_INVALID and in_force()
    for flags in (1, 2, 0x80000000):
        bad = c_bodies(other); bad[0].flags = flags
        assert lib.fx_set_obstacle_bodies(f._ctx, bad, 1) == capi.FX_E_INVALID and in_force()
    for key in ("box_lo", "box_hi", "linear", "angular", "pivot"):
        for a in range(3):
            for v in (float("nan"), float("inf"), -float("inf")):
                bad = c_bodies(other * 2)
                getattr(bad[1], key)[a] = v
                assert lib.fx_set_obstacle_bodies(f._ctx, bad, 2) == capi.FX_E_INVALID and in_force(), (key, a, v)
    for a in range(3):
        bad = c_bodies(other)
        bad[0].box_lo[a] = 0.5
        bad[0].box_hi[a] = 0.25
        assert lib.fx_set_obstacle_bodies(f._ctx, bad, 1) == capi.FX_E_INVALID and in_force()
    flat = c_bodies([mv.body((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])      # lo == hi is a box
    assert lib.fx_set_obstacle_bodies(f._ctx, flat, 1) == capi.FX_OK and len(f.GetObstacleBodies()) == 1
    assert lib.fx_set_obstacle_bodies(f._ctx, c_bodies(other * 16), 16) == capi.FX_OK and len(f.GetObstacleBodies()) == 16
    f.SetObstacleBodies(bodies)
    with pytest.raises(fx.FluidxError):
        f.SetObstacleBodies(other * 17)
    # the getter
    n = C.c_uint32(99)
    out = (capi.ObstacleBody * 16)()
    assert lib.fx_get_obstacle_bodies(f._ctx, None, 0, C.byref(n)) == capi.FX_OK and n.value == len(bodies)      # the count alone
    assert lib.fx_get_obstacle_bodies(f._ctx, out, 2, C.byref(n)) == capi.FX_OK and n.value == len(bodies) and out[2].struct_size == 0
    assert lib.fx_get_obstacle_bodies(f._ctx, out, 16, None) == capi.FX_E_INVALID
    assert lib.fx_get_obstacle_bodies(f._ctx, None, 4, C.byref(n)) == capi.FX_E_INVALID
    assert lib.fx_set_obstacle_bodies(None, good, 1) == capi.FX_E_INVALID and lib.fx_get_obstacle_bodies(None, out, 16, C.byref(n)) == capi.FX_E_INVALID
    # configuration: kept across UpdateFrame and a new mask, not digested
    before = sorted(f.digest(k) for k in ALL_FIELDS)
    f.SetObstacles(np.ones((8, 32, 32), np.uint8))
    f.UpdateFrame(f32(0.05), 2)
    f.SetObstacles(None)
    assert in_force() and before == sorted(f.digest(k) for k in ALL_FIELDS)
    assert lib.fx_set_obstacle_bodies(f._ctx, None, 0) == capi.FX_OK and f.GetObstacleBodies() == []

    # faithful contexts
    fa = make(dims, jacobi_iters=16, jacobi_mode="faithful")
    assert lib.fx_set_obstacle_bodies(fa._ctx, good, 1) == capi.FX_E_INVALID and fa.GetObstacleBodies() == []
    with pytest.raises(fx.FluidxError):
        fa.SetObstacleBodies(other)
    # slab ranks: a lone slab context, and the members of an in-process group
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    for r in ranks:
        assert lib.fx_set_obstacle_bodies(r._ctx, good, 1) == capi.FX_E_INVALID and r.GetObstacleBodies() == []
    fx.comm_init_local(ranks)
    for r in ranks:
        assert lib.fx_set_obstacle_bodies(r._ctx, good, 1) == capi.FX_E_INVALID
        assert lib.fx_set_obstacle_bodies(r._ctx, None, 0) == capi.FX_E_INVALID
        assert lib.fx_get_obstacle_bodies(r._ctx, out, 16, C.byref(n)) == capi.FX_OK and n.value == 0 and r.GetObstacleBodies() == []
    ro = fx.Fluid()
    assert ro.Init(64, 64, dims, render_only=True)
    assert lib.fx_set_obstacle_bodies(ro._ctx, good, 1) == capi.FX_E_STATE and lib.fx_set_obstacle_bodies(ro._ctx, None, 0) == capi.FX_E_STATE
    assert lib.fx_set_obstacle_bodies(ro._ctx, many, 17) == capi.FX_E_STATE       # ... whatever else is wrong with the call
    assert lib.fx_get_obstacle_bodies(ro._ctx, out, 16, C.byref(n)) == capi.FX_E_STATE
    for o in [f, fa, ro] + ranks:
        o.Release()


# ---- 6: the C++ wrapper -------------------------------------------------------------------------------------------------------------------
CXX = r'''
#include "Fluid.hpp"
#include <cstdio>
#include <cstdlib>
using namespace fluidx;
int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	const XMUINT3 grid = { 32, 32, 8 };
	Fluid::Options opt;
	opt.storage = FX_STORAGE_FP32; opt.jacobiIters = 8; opt.jacobiMode = FX_JACOBI_FIXED;
	Fluid fluid;
	if (!fluid.Init(nullptr, 0, 0, grid, opt)) return 3;
	std::vector<uint8_t> solid((size_t)32 * 32 * 8, 0);
	for (int z = 2; z < 6; ++z) for (int y = 4; y < 9; ++y) for (int x = 10; x < 13; ++x) solid[((size_t)z * 32 + y) * 32 + x] = 1;
	fx_obstacle_body b = {};
	b.struct_size = sizeof b;
	b.box_lo[0] = 0.25f; b.box_lo[1] = 0.0625f; b.box_lo[2] = 0.125f;
	b.box_hi[0] = 0.5f; b.box_hi[1] = 0.375f; b.box_hi[2] = 0.875f;
	b.linear[0] = 0.5f; b.linear[1] = -0.25f;
	b.angular[2] = 3.0f;
	b.pivot[0] = 0.375f; b.pivot[1] = 0.25f; b.pivot[2] = 0.5f;
	std::vector<fx_obstacle_body> list(1, b), back;
	if (!fluid.SetObstacles(solid) || !fluid.SetObstacleBodies(list)) return 4;
	if (!fluid.GetObstacleBodies(back) || back.size() != 1 || back[0].angular[2] != 3.0f || back[0].box_hi[1] != 0.375f) return 5;
	list.resize(17, b);
	if (fluid.SetObstacleBodies(list) || fluid.LastStatus() != FX_E_INVALID) return 6;             // the list in force stays
	if (!fluid.GetObstacleBodies(back) || back.size() != 1) return 7;
	const XMFLOAT4X4 id = { { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } } };
	const XMFLOAT3 eye = { 0, 0, -1 };
	for (int k = 0; k < 3; ++k) {
		fluid.UpdateFrame(2.0f / 32.0f, (uint8_t)(k % 3), id, id, eye);
		fluid.Simulate(nullptr, (uint8_t)(k % 3));
		if (fluid.LastStatus() != FX_OK) return 8;
	}
	if (fx_synchronize(fluid.Handle()) != FX_OK) return 9;
	return fluid.SaveCheckpoint(argv[1]) ? 0 : 10;
}
'''


def test_the_cxx_wrapper_sets_the_bodies(tmp_path):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cc)
    lib = fxbuild.ensure_built()
    libdir = os.path.dirname(lib)
    src, exe, ck = tmp_path / "bodies.cpp", str(tmp_path / "bodies"), str(tmp_path / "bodies.fxck")
    src.write_text(CXX)
    subprocess.run([cc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "fluidx12_amd", "csrc"), str(src), "-o", exe, "-L" + libdir, "-lfluidx_hip",
                    "-Wl,-rpath," + libdir], check=True, timeout=300)
    r = subprocess.run([exe, ck], capture_output=True, text=True, timeout=120)             # a fresh child process, under its own time limit
    assert r.returncode == 0, (r.returncode, r.stderr)
    # the same three steps through the Python mirror
    dims = (32, 32, 8)
    m = np.zeros((8, 32, 32), np.uint8)
    m[2:6, 4:9, 10:13] = 1
    body = mv.body((0.25, 0.0625, 0.125), (0.5, 0.375, 0.875), linear=(0.5, -0.25, 0.0), angular=(0.0, 0.0, 3.0), pivot=(0.375, 0.25, 0.5))
    f = make(dims, jacobi_iters=8)
    f.SetObstacles(m)
    f.SetObstacleBodies([body])
    for k in range(3):
        f.UpdateFrame(f32(2.0 / 32.0), k % 3)
        f.Simulate(k % 3)
    f.Synchronize()
    g = make(dims, jacobi_iters=8)
    g.LoadCheckpoint(ck)
    keep = (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE)
    assert [f.digest(k) for k in keep] == [g.digest(k) for k in keep]
    solid = m.astype(bool)
    assert same_bits(g.download(fx.FIELD_VELOCITY)[:, solid], mv.wall_velocity(m.shape, [body])[:, solid])
    f.Release(); g.Release()
