"""numpy model of one whole fx_simulate step with its optional stages on, composed from the per-stage models of this directory.

The order is the header's (include/fluidx_hip.h: "advect -> inflow -> emit -> heat -> enforce -> confine -> divergence -> relaxation ->
projection" of fx_set_open_walls, the trail "between the buoyancy pass and the obstacles' enforce pass" of fx_set_particle_trail, the
particle stage "behind the projection" with the sort "in front of the move"), not the scheduler's.  Which buffer a stage reads at its point
of the step is the header's too:
  advection    traces with VELOCITY and samples VELOCITY and the PREVIOUS colour (fx_update_frame has flipped the parity: COLOR names the
               buffer the step writes); the results are VELOCITY1 and COLOR
  inflow       scales COLOR by the weights of the advection's own back-trace: VELOCITY
  buoyancy     traces the temperature with VELOCITY, reads rho from COLOR behind the inflow pass, adds the force to VELOCITY1; the two
               temperature buffers swap, so everything behind it sees the new temperature as "the current one"
  trail        the positions the buffer holds now; adds to COLOR and, with buoyancy on, to the current temperature
  enforce      VELOCITY1 and COLOR
  confinement  VELOCITY1 -> VELOCITY1 (the two velocity names swap; VELOCITY is unspecified until the projection has written it)
  divergence   of VELOCITY1;  the solve starts from the pressure the previous step left;  the projection writes VELOCITY
  particles    the sort when this run of the stage is due one, then the move through the projected VELOCITY
Nothing here is new arithmetic: every line calls a model that a per-stage GPU test already holds its kernel to.

Left out of the model: the settable emitters, the heat sources and the built-in impulse.  All three evaluate exp2, their results are
specified only up to a threshold mask (tests/emitter_ref.py), and behind a pressure solve no mask contains the difference.  The
configurations here therefore run with fx_set_impulse(0), no emitters and no heat sources; the particle trail, which is integers and fused
multiply-adds, is the bit-exact source of smoke and heat instead.  tests/test_gpu_emitters.py and tests/test_gpu_buoyancy.py keep holding
the three.  Also left out: dt <= 0 (a paused frame), slab ranks, the faithful Jacobi mode, render paths.

`state` (a dict, never modified in place: `step` returns a new one):
  vel      [VELOCITY, VELOCITY1]  float32[3][Z][Y][X] each
  col      the two colour buffers float32[Z][Y][X][4], `parity` = which of them FX_FIELD_COLOR names
  p, b     FX_FIELD_PRESSURE, FX_FIELD_DIVERGENCE  float32[Z][Y][X]
  temp     FX_FIELD_TEMPERATURE or None while buoyancy is off
  rec      the particle records float32[n][4] or None;  runs = how often the particle stage has run (the sort's `every` counts it);
           order, live, sorts = what fx_particle_order_device / fx_particle_sort_info report
  trace    what the last step saw on its way, for tests/test_step_ref.py's conditions on the inputs (never compared with the device)
fp16 storage: the fields hold fp16-representable values and every model rounds what it stores once, as the per-stage files have it."""
import functools

import numpy as np

import buoyancy_ref as br
import maccormack_ref as mc
import moving_obstacle_ref as mv
import multigrid_ref as mg
import open_ref as orf
import particle_ref as pr
import particle_sort_ref as ps
import particle_trail_ref as tr
import vorticity_ref as vr
from oracle import orc

f32 = np.float32

# what `without` may name: one stage, or one of the two things the buoyancy pass and the trail each do, left out of an otherwise unchanged step
STAGES = ("inflow", "force", "trail_colour", "trail_heat", "enforce", "confine", "sort", "move")

DEFAULTS = dict(scheme="semi-lagrangian", address="clamp", half=False, faces=0, buoyancy=None, trail=None, mask=None, bodies=(), vort_eps=0.0,
                solver="jacobi", iters=40, multigrid=None, particles=None, sort_every=None)


def config(**kw):
    """scheme / address: the advection's;  half: fp16 storage;  faces: FX_WALL_* bits;  buoyancy: buoyancy_ref.params or None;
    trail: particle_trail_ref.trail or None;  mask, bodies: fx_set_obstacles / fx_set_obstacle_bodies;  vort_eps: the confinement's epsilon;
    solver "jacobi" with `iters` sweeps or "multigrid" with `multigrid` = multigrid_ref.defaults;  particles: particle_ref.params (the set
    itself is state["rec"]);  sort_every: None = sorting off, n = fx_set_particle_sort(enabled, n)"""
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    c = dict(DEFAULTS)
    c.update(kw)
    assert c["solver"] == "jacobi" or (c["mask"] is None and not c["faces"])          # fx_set_pressure_solver refuses the others
    return c


def initial(vel, col, p=None, temp=None, rec=None):
    """the state behind the uploads of a fresh context: FX_FIELD_VELOCITY, FX_FIELD_COLOR, FX_FIELD_PRESSURE, FX_FIELD_TEMPERATURE, fx_set_particles"""
    vel, col = np.array(vel, f32), np.array(col, f32)
    n = 0 if rec is None else len(rec)
    return dict(vel=[vel, np.zeros_like(vel)], col=[col, np.zeros_like(col)], parity=0, p=np.zeros(col.shape[:3], f32) if p is None else np.array(p, f32),
                b=np.zeros(col.shape[:3], f32), temp=None if temp is None else np.array(temp, f32), rec=None if rec is None else np.array(rec, f32),
                runs=0, order=np.zeros(n, np.uint32), live=0, sorts=0, trace={})


def step(state, config, dt, frame, without=()):
    """one fx_update_frame(dt, frame) + fx_simulate(frame) -> the state behind it.  `frame` picks one of the library's three per-frame
    constant slots and enters no arithmetic."""
    c, dt = config, f32(dt)
    assert dt > 0 and frame in (0, 1, 2) and set(without) <= set(STAGES)
    half, faces, mask, bodies = c["half"], c["faces"], c["mask"], list(c["bodies"])
    solid = None if mask is None else np.asarray(mask) != 0
    s = dict(state)
    trace = {}
    parity = s["parity"] ^ 1                                                  # fx_update_frame, dt > 0
    vel0 = s["vel"][0]
    # 1 advection
    v1, col = mc.step(vel0, s["col"][1 - parity], dt, c["address"], impulse=False, half=half, scheme=c["scheme"])
    # 2 inflow
    if faces and "inflow" not in without:
        col = orf.ref_inflow(col, vel0, dt, faces, half)
    # 3 buoyancy, no heat sources
    temp = s["temp"]
    if c["buoyancy"] is not None:
        if faces:
            temp, forced = orf.heat_apply(temp, vel0, v1, col, c["buoyancy"], [], dt, c["address"], half, solid=solid, faces=faces)
        else:
            temp, forced = br.apply(temp, vel0, v1, col, c["buoyancy"], [], dt, c["address"], half, solid=solid)
        if "force" not in without:
            v1 = forced
    # 4 trail
    if c["trail"] is not None and s["rec"] is not None:
        acc = tr.density(s["rec"], col.shape[2::-1])
        coloured, heated = tr.apply(acc, col, dt, c["trail"], temp=temp if c["buoyancy"] is not None else None, solid=solid, half=half)
        trace["trail_cells"] = (acc != 0) & ~(solid if solid is not None else np.zeros(acc.shape, bool))
        if "trail_colour" not in without:
            col = coloured
        if heated is not None and "trail_heat" not in without:
            temp = heated
    # 5 enforce
    if solid is not None and solid.any() and "enforce" not in without:
        v1, col = mv.ref_enforce(v1, col, mask, bodies, half)
    # 6 confinement
    if c["vort_eps"] > 0 and "confine" not in without:
        v1 = vr.confine_stored(v1, c["vort_eps"], dt, half)
    # 7 divergence, solve, projection
    if solid is not None or faces:
        b = mv.ref_divergence(v1, mask, bodies)
        p = mv.ref_jacobi(s["p"], b, mask, faces, c["iters"])
        vel = mv.ref_project(v1, p, mask, bodies, faces, half)
    else:
        b = orc.divergence(v1)
        p = mg.solve(s["p"], b, c["multigrid"])[0] if c["solver"] == "multigrid" else orc.jacobi(s["p"], b, c["iters"])[0]
        vel = orc.project(v1, p, half)
    # 8 particles, on the projected velocity
    rec, runs, order, live, sorts = s["rec"], s["runs"], s["order"], s["live"], s["sorts"]
    if rec is not None:
        if c["sort_every"]:
            due = runs % c["sort_every"] == 0
            if due and "sort" not in without:
                rec, order, live = ps.sort(rec, col.shape[2::-1])
                sorts += 1
                trace["order"] = order
        runs += 1
        trace["rec_in"], trace["vel"] = rec, vel
        if "move" not in without:
            rec = pr.move(rec, vel, dt, c["particles"], faces, solid)
    cols = list(s["col"])
    cols[parity] = col
    s.update(vel=[vel, v1], col=cols, parity=parity, p=np.asarray(p, f32), b=np.asarray(b, f32), temp=temp, rec=rec, runs=runs, order=order, live=live, sorts=sorts,
             trace=trace)
    return s


def fields(state):
    """name -> array, in the order the GPU test compares: the seven fields, then what the particle calls return"""
    out = dict(VELOCITY=state["vel"][0], VELOCITY1=state["vel"][1], COLOR=state["col"][state["parity"]], COLOR_PREV=state["col"][1 - state["parity"]],
               PRESSURE=state["p"], DIVERGENCE=state["b"])
    if state["temp"] is not None:
        out["TEMPERATURE"] = state["temp"]
    if state["rec"] is not None:
        out["PARTICLES"] = state["rec"]
        out["ORDER"] = state["order"]
        out["SORT_INFO"] = np.array([state["live"], state["sorts"]], np.uint32)
    return out


def first_difference(fa, fb):
    """two dicts as `fields` makes them: None if they agree in every bit, else (field, index of the first differing element, the two values,
    how many elements differ)"""
    assert list(fa) == list(fb), (list(fa), list(fb))
    for name in fa:
        x, y = np.ascontiguousarray(fa[name]), np.ascontiguousarray(fb[name])
        assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape, x.dtype, y.dtype)
        bad = np.argwhere(x.view(np.uint32) != y.view(np.uint32))
        if len(bad):
            at = tuple(int(v) for v in bad[0])
            return name, at, x[at], y[at], len(bad)
    return None


def same(a, b):
    return first_difference(fields(a), fields(b)) is None


# ---- the cases tests/test_step_ref.py and tests/test_gpu_step_model.py run ------------------------------------------------------------------
STEPS = 4
OPEN = orf.Y_HI | orf.X_LO
BUOY = br.params(ambient=0.25, density_weight=0.7, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2))             # a tilted `up`
TRAIL = tr.trail(rate=3.0, tint=(0.25, -0.5, 0.125, 0.7), heat=-2.5)
DRIFT, LIFETIME, COUNT = (0.03, -0.4, 0.02), 0.7, 4099
CASES = {"A": [(36, 36, 1), (68, 68, 5)], "B": [(64, 64, 8), (36, 36, 1)], "C": [(70, 70, 5)]}
STORAGES = ("fp32", "fp16")


def case_config(case, dims, storage):
    half = storage == "fp16"
    if case == "A":                                                           # the boundaries: open walls, a mask with bodies, mirror addressing
        from test_gpu_moving_obstacles import scene
        mask, bodies = scene(dims)
        return config(scheme="maccormack", address="mirror", half=half, faces=OPEN, buoyancy=BUOY, trail=TRAIL, mask=mask, bodies=bodies, vort_eps=4.0,
                      iters=8, particles=pr.params(scheme=pr.MIDPOINT, drift=DRIFT, lifetime=LIFETIME), sort_every=2)
    common = dict(half=half, buoyancy=BUOY, trail=TRAIL, vort_eps=4.0, particles=pr.params(scheme=pr.EULER, drift=DRIFT, lifetime=LIFETIME), sort_every=1)
    if case == "B":                                                           # the closed box with multigrid
        return config(solver="multigrid", multigrid=mg.defaults(dims), **common)
    assert case == "C"                                                        # the plain solver under MacCormack
    return config(scheme="maccormack", iters=7, **common)


def case_initial(case, dims, storage):
    """velocity, colour, pressure, temperature, records: seeded, fp16-representable where the storage is"""
    half = storage == "fp16"
    X, Y, Z = dims
    seed = 7100 + 10 * sorted(CASES).index(case)
    vel = pr.velocity(dims, seed, cells=0.6, half=half)
    rng = np.random.default_rng(seed + 1)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    col = col.astype(np.float16).astype(f32) if half else col
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    temp = tr.fields(dims, seed + 2)[1]                                       # random, -0 in every other cell
    return initial(vel, col, p, temp, pr.records(dims, COUNT, seed + 3))


@functools.lru_cache(maxsize=None)
def trajectory(case, dims, storage, without=(), **changes):
    """the STEPS states behind the initial one; `changes` replace members of the case's configuration (bodies=(), faces=0)"""
    cfg = dict(case_config(case, dims, storage), **dict(changes))
    s = case_initial(case, dims, storage)
    dt = pr.time_step(dims)
    out = []
    for i in range(STEPS):
        s = step(s, cfg, dt, i % 3, without)
        out.append(s)
    return tuple(out)
