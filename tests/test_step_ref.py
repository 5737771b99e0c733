"""CPU checks of tests/step_ref.py, the numpy model of one whole fx_simulate step: the anchors that tie the composition to the models it is made
of, and the conditions on the inputs of tests/test_gpu_step_model.py -- every optional stage took part in every case it is switched on in, in
bits, records died at open faces and stopped at solids, the trail reached a stated share of the cells, nothing overflowed.  These are
statements about the cases' seeds and parameters, checked on the model alone; the GPU file then compares the library with the same
trajectories bit for bit."""
import numpy as np
import pytest

import maccormack_ref as mc
import moving_obstacle_ref as mv
import particle_ref as pr
import step_ref as sr
from oracle import orc

f32 = np.float32
CASES = [(case, dims, storage) for case in sorted(sr.CASES) for dims in sr.CASES[case] for storage in sr.STORAGES]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def rand_state(dims, seed, half):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vel = (rng.standard_normal((3, Z, Y, X)) * 0.5).astype(f32)
    if Z == 1:
        vel[2] = 0
    col = rng.random((Z, Y, X, 4)).astype(f32)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    if half:
        vel, col = vel.astype(np.float16).astype(f32), col.astype(np.float16).astype(f32)
    return vel, col, p


# ---- the anchors ---------------------------------------------------------------------------------------------------------------------------
# The oracle's step always runs the reference's built-in impulse, the model never does.  On grids of eight cells a side no cell centre lies in
# the impulse ball (radius 1/16 about (0.5, 0.1, 0.5); 2-D: 1/32), so there the two steps are the same function and compare bit for bit.
NO_IMPULSE = [(8, 8, 6), (8, 8, 1)]


@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dims", NO_IMPULSE)
def test_with_everything_off_the_model_is_the_oracles_step(dims, half, address):
    assert not mc.impulse_support(dims).any()
    X, Y, Z = dims
    vel, col, p = rand_state(dims, 11, half)
    o = orc.Sim(X, Y, Z, iters=5, address=int(address == "mirror"), half=half)
    o.vel[0][:], o.col[o.parity][:], o.p[:] = vel, col, p
    s = sr.initial(vel, col, p)
    cfg = sr.config(address=address, half=half, iters=5)
    dt = pr.time_step(dims)
    for i in range(3):
        o.step(dt)
        s = sr.step(s, cfg, dt, i % 3)
        assert s["parity"] == o.parity
        assert same_bits(s["vel"][0], o.vel[0]) and same_bits(s["vel"][1], o.vel[1]) and same_bits(s["p"], o.p) and same_bits(s["b"], o.b), i
        assert same_bits(s["col"][0], o.col[0]) and same_bits(s["col"][1], o.col[1]), i
    assert s["temp"] is None and s["rec"] is None and o.vel[0].any()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dims", [(36, 36, 1), (20, 20, 5)])
def test_with_obstacles_and_bodies_alone_the_model_is_the_moving_obstacles_step(dims, half):
    from test_gpu_moving_obstacles import scene
    mask, bodies = scene(dims)
    vel, col, p = rand_state(dims, 13, half)
    cfg = sr.config(half=half, mask=mask, bodies=bodies, iters=6)
    dt = pr.time_step(dims)
    s = sr.step(sr.initial(vel, col, p), cfg, dt, 0)
    v1, c1 = mc.step(vel, col, dt, "clamp", impulse=False, half=half, scheme="semi-lagrangian")
    wv1, wc, wb, wq, wv = mv.ref_step(v1, c1, p, mask, bodies, 6, 0, half)
    assert same_bits(s["vel"][1], wv1) and same_bits(s["col"][s["parity"]], wc) and same_bits(s["b"], wb) and same_bits(s["p"], wq) and same_bits(s["vel"][0], wv)
    assert not same_bits(wv, sr.step(sr.initial(vel, col, p), dict(cfg, bodies=()), dt, 0)["vel"][0])


@pytest.mark.parametrize("dims", NO_IMPULSE)
def test_with_particles_alone_the_model_is_the_core_step_and_the_move(dims):
    X, Y, Z = dims
    vel, col, p = rand_state(dims, 17, False)
    rec = pr.records(dims, 257, 19)
    prm = pr.params(scheme=pr.MIDPOINT, drift=sr.DRIFT, lifetime=0.9)
    o = orc.Sim(X, Y, Z, iters=5)
    o.vel[0][:], o.col[o.parity][:], o.p[:] = vel, col, p
    s = sr.initial(vel, col, p, rec=rec)
    cfg = sr.config(iters=5, particles=prm)
    dt = pr.time_step(dims)
    for i in range(2):
        o.step(dt)
        rec = pr.move(rec, o.vel[0], dt, prm)
        s = sr.step(s, cfg, dt, i)
        assert same_bits(s["vel"][0], o.vel[0]) and same_bits(s["col"][s["parity"]], o.color) and same_bits(s["rec"], rec)
    assert (s["runs"], s["sorts"], s["live"]) == (2, 0, 0) and not same_bits(rec, pr.records(dims, 257, 19))


def test_the_sort_is_due_on_the_first_and_every_nth_run_of_the_stage():
    dims = (8, 8, 6)
    vel, col, p = rand_state(dims, 23, False)
    s = sr.initial(vel, col, p, rec=pr.records(dims, 257, 29))
    cfg = sr.config(iters=2, particles=pr.params(), sort_every=3)
    seen = []
    for i in range(7):
        s = sr.step(s, cfg, pr.time_step(dims), i % 3)
        seen.append("order" in s["trace"])
    assert seen == [True, False, False, True, False, False, True] and (s["runs"], s["sorts"]) == (7, 3)


# ---- the cases of the GPU file: every stage took part ----------------------------------------------------------------------------------------
def stages_of(case):
    """(name, `without` of the run that leaves it out, changes to the configuration of that run)"""
    both = [("the buoyancy force", ("force",), {}), ("the trail's colour", ("trail_colour",), {}), ("the trail's heat", ("trail_heat",), {}),
            ("the confinement", ("confine",), {}), ("the particle sort", ("sort",), {}), ("the particle move", ("move",), {})]
    if case != "A":
        return both
    return both + [("the inflow", ("inflow",), {}), ("the enforce pass", ("enforce",), {}), ("the bodies", (), dict(bodies=())), ("the open faces", (), dict(faces=0))]


@pytest.mark.parametrize("case,dims,storage", CASES)
def test_every_stage_of_the_case_changes_the_trajectory(case, dims, storage):
    full = sr.trajectory(case, dims, storage)[-1]
    for name, without, changes in stages_of(case):
        other = sr.trajectory(case, dims, storage, without, **changes)[-1]
        assert not sr.same(full, other), name
    # what each of them is there to change, not just anything
    cut = lambda w: sr.trajectory(case, dims, storage, (w,))[-1]
    assert not same_bits(full["vel"][0], cut("force")["vel"][0]) and not same_bits(full["vel"][0], cut("confine")["vel"][0])
    assert not same_bits(full["col"][full["parity"]], cut("trail_colour")["col"][full["parity"]]) and not same_bits(full["temp"], cut("trail_heat")["temp"])
    assert not same_bits(full["rec"], cut("sort")["rec"]) and not same_bits(full["rec"][:, :3], cut("move")["rec"][:, :3])
    # the heat the trail leaves lifts from the next step on: through the force, into the velocity
    assert not same_bits(full["vel"][0], cut("trail_heat")["vel"][0])
    if case == "A":
        assert not same_bits(full["col"][full["parity"]], cut("inflow")["col"][full["parity"]]) and not same_bits(full["vel"][1], cut("enforce")["vel"][1])
        assert not same_bits(full["temp"], sr.trajectory(case, dims, storage, (), faces=0)[-1]["temp"])         # the ambient ghost of the temperature


@pytest.mark.parametrize("case,dims", [("A", (36, 36, 1)), ("C", (70, 70, 5))])
def test_a_stage_on_the_wrong_buffer_or_parity_changes_the_trajectory(case, dims, monkeypatch):
    """the wiring faults the GPU file is there to catch, made in the model: each ends in other bits than the step as the header has it, so a
    library that made one of them could not equal the model"""
    full = sr.trajectory(case, dims, "fp32")[-1]
    cfg = sr.case_config(case, dims, "fp32")

    def run():
        s = sr.case_initial(case, dims, "fp32")
        for i in range(sr.STEPS):
            s = sr.step(s, cfg, pr.time_step(dims), i % 3)
        return s
    assert sr.same(run(), full)
    # the temperature traced with VELOCITY1, the other velocity buffer
    heat = sr.orf.heat_apply if cfg["faces"] else sr.br.apply
    with monkeypatch.context() as m:
        m.setattr(sr.orf if cfg["faces"] else sr.br, "heat_apply" if cfg["faces"] else "apply", lambda T, vel0, vel1, *a, **kw: heat(T, vel1, vel1, *a, **kw))
        assert not sr.same(run(), full)
    # the trail on the records of the wrong moment: the positions of one step earlier
    density, seen = sr.tr.density, []

    def stale(rec, d):
        seen.append(rec)
        return density(seen[-2] if len(seen) > 1 else rec, d)
    with monkeypatch.context() as m:
        m.setattr(sr.tr, "density", stale)
        assert not sr.same(run(), full)
    # a stage that does its work on one parity only
    confine, calls = sr.vr.confine_stored, []
    with monkeypatch.context() as m:
        m.setattr(sr.vr, "confine_stored", lambda u, *a: (calls.append(0), confine(u, *a) if len(calls) % 2 else np.array(u, f32))[1])
        assert not sr.same(run(), full)
    # the pressure solve from zero instead of from the previous step's pressure
    if case == "A":
        jac = sr.mv.ref_jacobi
        with monkeypatch.context() as m:
            m.setattr(sr.mv, "ref_jacobi", lambda p, *a: jac(np.zeros_like(p), *a))
            assert not sr.same(run(), full)
    # the sort due on the other runs of the stage
    s = sr.case_initial(case, dims, "fp32")
    s["runs"] = 1
    for i in range(sr.STEPS):
        s = sr.step(s, dict(cfg, sort_every=2), pr.time_step(dims), i % 3)
    assert not sr.same(s, full)


@pytest.mark.parametrize("case,dims,storage", CASES)
def test_the_stated_shares(case, dims, storage):
    cfg = sr.case_config(case, dims, storage)
    states = sr.trajectory(case, dims, storage)
    dt = pr.time_step(dims)
    identity = np.arange(sr.COUNT, dtype=np.uint32)
    sorted_steps = [i for i, s in enumerate(states) if "order" in s["trace"]]
    assert sorted_steps == ([0, 2] if case == "A" else [0, 1, 2, 3])           # every 2 / every 1: two due sorts in four steps at the least
    assert any(not np.array_equal(states[i]["trace"]["order"], identity) for i in sorted_steps)
    solid = None if cfg["mask"] is None else np.asarray(cfg["mask"]) != 0
    died_at_a_face = stopped = killed_by_age = 0
    for s in states:
        rec_in, vel = s["trace"]["rec_in"], s["trace"]["vel"]
        with np.errstate(invalid="ignore"):
            live_in, live_out = rec_in[:, 3] >= 0, s["rec"][:, 3] >= 0
            closed = pr.move(rec_in, vel, dt, cfg["particles"], 0, solid)[:, 3] >= 0
            immortal = pr.move(rec_in, vel, dt, dict(cfg["particles"], lifetime=0.0), cfg["faces"], solid)[:, 3] >= 0
        died_at_a_face += int((closed & ~live_out).sum())
        killed_by_age += int((immortal & ~live_out).sum())
        if solid is not None:
            free = pr.move(rec_in, vel, dt, cfg["particles"], cfg["faces"], None)
            stopped += int((live_in & (bits(free[:, :3]) != bits(s["rec"][:, :3])).any(axis=1)).sum())
        assert same_bits(s["rec"][~live_in], rec_in[~live_in])               # the dead keep their bits
    last = states[-1]
    assert 0 < killed_by_age and 0 < int(live_out.sum()) < int((sr.case_initial(case, dims, storage)["rec"][:, 3] >= 0).sum())
    if case == "A":
        assert died_at_a_face >= 1 and stopped >= 1, (died_at_a_face, stopped)
    fluid = np.ones(last["p"].shape, bool) if solid is None else ~solid
    share = last["trace"]["trail_cells"][fluid].mean()
    assert share >= 0.01, share
    for name, a in sr.fields(last).items():
        if a.dtype == f32 and name != "PARTICLES":                          # (the records hold NaN ages and positions by design)
            assert np.isfinite(a).all(), name
    if storage == "fp16":                                                     # what a fp16 context stores is fp16-representable
        for name in ("VELOCITY", "VELOCITY1", "COLOR", "COLOR_PREV"):
            a = sr.fields(last)[name]
            assert same_bits(a, a.astype(np.float16).astype(f32)), name
