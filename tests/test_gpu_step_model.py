"""fx_simulate with every optional stage on against tests/step_ref.py, the numpy model of the whole step: four steps of nothing but
fx_update_frame + fx_simulate on one context -- no stage call, no download before the end --, then every field, the particles, the sort's order
and its counts against the model's trajectory from the same initial state, as uint32 bit patterns with no tolerance.

The per-stage files hold each kernel to its model and fx_simulate to a list of stage calls copied from the scheduler; this file holds the
wiring to the header's prose: the order of the stages, which velocity, colour, pressure and temperature buffer each one reads at its point of
the step, on both parities, across a wrap of the frame index and two due sorts.  tests/test_step_ref.py shows on the CPU that every stage
changes these trajectories, so a stage that ran in the wrong place or read the other buffer cannot pass.

Cases (step_ref.CASES), both storages each:
  A  MacCormack, mirror addressing, open walls Y_HI | X_LO, buoyancy with a tilted `up`, a trail with tint and negative heat, the mask and
     bodies of test_gpu_moving_obstacles.scene, confinement, 8 boundary-aware sweeps, 4099 records, midpoint, sort every 2
     (36, 36, 1) 2-D, the smallest grid that holds the scene; (68, 68, 5) the wide sweep with X % 64 != 0, thin z
  B  semi-Lagrangian, clamp, a closed box, multigrid with the default cycles, Euler, sort every 1: (64, 64, 8) and (36, 36, 1)
  C  as B with the plain Jacobi solver, 7 sweeps, and MacCormack: (70, 70, 5), the planner's blockg family
No emitters, heat sources or built-in impulse: see the top of tests/step_ref.py."""
import numpy as np
import pytest

import fluidx12_amd as fx

import particle_ref as pr
import step_ref as sr

pytestmark = pytest.mark.gpu
CASES = [(case, dims, storage) for case in sorted(sr.CASES) for dims in sr.CASES[case] for storage in sr.STORAGES]
SCHEMES = {0: "euler", 1: "midpoint"}


def configure(f, cfg):
    """the setters of one configuration of step_ref.config, in no particular order but the header's "set the sort, then the set" """
    f.SetImpulse(0)
    f.SetAdvectionScheme(cfg["scheme"])
    if cfg["solver"] == "multigrid":
        m = cfg["multigrid"]
        f.SetPressureSolver("multigrid", cycles=m["cycles"], pre_sweeps=m["pre"], post_sweeps=m["post"], coarse_sweeps=m["coarse"], max_levels=m["max_levels"],
                            omega=float(m["omega"]))
    if cfg["mask"] is not None:
        f.SetObstacles(cfg["mask"])
        f.SetObstacleBodies(list(cfg["bodies"]))
    f.SetOpenWalls(cfg["faces"])
    if cfg["buoyancy"] is not None:
        f.SetBuoyancy(**cfg["buoyancy"])
    if cfg["vort_eps"]:
        f.SetVorticityConfinement(cfg["vort_eps"])
    if cfg["trail"] is not None:
        f.SetParticleTrail(cfg["trail"]["rate"], cfg["trail"]["tint"], cfg["trail"]["heat"])
    if cfg["sort_every"]:
        f.SetParticleSort(True, cfg["sort_every"])
    prm = cfg["particles"]
    f.SetParticleParams(SCHEMES[prm["scheme"]], prm["drift"], prm["lifetime"])


def device_fields(f, state):
    """what the context holds, under the names and in the order of step_ref.fields"""
    out = dict(VELOCITY=f.download(fx.FIELD_VELOCITY), VELOCITY1=f.download(fx.FIELD_VELOCITY1), COLOR=f.download(fx.FIELD_COLOR),
               COLOR_PREV=f.download(fx.FIELD_COLOR_PREV), PRESSURE=f.download(fx.FIELD_PRESSURE), DIVERGENCE=f.download(fx.FIELD_DIVERGENCE))
    if state["temp"] is not None:
        out["TEMPERATURE"] = f.download(fx.FIELD_TEMPERATURE)
    if state["rec"] is not None:
        out["PARTICLES"] = f.GetParticles()
        out["ORDER"] = f.ParticleOrder()
        out["SORT_INFO"] = np.array(f.ParticleSortInfo(), np.uint32)
    return out


@pytest.mark.parametrize("case,dims,storage", CASES)
def test_four_steps_of_simulate_are_the_models_trajectory(case, dims, storage):
    cfg = sr.case_config(case, dims, storage)
    s0 = sr.case_initial(case, dims, storage)
    want = sr.trajectory(case, dims, storage)[-1]
    f = fx.Fluid()
    assert f.Init(0, 0, dims, storage=storage, advect_address=cfg["address"], jacobi_iters=cfg["iters"]), f.last_status
    configure(f, cfg)
    f.upload(fx.FIELD_VELOCITY, s0["vel"][0]); f.upload(fx.FIELD_COLOR, s0["col"][0]); f.upload(fx.FIELD_PRESSURE, s0["p"])
    if s0["temp"] is not None:
        f.upload(fx.FIELD_TEMPERATURE, s0["temp"])
    f.SetParticles(s0["rec"])
    dt = pr.time_step(dims)
    for i in range(sr.STEPS):
        f.UpdateFrame(dt, i % 3)
        f.Simulate(i % 3)
    f.Synchronize()
    assert f.frame_info().frame_parity == want["parity"]
    got = device_fields(f, want)
    f.Release()
    diff = sr.first_difference(got, sr.fields(want))
    assert diff is None, "first difference in %s at %s: device %r, model %r (%d elements differ)" % diff
