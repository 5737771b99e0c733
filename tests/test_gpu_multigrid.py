"""The multigrid pressure solver on the GPU (fx_set_pressure_solver / fx_pressure_solve, csrc/fx_multigrid.hip: k_mg_smooth, k_mg_smooth_v4,
k_mg_residual_restrict, k_mg_prolong_correct, k_mg_tail).

Everything against the numpy model tests/multigrid_ref.py is bit for bit -- the pressure and, through fx_download_pressure_level, the correction
and the right-hand side every coarse level is left with; the rest are digests: the tail against the launches per level, fx_simulate against the
stage calls, the untouched default, the resume.  The one inequality is the convergence statement tests/test_multigrid_ref.py holds the model to,
on the same arrays."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import buoyancy_ref as br
import emitter_ref as er
import multigrid_ref as mg
import open_ref
from test_gpu_buoyancy import rand_state, time_step, same_bits, masks, make, ALL_FIELDS

pytestmark = pytest.mark.gpu
f32 = np.float32

# (fx_create takes square planes only, X = Y: the shapes vary the row length and the depth)
SCALAR = [(22, 22, 8), (70, 70, 4), (150, 150, 4)]         # rows shorter than a tile; across the 64-lane tile; two levels: 75 x 75 x 2
V4 = [(20, 20, 8), (136, 136, 4), (256, 256, 4), (320, 320, 4), (64, 64, 4)]  # five float4 a row; a ragged wave; X4 = 64, the wave seam; two x blocks; rows of 16 float4
FLAT = [(36, 36, 1), (150, 150, 1)]
ONE_LEVEL = [(37, 37, 1), (21, 21, 5)]
TAIL = [(32, 32, 32)]                                      # reaches the tail from 16^3
SHAPES = SCALAR + V4 + FLAT + ONE_LEVEL + TAIL


def variants(dims):
    """the default parameters; V(0, 1) with one coarse sweep (restriction and prolongation alone); one level; omega = 1; three cycles"""
    d = mg.defaults(dims)
    return [("default", d), ("V(0,1)", dict(d, pre=0, post=1, coarse=1)), ("one level", dict(d, max_levels=1)), ("omega 1", dict(d, omega=f32(1.0))),
            ("three cycles", dict(d, cycles=3))]


def set_solver(f, prm, flags=0):
    f.SetPressureSolver("multigrid", cycles=prm["cycles"], pre_sweeps=prm["pre"], post_sweeps=prm["post"], coarse_sweeps=prm["coarse"],
                        max_levels=prm["max_levels"], omega=float(prm["omega"]), flags=flags)


def fields(dims, seed):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    b = rng.standard_normal((Z, Y, X)).astype(f32)
    p[0, 0, :2] = f32(-0.0)
    b[0, 1, :2] = f32(0.0)
    return p, b


def solve_on_device(f, p, b):
    """one fx_pressure_solve from (p, b): the pressure and [None, (e_1, b_1), ...] of the levels in use"""
    f.upload(fx.FIELD_PRESSURE, p); f.upload(fx.FIELD_DIVERGENCE, b)
    f.PressureSolve()
    f.Synchronize()
    n = f.GetPressureSolver()["max_levels"]
    assert same_bits(f.DownloadPressureLevel(0, 1), b) and same_bits(f.download(fx.FIELD_DIVERGENCE), b)      # an input only
    got = f.download(fx.FIELD_PRESSURE)
    assert same_bits(f.DownloadPressureLevel(0, 0), got)
    return got, [None] + [(f.DownloadPressureLevel(l, 0), f.DownloadPressureLevel(l, 1)) for l in range(1, n)]


def assert_same_solve(got, want, what):
    (gp, gl), (wp, wl) = got, want
    assert len(gl) == len(wl), what
    for l in range(len(wl) - 1, 0, -1):                    # coarsest first: the first level that differs names the stage
        assert same_bits(gl[l][1], wl[l][1]), (what, "right-hand side of level", l)
        assert same_bits(gl[l][0], wl[l][0]), (what, "correction of level", l)
    assert same_bits(gp, wp), (what, "pressure")


# ---- 1: the solve against the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES)
def test_solve_matches_the_model(dims):
    p, b = fields(dims, 907)
    f = make(dims)
    for name, prm in variants(dims):
        set_solver(f, prm)
        levels = mg.plan(dims, prm["max_levels"])
        assert f.GetPressureSolver()["max_levels"] == len(levels)
        want = mg.solve(p, b, prm)
        assert not same_bits(want[0], p)
        assert_same_solve(solve_on_device(f, p, b), want, name)
    f.Release()
    assert (len(mg.plan(dims)) == 1) == (dims in ONE_LEVEL)


@pytest.mark.parametrize("dims", V4)
def test_both_sweep_kernels_match_the_model(dims):
    """no switch of the shipped library reaches the scalar sweep on a grid the wide one serves; both are held to the model instead: the wide one
    on this grid's level 0, the scalar one on a grid one cell longer in x and y (X % 4 = 1) that holds the same values"""
    X, Y, Z = dims
    p, b = fields((X + 1, Y + 1, Z), 911)
    omega = f32(6.0 / 7.0)
    for cut in (X, X + 1):
        f = make((cut, cut, Z))
        pc, bc = np.ascontiguousarray(p[:, :cut, :cut]), np.ascontiguousarray(b[:, :cut, :cut])
        f.SetPressureSolver("multigrid", cycles=1, coarse_sweeps=3, max_levels=1, omega=float(omega))
        got, _ = solve_on_device(f, pc, bc)
        f.Release()
        assert same_bits(got, mg.smooth(pc, bc, omega, 3)), cut


# ---- 2: the tail ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 32, 32), (20, 20, 8), (64, 64, 1), (128, 128, 1)])       # ... (128, 128, 1): level 1 is exactly 4096 cells
def test_the_tail_equals_the_launches_per_level(dims):
    p, b = fields(dims, 919)
    levels = mg.plan(dims)
    assert mg.tail_level(levels) == 1
    assert dims != (128, 128, 1) or levels[1][0] * levels[1][1] == 4096
    out = []
    for flags in (0, capi.MG_NO_TAIL):
        f = make(dims)
        f.timing_enable()
        for name, prm in variants(dims)[:2] + variants(dims)[4:]:
            set_solver(f, prm, flags)
            assert f.GetPressureSolver()["flags"] == flags
            out.append((name, flags, solve_on_device(f, p, b)))
        f.Synchronize()
        t = f.timing_read()
        out.append(("launches", flags, (int(t.jacobi_launches), int(t.jacobi_sweeps))))
        f.Release()
    half = len(out) // 2
    for (name, _, a), (_, _, c) in zip(out[:half - 1], out[half:-1]):
        assert_same_solve(a, c, name)
    # level-0 sweeps: 2 x (2 + 2), 2 x (0 + 1), 3 x (2 + 2); with the tail a cycle is its level-0 sweeps, the restriction, the tail, the prolongation
    assert out[half - 1][2] == (8 + 2 * 3 + 2 + 2 * 3 + 12 + 3 * 3, 8 + 2 + 12)
    assert out[-1][2][1] == 8 + 2 + 12 and out[-1][2][0] > out[half - 1][2][0]


# ---- 3: fx_simulate is the composition of the stage calls ---------------------------------------------------------------------------------------
def run_steps(dims, staged, extra, solver=True, **kw):
    _, vel0, _, col = rand_state(dims, 929, half=kw.get("storage") == "fp16", cells=0.3)
    f = make(dims, jacobi_iters=10, **kw)
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)
    if solver:
        f.SetPressureSolver("multigrid")
    if extra == "everything":
        f.SetEmitters([er.emitter((0.5, 0.3, 0.5), 0.2, color_rate=(1.0, 2.0, 3.0, 4.0), force=(5.0, 20.0, -3.0), swirl=30.0)])
        f.SetBuoyancy(**br.params(ambient=0.25, density_weight=0.7, lift=1.5, cooling=0.4, up=(0.3, 1.0, -0.2)))
        f.SetHeatSources(br.list_a()[:3])
        f.SetVorticityConfinement(4.0)
        f.SetAdvectionScheme("maccormack")
    dt = time_step(dims)
    for i in range(4):
        f.UpdateFrame(dt, i % 3)
        if staged:
            f.Advect(); f.OpenInflow(); f.Emit(); f.Heat(); f.EnforceObstacles(); f.ConfineVorticity()
            f.Divergence(); f.PressureSolve(); f.Project()
        else:
            f.Simulate(i % 3)
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS]
    f.Release()
    return out


@pytest.mark.parametrize("dims,storage,extra", [((32, 32, 32), "fp32", None), ((32, 32, 32), "fp16", None), ((64, 64, 1), "fp32", None),
                                                ((32, 32, 32), "fp32", "everything"), ((64, 64, 1), "fp16", "everything")])
def test_simulate_is_the_stage_composition(dims, storage, extra):
    whole = run_steps(dims, False, extra, storage=storage)
    assert whole == run_steps(dims, True, extra, storage=storage)
    assert whole[4] != run_steps(dims, False, extra, solver=False, storage=storage)[4]      # ... and the solver matters to the pressure


def test_pressure_solve_is_the_jacobi_stage_by_default():
    dims = (32, 32, 32)
    assert run_steps(dims, True, None, solver=False) == run_steps(dims, False, None, solver=False)


# ---- 4: off means off ---------------------------------------------------------------------------------------------------------------------------
def run_default(dims, touch):
    f = make(dims, jacobi_iters=12)
    assert f.GetPressureSolver()["kind"] == capi.PRESSURE_JACOBI and f.GetPressureSolver()["max_levels"] == 1
    if touch:
        f.SetPressureSolver("multigrid")
        assert f.GetPressureSolver()["kind"] == capi.PRESSURE_MULTIGRID
        f.UpdateFrame(time_step(dims), 0)
        assert f.GetPressureSolver()["kind"] == capi.PRESSURE_MULTIGRID      # configuration: kept across fx_update_frame
        f.SetPressureSolver("multigrid", cycles=1)                            # (again)
        f.SetPressureSolver("jacobi")
        assert f.GetPressureSolver() == dict(kind=0, flags=0, cycles=0, pre_sweeps=0, post_sweeps=0, coarse_sweeps=0, max_levels=1, omega=0.0)
    else:
        f.UpdateFrame(time_step(dims), 0)                                     # (the same parity history)
    dt = time_step(dims)
    for k in range(6):
        f.UpdateFrame(dt, k % 3)
        f.Simulate(k % 3)
    f.Synchronize()
    out = [f.digest(k) for k in ALL_FIELDS]
    f.Release()
    return out


@pytest.mark.parametrize("dims", [(70, 70, 6), (64, 64, 1)])
def test_set_and_reset_is_never_set(dims):
    assert run_default(dims, False) == run_default(dims, True)


@pytest.mark.parametrize("dims", [(64, 64, 4), (70, 70, 4), (36, 36, 1)])
def test_jacobi_stage_is_unchanged_while_multigrid_is_set(dims):
    p, b = fields(dims, 937)
    f = make(dims)
    f.SetPressureSolver("multigrid")
    f.upload(fx.FIELD_PRESSURE, p); f.upload(fx.FIELD_DIVERGENCE, b)
    f.Jacobi(5)
    f.Synchronize()
    got = f.download(fx.FIELD_PRESSURE)
    f.Release()
    assert same_bits(got, open_ref.ref_jacobi(p, b, None, 0, 5))


# ---- 5: resume ----------------------------------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_identically(tmp_path):
    dims = (32, 32, 32)
    path = str(tmp_path / "multigrid.fxck")

    def steps(f, first, count):
        dt = time_step(dims)
        for k in range(first, first + count):
            f.UpdateFrame(dt, k % 3)
            f.Simulate(k % 3)
        f.Synchronize()
    a = make(dims, jacobi_iters=10)
    a.SetPressureSolver("multigrid")
    steps(a, 0, 3)
    a.SaveCheckpoint(path)
    steps(a, 3, 3)
    b = make(dims, jacobi_iters=10)
    b.LoadCheckpoint(path)
    assert b.GetPressureSolver()["kind"] == capi.PRESSURE_JACOBI          # configuration is not stored
    b.SetPressureSolver("multigrid")
    steps(b, 3, 3)
    assert [a.digest(k) for k in ALL_FIELDS] == [b.digest(k) for k in ALL_FIELDS]
    c = make(dims, jacobi_iters=10)                                      # ... and the solver matters to those steps
    c.LoadCheckpoint(path)
    steps(c, 3, 3)
    assert c.digest(fx.FIELD_PRESSURE) != a.digest(fx.FIELD_PRESSURE)
    for f in (a, b, c):
        f.Release()


# ---- 6: refusals and state codes ----------------------------------------------------------------------------------------------------------------
def solver(**kw):
    v = dict(kind=capi.PRESSURE_MULTIGRID, flags=0, cycles=2, pre_sweeps=2, post_sweeps=2, coarse_sweeps=16, max_levels=0, omega=0.8)
    v.update(kw)
    return capi.PressureSolver(*[v[name] for name, _ in capi.PressureSolver._fields_])


def test_status_codes():
    lib = capi.load()
    dims = (32, 32, 32)
    f = make(dims)
    got = capi.PressureSolver()
    buf = np.empty(dims[::-1], f32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.fx_get_pressure_solver(f._ctx, None) == capi.FX_E_INVALID
    assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver())) == capi.FX_OK
    good = f.GetPressureSolver()
    assert good["max_levels"] == 5 and good["cycles"] == 2
    bad = [dict(kind=2), dict(kind=0xFFFFFFFF), dict(flags=2), dict(flags=0x80000001), dict(cycles=0), dict(cycles=65), dict(pre_sweeps=65),
           dict(post_sweeps=65), dict(coarse_sweeps=0), dict(coarse_sweeps=257), dict(max_levels=13), dict(omega=0.0), dict(omega=-0.5),
           dict(omega=1.0000001), dict(omega=float("nan")), dict(omega=float("inf"))]
    for kw in bad:
        assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver(**kw))) == capi.FX_E_INVALID, kw
        assert f.GetPressureSolver() == good, kw                          # the previous setting stays in force
    for kw in (dict(cycles=64, pre_sweeps=0, post_sweeps=0, coarse_sweeps=1, omega=1.0), dict(cycles=1, pre_sweeps=64, post_sweeps=64, coarse_sweeps=256, max_levels=12)):
        assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver(**kw))) == capi.FX_OK, kw
    assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver(max_levels=2))) == capi.FX_OK and f.GetPressureSolver()["max_levels"] == 2
    with pytest.raises(ValueError):
        f.SetPressureSolver("cg")

    # the levels: what is there, exact sizes only
    small = np.empty((16, 16, 16), f32)
    sp = small.ctypes.data_as(C.c_void_p)
    for what in (0, 1):
        assert lib.fx_download_pressure_level(f._ctx, 0, what, ptr, buf.nbytes) == capi.FX_OK
        assert lib.fx_download_pressure_level(f._ctx, 1, what, sp, small.nbytes) == capi.FX_OK
        assert lib.fx_download_pressure_level(f._ctx, 1, what, sp, small.nbytes - 4) == capi.FX_E_INVALID
        assert lib.fx_download_pressure_level(f._ctx, 2, what, sp, small.nbytes) == capi.FX_E_INVALID      # max_levels = 2: no such level
        assert lib.fx_download_pressure_level(f._ctx, 1, what, None, small.nbytes) == capi.FX_E_INVALID
    assert lib.fx_download_pressure_level(f._ctx, 0, 2, ptr, buf.nbytes) == capi.FX_E_INVALID

    # obstacles and open walls, both orders
    solid = masks(dims)["ball"]
    assert lib.fx_set_obstacles(f._ctx, None, solid.ctypes.data, solid.nbytes, 0) == capi.FX_E_STATE
    assert lib.fx_set_obstacles(f._ctx, None, None, 0, 0) == capi.FX_OK                       # detaching nothing is no conflict
    assert lib.fx_set_open_walls(f._ctx, capi.WALL_Y_HI) == capi.FX_E_STATE and lib.fx_set_open_walls(f._ctx, 0) == capi.FX_OK
    assert f.GetOpenWalls() == 0 and f.GetPressureSolver()["kind"] == capi.PRESSURE_MULTIGRID
    assert lib.fx_set_pressure_solver(f._ctx, None) == capi.FX_OK and f.GetPressureSolver()["kind"] == capi.PRESSURE_JACOBI
    assert lib.fx_download_pressure_level(f._ctx, 1, 0, sp, small.nbytes) == capi.FX_E_INVALID  # the pyramid is gone
    assert lib.fx_download_pressure_level(f._ctx, 0, 0, ptr, buf.nbytes) == capi.FX_OK
    f.SetObstacles(solid)
    assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver())) == capi.FX_E_STATE
    assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver(kind=capi.PRESSURE_JACOBI))) == capi.FX_OK
    f.SetObstacles(None)
    f.SetOpenWalls(capi.WALL_X_LO)
    assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver())) == capi.FX_E_STATE and f.GetPressureSolver()["kind"] == capi.PRESSURE_JACOBI
    f.SetOpenWalls(0)
    assert lib.fx_set_pressure_solver(f._ctx, C.byref(solver())) == capi.FX_OK

    faithful = make((64, 64, 16), jacobi_mode="faithful", jacobi_iters=16)
    assert lib.fx_set_pressure_solver(faithful._ctx, C.byref(solver())) == capi.FX_E_INVALID
    assert lib.fx_set_pressure_solver(faithful._ctx, None) == capi.FX_OK
    assert lib.fx_get_pressure_solver(faithful._ctx, C.byref(got)) == capi.FX_OK and got.kind == capi.PRESSURE_JACOBI

    # slab ranks: a lone slab context, and the members of an in-process group
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, dims, slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)

    def slab_refusals(r):
        assert lib.fx_set_pressure_solver(r._ctx, C.byref(solver())) == capi.FX_E_INVALID and lib.fx_set_pressure_solver(r._ctx, None) == capi.FX_E_INVALID
        assert r.GetPressureSolver()["kind"] == capi.PRESSURE_JACOBI      # (slab ranks may ask)
        assert lib.fx_download_pressure_level(r._ctx, 0, 0, ptr, buf.nbytes) == capi.FX_E_INVALID
    for r in ranks:
        slab_refusals(r)
    fx.comm_init_local(ranks)
    ranks[0].UpdateFrame(time_step(dims), 0)
    for r in ranks:
        slab_refusals(r)
        assert lib.fx_pressure_solve(r._ctx, None) == capi.FX_E_INVALID  # the stage call of a rank of a chain, as fx_jacobi

    ro = fx.Fluid()
    assert ro.Init(64, 64, dims, render_only=True)
    assert lib.fx_set_pressure_solver(ro._ctx, C.byref(solver())) == capi.FX_E_STATE and lib.fx_set_pressure_solver(ro._ctx, None) == capi.FX_E_STATE
    assert lib.fx_set_pressure_solver(ro._ctx, C.byref(solver(kind=9))) == capi.FX_E_STATE      # ... whatever else is wrong with the call
    assert lib.fx_get_pressure_solver(ro._ctx, C.byref(got)) == capi.FX_E_STATE
    assert lib.fx_pressure_solve(ro._ctx, None) == capi.FX_E_STATE
    assert lib.fx_download_pressure_level(ro._ctx, 0, 0, ptr, buf.nbytes) == capi.FX_E_STATE
    for o in [f, faithful, ro] + ranks:
        o.Release()


# ---- 7: what the solver is for, on the device ---------------------------------------------------------------------------------------------------
def test_one_solve_leaves_less_than_half_of_forty_jacobi_sweeps_on_the_device():
    """the 32^3 case of tests/test_multigrid_ref.py, the same arrays and the same factor"""
    dims = (32, 32, 32)
    b = mg.plume_rhs(dims)
    zero = np.zeros(dims[::-1], f32)
    f = make(dims)
    f.SetPressureSolver("multigrid")
    got, _ = solve_on_device(f, zero, b)
    f.SetPressureSolver("jacobi")
    f.upload(fx.FIELD_PRESSURE, zero)
    f.Jacobi(40)
    f.Synchronize()
    jac = f.download(fx.FIELD_PRESSURE)
    f.Release()
    r0 = mg.rms_residual(zero, b)
    rm, rj = mg.rms_residual(got, b) / r0, mg.rms_residual(jac, b) / r0
    print("32^3 on the device: multigrid %.4f, 40 Jacobi sweeps %.4f of the initial residual" % (rm, rj))
    assert same_bits(got, mg.solve(zero, b)[0]) and same_bits(jac, open_ref.ref_jacobi(zero, b, None, 0, 40))
    assert rm <= 0.5 * rj
