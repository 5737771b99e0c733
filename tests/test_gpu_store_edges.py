"""The optional stages of the step at the edges of their number formats, BIT FOR BIT against their models -- there is no tolerance in this file.

The kernels of fx_vorticity.hip, fx_emit.hip, fx_heat.hip, fx_obstacle.hip, fx_open.hip, fx_maccormack.hip and fx_multigrid.hip read and write
their fields through csrc/fx_store.h (Cell<HALF>, Sto<HALF>, to_h16, Off<WIDE>), not through the Store<HALF> of fx_sim.hip that
tests/test_gpu_stage_matrix.py holds to these ranges.  Their own test files draw every field from standard_normal * O(1) and random(); here:

  part 1  fp16 storage: stores into the binary16 subnormal range, across the overflow boundary (65504 | 65520 -> inf) and of -0, as bit patterns
          -- a kernel that flushed, clamped or rounded twice there would fail;
  part 2  fp32 storage: fields of fp32 subnormals through the confinement's sqrtf and /, the boundary-aware divergence / sweeps / projection,
          a multigrid solve and the field passes -- the library keeps denormals, and so do the models;
  part 3  the WIDE = true instantiations (64-bit byte offsets, taken from 2^28 cells on), which no other test executes, on the lab build
          with the switch WIDE_OFFSETS.

The inputs and the models' outputs are the cases of tests/store_edges.py; every test asserts the case's conditions -- statements about the
MODEL's output, which tests/test_store_edges.py also holds without a GPU -- before it compares.  Parts 1 and 2 set no launcher switch: they
run on the shipped library.  Out of scope: NaN and inf among the inputs, grids of 2^28 cells and more, slab ranks, the render paths."""
import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import multigrid_ref as mg
import store_edges as se
from store_edges import ids, bits
from test_gpu_stage_matrix import half_bits
from test_gpu_multigrid import set_solver, solve_on_device, assert_same_solve, fields as mg_fields

pytestmark = pytest.mark.gpu
ADDRESSES = ["clamp", "mirror"]
STORAGES = ["fp32", "fp16"]


@pytest.fixture(autouse=True)
def quiet_casts():
    with np.errstate(over="ignore"):                         # the models round past 65504 to inf on purpose
        yield


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status            # simulation only: no viewport
    return f


def explain(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    return "%d of %d differ; first at %s: got %r (%#x) want %r (%#x)" % (len(bad), got.size, i, got[i], bits(got)[i], want[i], bits(want)[i])


def assert_same(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (what, explain(got, want))


def assert_same_half(got, want, what=""):
    """as bit patterns of binary16 (half_bits asserts that what the download returned is representable)"""
    assert np.array_equal(half_bits(got), half_bits(want)), (what, explain(got, want))


# ---- the stages, each from a case of store_edges.py ----------------------------------------------------------------------------------------
def run_vorticity(c, dims, storage):
    f = make(dims, storage=storage)
    f.upload(fx.FIELD_VELOCITY1, c.vel)
    f.UpdateFrame(c.dt, 0)
    f.SetVorticityConfinement(c.eps)
    f.ConfineVorticity()
    f.Synchronize()
    out = f.download(fx.FIELD_VELOCITY1)
    f.Release()
    return out


def run_emit(c, dims, storage):
    f = make(dims, storage=storage)
    f.UpdateFrame(c.dt, 0)
    f.upload(fx.FIELD_VELOCITY1, c.vel); f.upload(fx.FIELD_COLOR, c.col)
    f.SetEmitters(c.emitters)
    f.Emit()
    f.Synchronize()
    out = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.Release()
    return out


def run_heat(c, dims, storage, address="clamp"):
    f = make(dims, storage=storage, advect_address=address)
    f.SetBuoyancy(**c.prm)
    f.SetHeatSources([])
    f.UpdateFrame(c.dt, 0)
    f.upload(fx.FIELD_VELOCITY, c.vel0); f.upload(fx.FIELD_VELOCITY1, c.vel1); f.upload(fx.FIELD_COLOR, c.col); f.upload(fx.FIELD_TEMPERATURE, c.T)
    f.Heat()
    f.Synchronize()
    out = f.download(fx.FIELD_TEMPERATURE), f.download(fx.FIELD_VELOCITY1)
    f.Release()
    return out


def run_inflow(c, dims, storage):
    f = make(dims, storage=storage)
    f.UpdateFrame(c.dt, 0)
    f.upload(fx.FIELD_VELOCITY, c.vel0)
    f.SetOpenWalls(c.faces)
    f.upload(fx.FIELD_COLOR, c.col)
    f.OpenInflow()
    f.Synchronize()
    out = f.download(fx.FIELD_COLOR)
    f.Release()
    return out


def run_maccormack(vel0, col, dt, dims, storage, address):
    f = make(dims, storage=storage, advect_address=address)
    f.SetAdvectionScheme(capi.ADVECT_MACCORMACK)
    f.SetImpulse(0)
    f.upload(fx.FIELD_VELOCITY, vel0); f.upload(fx.FIELD_COLOR, col)      # (UpdateFrame flips the parity: the advection reads this colour)
    f.UpdateFrame(dt, 0)
    f.Advect()
    f.Synchronize()
    out = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.Release()
    return out


def bounded(dims, c, **kw):
    """a context under one of the three settings of the boundary-aware kernels"""
    f = make(dims, **kw)
    f.SetObstacles(c.mask)
    f.SetOpenWalls(c.faces)
    f.UpdateFrame(se.time_step(dims), 0)
    return f


# ---- part 1: binary16 edges, fp16 storage -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps,overflow", se.VORTICITY_HALF)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_fp16_vorticity_stores_every_binary16_range(dims, eps, overflow):
    """two cases on one state: epsilon = 1e-3 stores subnormals and -0 and cannot overflow, epsilon = 8 pushes velocities past 65504"""
    c = se.vorticity_half(dims, eps)
    se.assert_conditions(c)
    assert_same_half(run_vorticity(c, dims, "fp16"), c.want)


@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_fp16_emitters_store_every_binary16_range(dims):
    """bit for bit INSIDE the supports too: with force = 0 and swirl != 0 the force is dz * -swirl and dx * swirl exactly, and every colour
    rate is 0 or 1e9, so no stored bit depends on the last bits of exp2 (tests/test_store_edges.py perturbs the basis to show it; the
    precondition near_threshold == 0 is one of the case's conditions).  Swirl 1e-4 reaches the subnormals, 3e6 the overflow.
    Left out: -0 among the colour inputs -- saturate(-0) is a maximum of -0 and +0, whose result neither IEEE 754 nor numpy fixes.
    On the 2-D grid the force has no swirl term and is 0: the velocity comes back as it was, its subnormals included, but for -0 -> +0"""
    c = se.emit_half(dims)
    se.assert_conditions(c)
    gv, gc = run_emit(c, dims, "fp16")
    m = c.touched
    assert_same_half(gv[:, ~m], c.vel[:, ~m], "outside"); assert_same_half(gc[~m], c.col[~m], "outside")
    assert_same_half(gv, c.want_vel); assert_same_half(gc, c.want_col)


@pytest.mark.parametrize("address", ADDRESSES)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_fp16_buoyancy_force_stores_every_binary16_range(dims, address):
    """no sources: the pass uses no transcendental and is exact everywhere, the (fp32) temperature included"""
    c = se.heat_half(dims, address)
    se.assert_conditions(c)
    gT, gv = run_heat(c, dims, "fp16", address)
    assert_same(gT, c.want_T, "temperature")
    assert_same_half(gv, c.want, "VELOCITY1")


@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_fp16_inflow_stores_every_binary16_range(dims):
    """every legal face open.  The blend towards clear air cannot overflow; it produces subnormals and -0 in plenty"""
    c = se.inflow_half(dims)
    se.assert_conditions(c)
    got = run_inflow(c, dims, "fp16")
    assert_same_half(got, c.want)
    assert_same_half(got[c.w == 1], c.col[c.w == 1])


@pytest.mark.parametrize("dims", se.BND_SHAPES, ids=ids)
def test_fp16_enforce_zeroes_the_solid_cells_and_nothing_else(dims):
    """solid cells that held -0, subnormals and +-65504 come back as +0 bits; no other cell changes a bit"""
    c = se.enforce_half(dims)
    se.assert_conditions(c)
    f = make(dims, storage="fp16")
    f.SetObstacles(c.mask)
    f.UpdateFrame(se.time_step(dims), 0)
    f.upload(fx.FIELD_VELOCITY1, c.vel); f.upload(fx.FIELD_COLOR, c.col)
    f.EnforceObstacles()
    gv, gc = f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR)
    f.Release()
    s = c.mask != 0
    assert not half_bits(gv)[:, s].any() and not half_bits(gc)[s].any()
    assert_same_half(gv[:, ~s], c.vel[:, ~s]); assert_same_half(gc[~s], c.col[~s])
    assert_same_half(gv, c.want_vel); assert_same_half(gc, c.want_col)


@pytest.mark.parametrize("name", se.PROJECT_SETTINGS)
@pytest.mark.parametrize("dims", se.BND_SHAPES, ids=ids)
def test_fp16_boundary_projection_stores_every_binary16_range(dims, name):
    """k_project_bnd under obstacles alone, open walls alone and both: the state has extra mass at both ends of the binary16 range"""
    c = se.project_half(dims, name)
    se.assert_conditions(c)
    f = bounded(dims, c, storage="fp16")
    f.upload(fx.FIELD_VELOCITY1, c.vel); f.upload(fx.FIELD_PRESSURE, c.p)
    assert_same_half(f.download(fx.FIELD_VELOCITY1), c.vel, "upload")      # the upload kept -0 and the subnormals
    f.Project()
    got = f.download(fx.FIELD_VELOCITY)
    f.Release()
    assert_same_half(got, c.want)


@pytest.mark.parametrize("address", ADDRESSES)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_fp16_maccormack_stores_every_binary16_range(dims, address):
    """the impulse off, so bit for bit everywhere.  No store can overflow: the result is limited to storable taps and then multiplied by an
    attenuation below 1"""
    c = se.maccormack_half(dims, address)
    se.assert_conditions(c)
    gv, gc = run_maccormack(c.vel0, c.col, c.dt, dims, "fp16", address)
    assert_same_half(gv, c.want_vel, "velocity"); assert_same_half(gc, c.want_col, "colour")


# ---- part 2: fp32 subnormals, fp32 storage ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["log", "all"])
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_fp32_vorticity_of_subnormal_fields(dims, kind):
    """"log": velocities log-uniform in 2^-140 .. 2^-60 -- the squares under the pass's sqrtf are subnormal in 0.3 of the cells and more, and
    the pass changes 0.15 of the cells and more: where a square root or a division that mishandles denormals would show.  "all":
    standard_normal * 2^-128, every input subnormal -- the model changes nothing, so the pass must return the field bit for bit (a kernel
    that flushed would return zeros)"""
    c = se.vorticity_subnormal(dims, kind)
    se.assert_conditions(c)
    got = run_vorticity(c, dims, "fp32")
    assert_same(got, c.want)
    if kind == "all":
        assert_same(got, c.vel)


@pytest.mark.parametrize("name", se.PROJECT_SETTINGS)
@pytest.mark.parametrize("dims", se.BND_SHAPES, ids=ids)
def test_fp32_boundary_solve_of_subnormal_fields(dims, name):
    """the boundary-aware divergence, five sweeps (k_jacobi_bnd; k_jacobi_bnd_v4 on (68, 68, 5)) and the boundary-aware projection on fields of
    standard_normal * 2^-128, under obstacles alone, open walls alone and both"""
    c = se.pressure_subnormal(dims, name)
    se.assert_conditions(c)
    f = bounded(dims, c, jacobi_iters=se.SWEEPS)
    f.upload(fx.FIELD_VELOCITY1, c.vel); f.upload(fx.FIELD_PRESSURE, c.p)
    f.EnforceObstacles()
    f.Divergence()
    assert_same(f.download(fx.FIELD_DIVERGENCE), c.b, "divergence")
    f.Jacobi(se.SWEEPS)
    assert_same(f.download(fx.FIELD_PRESSURE), c.q, "pressure")
    f.Project()
    got = f.download(fx.FIELD_VELOCITY)
    f.Release()
    assert_same(got, c.w, "velocity")


@pytest.mark.parametrize("dims", se.MG_SHAPES, ids=ids)
def test_fp32_multigrid_solve_of_subnormal_fields(dims):
    """one solve with the default parameters on standard_normal * 2^-131 (three octaves below the fields above: the coarse corrections grow
    the pressure): the pressure and every level's correction and right-hand side"""
    c = se.multigrid_subnormal(dims)
    se.assert_conditions(c)
    f = make(dims)
    set_solver(f, c.prm)
    got = solve_on_device(f, c.p, c.b)
    f.Release()
    assert_same_solve(got, c.want, "subnormal")


@pytest.mark.parametrize("which", se.FIELD_INPUTS)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_fp32_field_passes_of_subnormal_fields(dims, which):
    """MacCormack, fx_heat and fx_open_inflow on a subnormal colour and on a subnormal temperature with ambient = 0; the tracing velocity is
    an ordinary one that crosses cells (only the buoyancy pass reads the temperature: under the "temperature" input the other two run on its
    ordinary colour)"""
    c = se.field_subnormal(dims, which)
    se.assert_conditions(c)
    gv, gc = run_maccormack(c.vel0, c.col, c.dt, dims, "fp32", "clamp")
    assert_same(gv, c.mc_vel, "maccormack velocity"); assert_same(gc, c.mc_col, "maccormack colour")
    gT, gv = run_heat(c, dims, "fp32")
    assert_same(gT, c.heat_T, "temperature"); assert_same(gv, c.heat_vel, "VELOCITY1")
    assert_same(run_inflow(c, dims, "fp32"), c.inflow, "inflow")


# ---- part 3: the WIDE instantiations, on the lab build ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_wide_offset_kernels_match_the_models(dims, storage, knob):
    """WIDE_OFFSETS = 1 (a lab switch: the contexts run on the lab build) makes colour_wants_wide_offsets answer true on these small grids,
    so fx_emit, fx_heat, fx_open_inflow and the MacCormack fx_advect run k_emit, k_heat, k_open_inflow, k_mc_predict and k_mc_correct with
    WIDE = true, on the part-1 states (binary16 values: storable in both storages), bit for bit against the models.
    This executes every WIDE instantiation; it does not prove offsets beyond 2^32 -- that needs 2^28 cells and minutes of host time"""
    import buoyancy_ref as br
    import emitter_ref as er
    import maccormack_ref as mr
    import open_ref as orf
    knob("WIDE_OFFSETS", "1")
    half = storage == "fp16"
    c = se.emit_half(dims)
    gv, gc = run_emit(c, dims, storage)
    wv, wc, _ = er.apply(c.vel, c.col, c.emitters, c.dt, half=half)
    assert_same(gv, wv, "emit velocity"); assert_same(gc, wc, "emit colour")
    c = se.heat_half(dims)
    gT, gv = run_heat(c, dims, storage)
    wT, wv = br.apply(c.T, c.vel0, c.vel1, c.col, c.prm, [], c.dt, "clamp", half=half)
    assert_same(gT, wT, "heat temperature"); assert_same(gv, wv, "heat VELOCITY1")
    c = se.inflow_half(dims)
    assert_same(run_inflow(c, dims, storage), orf.ref_inflow(c.col, c.vel0, c.dt, c.faces, half=half), "inflow")
    for address in ADDRESSES:
        c = se.maccormack_half(dims, address)
        gv, gc = run_maccormack(c.vel0, c.col, c.dt, dims, storage, address)
        wv, wc = mr.step(c.vel0, c.col, c.dt, address, impulse=False, half=half)
        assert_same(gv, wv, "maccormack velocity " + address); assert_same(gc, wc, "maccormack colour " + address)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", [(70, 70, 4), (64, 64, 4)], ids=ids)
def test_wide_offset_multigrid_matches_the_model(dims, storage, knob):
    """WIDE_OFFSETS = 1 makes mg_wide answer true on every level: k_mg_smooth (rows of 70 cells), k_mg_smooth_v4 (rows of 64),
    k_mg_residual_restrict and k_mg_prolong_correct with WIDE = true, on the fields of tests/test_gpu_multigrid.py and on the subnormal ones.
    (The pressure is fp32 under either storage.)  The same limit as above: 64-bit offsets are executed, not driven beyond 2^32"""
    knob("WIDE_OFFSETS", "1")
    f = make(dims, storage=storage)
    prm = mg.defaults(dims)
    set_solver(f, prm)
    p, b = mg_fields(dims, 907)
    assert_same_solve(solve_on_device(f, p, b), mg.solve(p, b, prm), "default")
    c = se.multigrid_subnormal(dims)
    assert_same_solve(solve_on_device(f, c.p, c.b), c.want, "subnormal")
    f.Release()
