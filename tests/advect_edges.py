"""Input recipes of tests/test_gpu_advect_edges.py: the states that drive the STAGED advection (csrc/fx_advect_lds.hip: k_advect_lds and
k_advect_far) to the edges its gather kernels (k_advect / k_advect_fast) are held to, with the references' outputs for them.

  geometry   the five grids of PLAN -- the smallest at which the staged path has full tiles through the power-of-two and the general code, a last
             x tile of one lane and of 63, a last tile row of one wave and of seven, the minimum of 12 planes and a chunk of one plane -- under
             random velocities from well inside the staged window (scale 0.2) to far outside (12), half of the rows slowed down
  recipe A   fp16 stores into the binary16 subnormals and of -0 (tests/test_gpu_stage_matrix.py half_range_state, reused)
  recipe B   fp32 fields of subnormals
  recipe C   +inf, -inf and NaN planted into every velocity component and every colour channel, fp32 and fp16

Two references.  The model: maccormack_ref.step(scheme="semi-lagrangian", impulse=False) -- k_advect's arithmetic in numpy, exact (tests/
fma_ref.py), over the whole field with the built-in impulse switched off (fx_set_impulse(0): no transcendental).  The oracle: orc.advect, with
the impulse, outside its ball.  tests/test_advect_edges.py holds every Case to its conditions and the two references to each other on the CPU
alone; the GPU tests assert the conditions again and then compare bit for bit.  "In-window": |u_a| dt N_a < 1 on all three axes, from the
inputs -- only used to show that the voxels the staged kernel serves from its window and the ones it hands to the gathers both exist.

PLAN is what fx::advect_lds_plan (csrc/fx_advect_plan.cpp) answers for each grid under ADVECT_LDS = 2; tests/test_advect_edges.py asks it."""
import functools

import numpy as np

import maccormack_ref as mr
from oracle import orc
from store_edges import assert_conditions, bits, case, same_bits, time_step, to_half                       # noqa: F401  (the tests take them from here)
from test_gpu_stage_matrix import far_from_the_impulse, half_bits, half_classes, half_range_state, subnormal_share

f32 = np.float32
# grid -> P2, (x tiles, lanes in the last), (tile rows, rows in the last), planes per chunk while deferring
PLAN = {
    (64, 64, 16): dict(p2=True, x=(1, 64), y=(8, 8), chunks=[16]),               # the smallest power-of-two grid, one chunk
    (64, 64, 12): dict(p2=False, x=(1, 64), y=(8, 8), chunks=[8, 4]),            # the minimum of 12 planes; full tiles through the general code
    (65, 65, 17): dict(p2=False, x=(2, 1), y=(9, 1), chunks=[8, 8, 1]),          # one live lane, one live wave, a chunk of one plane
    (127, 127, 13): dict(p2=False, x=(2, 63), y=(16, 7), chunks=[8, 5]),         # one missing lane, one missing row
    (129, 129, 12): dict(p2=False, x=(3, 1), y=(17, 1), chunks=[8, 4]),          # a third tile of one lane
}
SHAPES = list(PLAN)
RANGE_SHAPES = [(64, 64, 16), (65, 65, 17), (129, 129, 12)]
ALPHA_SHAPES = [(64, 64, 16), (65, 65, 17)]
STORAGES = ["fp32", "fp16"]
ADDRESSES = ["clamp", "mirror"]
SCALES = [0.2, 3.0, 12.0]
# the shipped switches of the three kernel settings: staged + k_advect_far | staged, gathers inside the kernel | k_advect_fast / k_advect
KERNELS = {"staged": {"ADVECT_LDS": "2", "ADVECT_DEFER": "1"}, "inline": {"ADVECT_LDS": "2", "ADVECT_DEFER": "0"}, "gather": {"ADVECT_LDS": "0"}}
PLANT = 0.002                                                # share of +inf, of -inf and of NaN in every plane of recipe C


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def in_window(vel, dims, dt):
    """[Z][Y][X]: the back-trace moves less than a cell along every axis (False where the voxel's own velocity is not finite)"""
    with np.errstate(invalid="ignore"):
        return np.logical_and.reduce([np.abs(vel[a]).astype(np.float64) * float(dt) * n < 1 for a, n in enumerate(dims)])


def references(vel, col, dt, address, half):
    """(model velocity, model colour, oracle velocity, oracle colour); the model without the impulse, the oracle with it"""
    with np.errstate(all="ignore"):
        mv, mc = mr.step(vel, col, dt, address, impulse=False, half=half, scheme="semi-lagrangian")
        ov, oc = orc.advect(vel, col, dt, address=int(address == "mirror"), half=half)
    return mv, mc, ov, oc


def build(what, dims, vel, col, address, half, conditions):
    dt = time_step(dims)
    mv, mc, ov, oc = references(vel, col, dt, address, half)
    return case(what=what, dims=dims, vel=vel, col=col, dt=dt, address=address, half=half, storage="fp16" if half else "fp32", want_vel=mv, want_col=mc,
                orc_vel=ov, orc_col=oc, far=far_from_the_impulse(dims), inwin=in_window(vel, dims, dt), conditions=conditions)


def values(c, sel, vel=None, col=None):
    """the seven stored quantities of the voxels `sel` [Z][Y][X] as one vector (the model's unless given)"""
    vel, col = c.want_vel if vel is None else vel, c.want_col if col is None else col
    return np.concatenate([vel[:, sel].ravel(), col[sel].ravel()])


def same_but_nan(got, want):
    """NaN exactly where `want` has NaN (payload unspecified), every other value bit for bit -> (equal, differing count, first places)"""
    n = np.isnan(want)
    bad = (np.isnan(got) != n) | ((bits(got) != bits(want)) & ~n)
    return not bad.any(), int(bad.sum()), np.argwhere(bad)[:6].tolist()


def agree_outside_the_ball(c):
    """the model and the oracle on the voxels the impulse does not touch: the link from the model to the pinned oracle"""
    far = c.far
    return same_but_nan(c.want_vel[:, far], c.orc_vel[:, far])[0] and same_but_nan(c.want_col[far], c.orc_col[far])[0]


def populations(c):
    return (("in-window", c.inwin), ("far", ~c.inwin))


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def geometry(dims, storage, address, scale):
    """tests/test_gpu_sim.py test_advect_lds_path_bit_identical's state: waves that stay inside the window and waves that leave it in one workgroup"""
    X, Y, Z = dims
    rng = np.random.default_rng(7700 + X + 7 * Z + int(scale * 10))
    vel = (rng.standard_normal((3, Z, Y, X)) * scale).astype(f32)
    vel[:, :, : Y // 2] *= f32(0.05)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    half = storage == "fp16"
    if half:
        vel, col = to_half(vel), to_half(col)
    what = "geometry %s %s %s %g" % (dims, storage, address, scale)
    c = build(what, dims, vel, col, address, half, [])
    c.conditions.append((what + ": NaN count of the model", float(np.isnan(c.want_vel).sum() + np.isnan(c.want_col).sum()), "==", 0.0))
    return c


# ---- recipe A: binary16 subnormals and -0 -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def half_edges(dims, address):
    vel, col, _ = half_range_state(dims)
    what = "A %s %s" % (dims, address)
    c = build(what, dims, vel, col, address, True, [])
    c.conditions.append((what + ": in-window share", float(c.inwin.mean()), ">=", 0.1))
    c.conditions.append((what + ": far share", float(1 - c.inwin.mean()), ">=", 0.1))
    for name, sel in populations(c):
        sub, inf, nz, nan = (float(v) for v in half_classes(half_bits(values(c, sel))))
        c.conditions += [("%s %s: subnormal share" % (what, name), sub, ">=", 0.02), ("%s %s: -0 share" % (what, name), nz, ">=", 2e-4),
                         ("%s %s: NaN share" % (what, name), nan, "==", 0.0), ("%s %s: inf share" % (what, name), inf, "==", 0.0)]
    return c


# ---- recipe B: fp32 subnormals ----------------------------------------------------------------------------------------------------------------
TINY = 2.0 ** -128                                           # standard_normal * 2^-128: below the smallest normal (2^-126) up to four sigma


@functools.lru_cache(maxsize=None)
def subnormal(dims, address):
    """colour subnormal everywhere; velocity subnormal in the rows y < Y / 2 (every trace stays in its cell) and standard_normal * 3 above (most
    traces leave the window: the gathers see subnormal taps too)"""
    X, Y, Z = dims
    rng = np.random.default_rng(7804 + X + 7 * Z)           # (a seed at which (129, 129, 12) holds a tie that a twice-rounded fma gets wrong: tests/test_fma_ref.py)
    col = (rng.standard_normal((Z, Y, X, 4)) * TINY).astype(f32)
    vel = (rng.standard_normal((3, Z, Y, X)) * TINY).astype(f32)
    vel[:, :, Y // 2:] = (rng.standard_normal((3, Z, Y - Y // 2, X)) * 3).astype(f32)
    what = "B %s %s" % (dims, address)
    c = build(what, dims, vel, col, address, False, [])
    share = float(c.inwin.mean())
    c.conditions += [(what + ": in-window share", share, ">=", 0.3), (what + ": far share", 1 - share, ">=", 0.3)]
    for name, sel in populations(c):
        c.conditions.append(("%s %s: subnormal and non-zero share of the colour" % (what, name), subnormal_share(c.want_col[sel]), ">", 0.99))
    c.conditions.append((what + " in-window: subnormal and non-zero share of the velocity", subnormal_share(c.want_vel[:, c.inwin]), ">", 0.95))
    return c


# ---- recipe C: non-finite values -------------------------------------------------------------------------------------------------------------
def plant(rng, a):
    """+inf, -inf and NaN into PLANT of the cells each, independently (a later one overwrites an earlier one)"""
    for v in (np.inf, -np.inf, np.nan):
        a[rng.random(a.shape) < PLANT] = v
    return a


@functools.lru_cache(maxsize=None)
def nonfinite_state(dims):
    X, Y, Z = dims
    rng = np.random.default_rng(7900 + X + 7 * Z)
    vel = rng.standard_normal((3, Z, Y, X)).astype(f32)
    vel[:, :, : Y // 2] *= f32(0.05)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    vel, col = to_half(vel), to_half(col)
    for a in range(3):
        plant(rng, vel[a])
    for i in range(4):
        plant(rng, col[..., i])
    vel.setflags(write=False); col.setflags(write=False)
    return vel, col


def own_velocity_not_finite(c):
    return ~np.isfinite(c.vel).all(axis=0)


def all_seven_nan(sel, vel, col):
    return bool(np.isnan(vel[:, sel]).all() and np.isnan(col[sel]).all())


@functools.lru_cache(maxsize=None)
def nonfinite(dims, storage, address):
    """the state holds binary16 values, so one state serves both storages.  A voxel whose own velocity is not finite has a NaN fraction on
    that axis (inf - inf, or NaN): every lerp along it is NaN whatever the taps hold -- all seven stored quantities are NaN"""
    vel, col = nonfinite_state(dims)
    what = "C %s %s %s" % (dims, storage, address)
    c = build(what, dims, vel, col, address, storage == "fp16", [])
    lost = own_velocity_not_finite(c)
    share = float(c.inwin.mean())
    c.conditions += [(what + ": in-window share (own velocity finite)", share, ">=", 0.3), (what + ": share of the other voxels", 1 - share, ">=", 0.2),
                     (what + ": voxels whose own velocity is not finite", float(lost.sum()), ">=", 100.0),
                     (what + ": ... and the model stores NaN in all seven quantities there", float(all_seven_nan(lost, c.want_vel, c.want_col)), "==", 1.0)]
    for name, sel in populations(c):
        v = values(c, sel)
        c.conditions += [("%s %s: NaN share" % (what, name), float(np.isnan(v).mean()), ">=", 0.01), ("%s %s: inf share" % (what, name), float(np.isinf(v).mean()), ">=", 1e-3)]
    return c
