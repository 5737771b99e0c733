"""Every storage x row-class kernel of the step's non-Jacobi stages against the CPU oracle.

launch_divergence and launch_project (fluidx12_amd/csrc/fx_sim.hip) pick a kernel by storage type and by what divides the row length
(fx::sim_row_kernel): k_*_v4 (X % 4 == 0), k_*_vw<3> (fp32, X % 3 == 0), k_*_vw<2> (X even) and the scalar kernels (the rest).  SHAPES
below are the smallest at which each of them has an interior, both x edges, a partial block and both z faces; ROW_CLASS says which kernel
each takes in fp32 / fp16, and tests/test_stage_matrix.py (CPU) holds the library to it.  On every shape and both storages:
  * divergence and projection == oracle bit for bit; advection (clamp / mirror, taps within a cell and across every border) bit for bit
    outside the impulse ball and within the bars of test_gpu_sim.py::test_advect_lds_path_bit_identical over the whole field;
  * two whole steps from a random state, both Jacobi modes, one case per kernel;
  * fp16 only: stores into the binary16 subnormal range, across the overflow boundary (65504 | 65520 -> inf) and of -0, as bit patterns;
  * fp32 only: fields of fp32 subnormals through divergence, Jacobi (every shipped family of the default schedule) and projection, bit for
    bit -- the library keeps denormals and so does the oracle;
  * the new row classes in z-slabs == the single domain, on the shared-stream and the peer group;
  * fx_field_digest refuses ranges whose 32-bit sum wraps.
No test here sets a launcher switch: all of it runs on the shipped library."""
import ctypes as C
import functools

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi
from oracle import orc

pytestmark = pytest.mark.gpu
f32 = np.float32

# shape -> the kernel of the divergence / projection family it takes in (fp32, fp16)
ROW_CLASS = {
    (6, 6, 2): ("vw3", "vw2"), (10, 10, 3): ("vw2", "vw2"), (70, 70, 5): ("vw2", "vw2"), (130, 130, 4): ("vw2", "vw2"), (258, 258, 2): ("vw3", "vw2"),
    (9, 9, 3): ("vw3", "scalar"), (150, 150, 3): ("vw3", "vw2"), (201, 201, 3): ("vw3", "scalar"),
    (5, 5, 2): ("scalar", "scalar"), (35, 35, 4): ("scalar", "scalar"), (67, 67, 3): ("scalar", "scalar"), (131, 131, 2): ("scalar", "scalar"),
    (36, 36, 6): ("v4", "v4"), (260, 260, 2): ("v4", "v4"),
}
SHAPES = list(ROW_CLASS)
STORAGES = ["fp32", "fp16"]
# two whole steps: one case per kernel and storage in each Jacobi mode (faithful: the divergence runs inside k_freeze_dense)
STEP_CASES = [dict(dims=d, storage=s, mode=m, address=a, iters=n, scale=c)
              for m, n in (("fixed", 7), ("faithful", 24))
              for d, s, a, c in (((260, 260, 2), "fp32", "clamp", 1.0), ((201, 201, 3), "fp32", "mirror", 3.0), ((130, 130, 4), "fp32", "clamp", 0.2),
                                 ((67, 67, 3), "fp32", "mirror", 1.0), ((36, 36, 6), "fp16", "mirror", 1.0), ((150, 150, 3), "fp16", "clamp", 3.0),
                                 ((131, 131, 2), "fp16", "clamp", 1.0), ((35, 35, 4), "fp16", "mirror", 0.2))]


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


def bits(a):
    """fp32 bit patterns: -0 != +0, and a NaN equals itself"""
    return np.ascontiguousarray(a, f32).view(np.uint32)


def half_bits(a):
    """bit patterns of the binary16 values a field holds (what a download of fp16 storage returns is exactly representable)"""
    h = np.asarray(a, f32).astype(np.float16)
    assert np.array_equal(bits(h.astype(f32)), bits(a))
    return h.view(np.uint16)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.sqrt((b ** 2).sum())
    d = np.sqrt(((a - b) ** 2).sum())
    return d / n if n > 0 else d


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)                              # shared among tests: nobody changes a reference
    return arrays


def storable(a, half):
    return a.astype(np.float16).astype(f32) if half else a


@functools.lru_cache(maxsize=None)
def state(dims, storage, scale=0.5):
    X, Y, Z = dims
    rng = np.random.default_rng(1200 + X + 7 * Z + int(scale * 10))
    half = storage == "fp16"
    vel = storable((rng.standard_normal((3, Z, Y, X)) * scale).astype(f32), half)
    col = storable(rng.random((Z, Y, X, 4)).astype(f32), half)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    return frozen(vel, col, p)


def far_from_the_impulse(dims):
    """outside the impulse ball there is no transcendental on the advection's path (the mask of test_gpu_sim.py::test_advect_matches_oracle)"""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return ((x + .5) / X - .5) ** 2 + ((y + .5) / Y - .1) ** 2 + ((z + .5) / Z - .5) ** 2 > (1.5 / 16) ** 2


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(320, 240, dims, **kw), f.last_status
    return f


def where(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    return len(bad), bad[:6].tolist()


# ---- divergence / projection / advection on every shape x storage ------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_divergence_bit_exact(dims, storage):
    vel, _, _ = state(dims, storage)
    f = make(dims, storage=storage)
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.UpdateFrame(f32(f.default_time_step()), 0)
    f.Divergence()
    got, want = f.download(fx.FIELD_DIVERGENCE), orc.divergence(vel)
    assert np.array_equal(bits(got), bits(want)), where(got, want)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_projection_bit_exact(dims, storage):
    vel, _, p = state(dims, storage)
    f = make(dims, storage=storage)
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.upload(fx.FIELD_PRESSURE, p)
    f.UpdateFrame(f32(f.default_time_step()), 0)
    f.Project()
    got, want = f.download(fx.FIELD_VELOCITY), orc.project(vel, p, half=storage == "fp16")
    assert np.array_equal(bits(got), bits(want)), where(got, want)


def advect(dims, storage, address, vel, col):
    f = make(dims, storage=storage, advect_address=address)
    dt = f32(f.default_time_step())
    f.upload(fx.FIELD_VELOCITY, vel)
    f.upload(fx.FIELD_COLOR, col)                            # parity 0 -> UpdateFrame flips: the advection reads this one
    f.UpdateFrame(dt, 0)
    f.Advect()
    f.Synchronize()
    vo, co = orc.advect(vel, col, dt, address=int(address == "mirror"), half=storage == "fp16")
    return f.download(fx.FIELD_VELOCITY1), f.download(fx.FIELD_COLOR), vo, co


@pytest.mark.parametrize("scale", [1.5, 12.0])               # 12: taps across every border and through the mirror's second period
@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_advection_matches_oracle(dims, storage, address, scale):
    vel, col, _ = state(dims, storage, scale)
    gv, gc, vo, co = advect(dims, storage, address, vel, col)
    far = far_from_the_impulse(dims)
    assert far.any()
    assert np.array_equal(bits(gv[:, far]), bits(vo[:, far])), where(gv * far, vo * far)
    assert np.array_equal(bits(gc[far]), bits(co[far]))
    ev, ec = rel_l2(gv, vo), rel_l2(gc, co)
    print("advect %s %s %s %g: rel-L2 velocity %.3g colour %.3g" % (dims, storage, address, scale, ev, ec))
    bar = 1e-4 if storage == "fp16" else 1e-6
    assert ev < bar and ec < bar, (ev, ec)


# ---- two whole steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "%s-%s-%s" % (ids(c["dims"]), c["storage"], c["mode"]))
def test_two_steps_match_oracle(case):
    import test_gpu_fuzz as fuzz
    X, _, Z = case["dims"]
    fuzz.check_random_step(dict(case, fuse=0, rng=np.random.default_rng(2300 + X + Z)))


# ---- binary16: subnormals, the overflow boundary, -0 -------------------------------------------------------------------------
HALF_SHAPES = [d for d in SHAPES if d[0] >= 35]


def log_uniform(rng, shape, lo, hi):
    return (np.exp2(rng.uniform(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)).astype(f32)


@functools.lru_cache(maxsize=None)
def half_range_state(dims):
    """velocity magnitudes log-uniform in 2^-27 .. 2^16 (clipped to the largest binary16), pressure in 2^-30 .. 2^15, random signs; a
    lattice of +0 cells and, on the odd planes of component 0, of -0 cells; colour random() ** 8"""
    X, Y, Z = dims
    rng = np.random.default_rng(3400 + X + Z)
    vel = np.clip(log_uniform(rng, (3, Z, Y, X), -27, 16), -65504, 65504).astype(np.float16).astype(f32)
    vel[:, ::2, ::3, ::5] = 0.0
    vel[0, 1::2, ::3, ::5] = -0.0
    p = log_uniform(rng, (Z, Y, X), -30, 15)
    col = (rng.random((Z, Y, X, 4)) ** 8).astype(np.float16).astype(f32)
    return frozen(vel, col, p)


def half_classes(h):
    """fractions of a field of binary16 bit patterns: subnormal (non-zero), +-inf, -0, NaN"""
    e, m = h & 0x7C00, h & 0x03FF
    return ((e == 0) & (m != 0)).mean(), ((e == 0x7C00) & (m == 0)).mean(), (h == 0x8000).mean(), ((e == 0x7C00) & (m != 0)).mean()


def assert_the_edges_are_reached(h, what, overflow=True):
    """conditions on the ORACLE's output (if a state misses them its recipe is wrong, not these bounds): the comparison that follows
    sees stores into the subnormal range, across the overflow boundary and of -0, and no NaN whose payload nobody specifies"""
    sub, inf, negzero, nan = half_classes(h)
    print("%s: subnormal %.4f inf %.5f -0 %.5f NaN %g" % (what, sub, inf, negzero, nan))
    assert sub >= 0.02 and negzero >= 2e-4 and nan == 0, (what, sub, inf, negzero, nan)
    assert inf >= 2e-4 if overflow else inf == 0, (what, inf)


@pytest.mark.parametrize("dims", HALF_SHAPES, ids=ids)
def test_fp16_projection_stores_every_binary16_range(dims):
    vel, _, p = half_range_state(dims)
    want = half_bits(orc.project(vel, p, half=True))
    assert_the_edges_are_reached(want, "project %s" % (dims,))
    f = make(dims, storage="fp16")
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.upload(fx.FIELD_PRESSURE, p)
    assert np.array_equal(half_bits(f.download(fx.FIELD_VELOCITY1)), half_bits(vel))       # the upload kept -0 and the subnormals
    f.UpdateFrame(f32(f.default_time_step()), 0)
    f.Project()
    got = half_bits(f.download(fx.FIELD_VELOCITY))
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:6].tolist())


@pytest.mark.parametrize("address", ["clamp", "mirror"])
@pytest.mark.parametrize("dims", HALF_SHAPES, ids=ids)
def test_fp16_advection_stores_every_binary16_range(dims, address):
    """the same state through the advection, outside the impulse ball: subnormal stores and -0 (a negative result below 2^-25) as bit
    patterns.  No store can overflow here -- a stored value is a convex combination of storable taps times 1 - 0.2 dt < 1 -- and an inf
    among the inputs would make the filter's inf - inf a NaN, so the overflow boundary is the projection test's alone"""
    vel, col, _ = half_range_state(dims)
    gv, gc, vo, co = advect(dims, "fp16", address, vel, col)
    far = far_from_the_impulse(dims)
    want = np.concatenate([half_bits(vo[:, far]).ravel(), half_bits(co[far]).ravel()])
    assert_the_edges_are_reached(want, "advect %s %s" % (dims, address), overflow=False)
    got = np.concatenate([half_bits(gv[:, far]).ravel(), half_bits(gc[far]).ravel()])
    assert np.array_equal(got, want), (int((got != want).sum()), np.flatnonzero(got != want)[:6].tolist())


# ---- fp32 subnormals: divergence, Jacobi and projection keep them, like the oracle ----------------------------------------------------
# (geometry, Jacobi mode, sweeps, the launches of the default schedule as tests/golden/jacobi_plan.json writes them -- tests/test_stage_matrix.py
# asks the planner for the same): the matrix shapes run k_jacobi_blockg or single sweeps; below them one geometry per shipped Jacobi family --
# single sweeps at 64 cells (the strip twos of that width answer a jacobi_fuse request only), block2, blockg, the octet's fours with a strip
# three, rows of 264 cells below and from the depth where the x tiles of the octet take them, 512 cells as three such tiles, a strip two
# behind a three, the 2-D tiles, and the sparse solver of the faithful mode
ONES, BLOCKG = "7*sweep1:1", "3*blockg:2 sweep1:1"
SUBNORMAL_CASES = [(d, "fixed", 7, BLOCKG if d in ((10, 10, 3), (70, 70, 5), (9, 9, 3), (150, 150, 3), (35, 35, 4), (36, 36, 6)) else ONES) for d in SHAPES] + [
    ((64, 64, 8), "fixed", 7, ONES), ((128, 128, 8), "fixed", 7, "3*block2:2 sweep1:1"), ((150, 150, 6), "fixed", 7, BLOCKG),
    ((256, 256, 8), "fixed", 7, "strip4:4 strip3:3"), ((264, 264, 8), "fixed", 7, ONES), ((264, 264, 16), "fixed", 7, "strip4:4 3*sweep1:1"),
    ((512, 512, 8), "fixed", 7, "strip4:4 strip3:3"), ((256, 256, 8), "fixed", 5, "strip3:3 strip:2"), ((64, 64, 1), "fixed", 7, "tile2d:7"),
    ((64, 64, 8), "faithful", 6, None)]


def launches_of(plan):
    """'3*blockg:2 sweep1:1' -> 4"""
    return sum(int(item.rpartition("*")[0] or 1) for item in plan.split())


def subnormal_share(a):
    a = np.abs(np.asarray(a, f32))
    return float(((a > 0) & (a < np.finfo(f32).tiny)).mean())


@pytest.mark.parametrize("dims,mode,sweeps,plan", SUBNORMAL_CASES, ids=[("%s-%s-%d" % (ids(c[0]), c[1], c[2])) for c in SUBNORMAL_CASES])
def test_fp32_subnormal_fields_bit_exact(dims, mode, sweeps, plan):
    X, Y, Z = dims
    rng = np.random.default_rng(4500 + X + Z)
    tiny = 2.0 ** -128                                       # standard_normal * 2^-128: below the smallest normal (2^-126) up to four sigma
    vel = (rng.standard_normal((3, Z, Y, X)) * tiny).astype(f32)
    p = (rng.standard_normal((Z, Y, X)) * tiny).astype(f32)
    if Z == 1:
        vel[2] = 0
    b = orc.divergence(vel)
    q, k = orc.jacobi(p, b, sweeps, mode=int(mode == "faithful"))
    w = orc.project(vel, q)
    shares = [subnormal_share(a) for a in (b, q, w[:2] if Z == 1 else w)]
    print("subnormal and non-zero: divergence %.4f pressure %.4f velocity %.4f" % tuple(shares))
    assert min(shares) > 0.99, shares                        # a condition on the oracle's output, not a measurement of the kernels

    f = make(dims, jacobi_iters=sweeps, jacobi_mode=mode)
    f.upload(fx.FIELD_VELOCITY1, vel)
    f.upload(fx.FIELD_PRESSURE, p)
    f.UpdateFrame(f32(f.default_time_step()), 0)
    f.Divergence()
    got = f.download(fx.FIELD_DIVERGENCE)
    assert np.array_equal(bits(got), bits(b)), ("divergence",) + where(got, b)
    f.timing_enable(True); f.timing_read(True)
    f.Jacobi(sweeps)
    f.Synchronize()
    t = f.timing_read(True)
    if mode == "faithful":
        assert (t.freeze_solves, t.freeze_sweeps) == (1, k)
    else:
        assert t.jacobi_sweeps == sweeps and k == sweeps
        assert t.jacobi_launches == launches_of(plan), (t.jacobi_launches, plan)
    got = f.download(fx.FIELD_PRESSURE)
    assert np.array_equal(bits(got), bits(q)), ("jacobi",) + where(got, q)
    f.Project()
    got = f.download(fx.FIELD_VELOCITY)
    assert np.array_equal(bits(got), bits(w)), ("project",) + where(got, w)


# ---- the new row classes in z-slabs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["shared", "peer"])
@pytest.mark.parametrize("dims,storage,nranks", [((70, 70, 24), "fp16", 2), ((35, 35, 24), "fp32", 3), ((35, 35, 24), "fp16", 3), ((201, 201, 18), "fp16", 2)],
                         ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_slabs_of_the_row_classes_equal_the_single_domain(dims, storage, nranks, group, monkeypatch):
    """pairs in fp16 rows of 70 cells, the scalar kernels (rows of 35 cells, both storages; 201 in fp16) on slab geometries: three steps ==
    the single domain bit for bit.  Halos as test_gpu_fuzz.draw_slabs sizes them: every slab at least max(halo_advect, halo_jacobi) planes"""
    import test_gpu_slabs as slabs
    from fluidx12_amd import fluid as fluid_mod
    monkeypatch.setattr(fluid_mod, "default_local_group", group)
    ha, hj = 6, 4
    assert dims[2] // nranks >= max(ha, hj)
    kw = dict(jacobi_iters=9, storage=storage)
    ref = slabs.run_single(dims, 3, **kw)
    fl = slabs.run_slabs(dims, 3, nranks, halo_advect=ha, halo_jacobi=hj, **kw)
    for field, axis in ((fx.FIELD_VELOCITY, 1), (fx.FIELD_COLOR, 0), (fx.FIELD_PRESSURE, 0)):
        got, want = slabs.gather(fl, field, axis), ref.download(field)
        assert want.any()
        assert np.array_equal(bits(got), bits(want)), (field,) + where(got, want)


# ---- fx_field_digest's range ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [None, (8, 8)])
def test_digest_refuses_ranges_that_wrap(slab):
    """through the C ABI: a z_count whose 32-bit sum with z_begin wraps (5 + 0xFFFFFFFF), one plane too many, the plane behind the last:
    FX_E_INVALID, `out` untouched (fx::digest_range_ok, checked on the host in tests/test_stage_matrix.py)"""
    dims = (16, 16, 24)
    kw = dict(slab=slab, halo_advect=6, halo_jacobi=2) if slab else {}
    f = make(dims, **kw)
    z0, nz = slab or (0, dims[2])
    lib = capi.load()
    mark = 0x5A5A5A5A5A5A5A5A
    for a, n in ((5, 0xFFFFFFFF), (z0 + 5, 0xFFFFFFFF), (0, nz + 1), (z0, nz + 1), (z0 + nz, 1), (z0 + nz, 0xFFFFFFFF - nz + 1), (0xFFFFFFFF, 2)):
        out = (C.c_uint64 * 2)(mark, mark)
        assert lib.fx_field_digest(f._ctx, fx.FIELD_PRESSURE, a, n, out) == capi.FX_E_INVALID, (a, n)
        assert (out[0], out[1]) == (mark, mark)
    whole = f.digest(fx.FIELD_PRESSURE)
    assert f.digest(fx.FIELD_PRESSURE, z0, nz) == whole
    parts = f.digest(fx.FIELD_PRESSURE, z0, 1), f.digest(fx.FIELD_PRESSURE, z0 + 1, nz - 1)
    lo = (parts[0] + parts[1]) & ((1 << 64) - 1)              # the digest's two words are wrapping sums over the cells
    hi = ((parts[0] >> 64) + (parts[1] >> 64)) & ((1 << 64) - 1)
    assert ((hi << 64) | lo) == whole
    with pytest.raises(ValueError):
        f.digest(fx.FIELD_PRESSURE, -1, 1)
    with pytest.raises(ValueError):
        f.digest(fx.FIELD_PRESSURE, 0, 1 << 32)
