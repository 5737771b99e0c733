"""The particle sort on the GPU (fx_set_particle_sort / fx_sort_particles ..., csrc/fx_particle_sort.hip) against the numpy model
tests/particle_sort_ref.py: the sorted buffer, order and live, everything compared as uint32 bits.

Shapes: particle_ref.SHAPES -- keys of 11 to 19 bits, two and three passes -- and (3, 3, 2), one pass of 5 bits (it stands in for (5, 3, 2), which
no context can hold: fx_create takes X == Y only; the model and the planner are tested on (5, 3, 2) itself).  Counts: 1, 2, 255, 256, 257, 4099, 65 537,
2^18 + 1, and what the planner says its own edges are: one below, at and one above the records of a workgroup, and the first count whose histogram
takes a second scan block; on (70, 70, 5) also the last count whose block sums are scanned in one round and one that needs a second (a little
over two million records).  The sort reads no field, so both storages are run on one shape only."""
import ctypes as C
import functools

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import particle_ref as pr
import particle_sort_ref as ps

pytestmark = pytest.mark.gpu
f32 = np.float32
SHAPES = ps.GPU_SHAPES
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
DRIFT = (0.03, -0.4, 0.02)


def make(dims, **kw):
    f = fx.Fluid()
    assert f.Init(0, 0, dims, **kw), f.last_status
    return f


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(ps.bits(a), ps.bits(b))


def counts_of(dims):
    return sorted(set(ps.COUNTS + ps.threshold_counts(dims)))


def sort_and_check(f, rec, dims, tag):
    """SetParticles(rec), SortParticles(), and the three results against the model; -> the model's (sorted, order, live)"""
    f.SetParticles(rec)
    ptr = f.ParticlesDevice()
    f.SortParticles()
    want, order, live = ps.sort(rec, dims)
    got = f.GetParticles()
    assert same_bits(got, want), tag
    assert np.array_equal(f.ParticleOrder(), order), tag
    assert f.ParticleSortInfo() == (live, 1), tag
    assert f.ParticlesDevice() == ptr, tag
    return want, order, live


# ---- 1: arrangements against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,storage", [(d, "fp32") for d in SHAPES] + [((20, 20, 12), "fp16")])
def test_every_arrangement_sorts_as_the_model_does(dims, storage):
    f = make(dims, storage=storage)
    f.SetParticleSort(True)
    for n in counts_of(dims):
        rec = ps.arrangement("random", dims, n, seed=n % 97)
        _, _, live = sort_and_check(f, rec, dims, ("random", n))
        assert n < 5 or 0 < live < n
    big = 65537                                                            # stability across workgroups decides every position
    for name in ps.ARRANGEMENTS[1:]:
        for n in (big, 257) if name in ("one_cell", "two_cells", "live_dead", "all_dead") else (4099,):
            rec = ps.arrangement(name, dims, n, seed=3)
            _, order, live = sort_and_check(f, rec, dims, (name, n))
            if name == "all_dead":
                assert live == 0 and np.array_equal(order, np.arange(n, dtype=np.uint32))
            if name in ("all_live", "one_cell", "two_cells", "edges"):
                assert live == n
            if name in ("one_cell", "sorted"):
                assert np.array_equal(order, np.arange(n, dtype=np.uint32))
    f.Release()


@pytest.mark.parametrize("name", ["random", "two_cells", "live_dead"])
@pytest.mark.parametrize("which", [0, 1], ids=["last_single_round", "second_round"])
def test_the_scan_of_the_block_sums_carries_into_a_second_round(which, name):
    """(70, 70, 5): digits of 8 + 7 bits.  The largest count whose 8-bit pass has 256 scan blocks, one round of k_psort_scan_sums, and a count
    with 260: the running total crosses into a second round that holds more than one entry (tests/test_particle_sort_ref.py holds the planner
    to both figures).  A little over two million records each."""
    dims = (70, 70, 5)
    n = ps.scan_round_counts(dims)[which]
    f = make(dims)
    f.SetParticleSort(True)
    _, order, live = sort_and_check(f, ps.arrangement(name, dims, n, seed=31), dims, (name, n))
    assert 0 < live <= n and not np.array_equal(order, np.arange(n, dtype=np.uint32))
    f.Release()


# ---- 2: a second sort is the identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES)
def test_a_second_sort_is_the_identity(dims):
    f = make(dims)
    f.SetParticleSort(True)
    for n in (257, 65537):
        rec = ps.arrangement("random", dims, n, seed=11)
        want, _, live = sort_and_check(f, rec, dims, n)
        f.SortParticles()
        assert same_bits(f.GetParticles(), want) and np.array_equal(f.ParticleOrder(), np.arange(n, dtype=np.uint32))
        assert f.ParticleSortInfo() == (live, 2)
    f.Release()


# ---- 3: the pointer survives ----------------------------------------------------------------------------------------------------------------
def test_the_pointer_survives_and_serves_the_point_query():
    import torch
    dims, n = (20, 20, 12), 4099
    vel = pr.velocity(dims, 601)
    f = make(dims)
    f.upload(fx.FIELD_VELOCITY, vel)
    f.SetParticleSort(True)
    rec = ps.arrangement("random", dims, n, seed=5)
    f.SetParticles(rec)
    ptr, count = f.ParticlesDevice()
    f.SortParticles()
    assert f.ParticlesDevice() == (ptr, count) and ptr % 16 == 0 and count == n
    order_ptr, live_ptr = f.ParticleOrderDevice()
    assert order_ptr and live_ptr and order_ptr % 4 == 0 and live_ptr % 4 == 0
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fp = C.POINTER(C.c_float)
    capi.check(capi.load().fx_sample_velocity(f._ctx, None, C.cast(ptr, fp), n, C.cast(out.data_ptr(), fp), capi.PARTICLES_DEVICE), "device query")
    f.Synchronize()
    torch.cuda.synchronize()
    want = ps.sort(rec, dims)[0]
    assert same_bits(out.cpu().numpy(), pr.sample(vel, want))                # the query sees the sorted set
    f.Release()


# ---- 4: passive -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["euler", "midpoint"])
def test_sort_then_move_is_the_models_move_permuted_and_no_field_changes(scheme):
    dims, n = (20, 20, 12), 4099
    dt = pr.time_step(dims)
    vel = pr.velocity(dims, 601, cells=1.5)
    col = np.random.default_rng(653).random((dims[2], dims[1], dims[0], 4)).astype(f32)
    solid, faces, lifetime = pr.box_mask(dims), pr.X_HI | pr.Y_LO, 0.5 + float(dt)
    f = make(dims)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.UpdateFrame(dt, 0)
    f.SetObstacles(solid)
    f.SetOpenWalls(faces)
    f.SetParticleParams(scheme, DRIFT, lifetime)
    f.SetParticleSort(True)
    prm = pr.params(scheme=pr.MIDPOINT if scheme == "midpoint" else pr.EULER, drift=DRIFT, lifetime=lifetime)
    rec = ps.arrangement("random", dims, n, seed=7)
    f.SetParticles(rec)
    before = [f.digest(k) for k in ALL_FIELDS]
    f.SortParticles()
    assert before == [f.digest(k) for k in ALL_FIELDS]
    order = f.ParticleOrder()
    assert np.array_equal(order, ps.sort(rec, dims)[1])
    f.MoveParticles()
    moved = pr.move(rec, vel, dt, prm, faces, solid)
    assert same_bits(f.GetParticles(), moved[order])
    free = pr.move(rec, vel, dt, prm)
    assert not same_bits(moved[:, :3], free[:, :3]) and not same_bits(moved[:, 3], free[:, 3])     # the solid and the open walls both took part
    assert before == [f.digest(k) for k in ALL_FIELDS]
    f.Release()


# ---- 5: in the step -------------------------------------------------------------------------------------------------------------------------
ITERS = 8


def stepped(dims, every, steps=4):
    """`steps` fx_simulate steps with a set; every = None: sorting off, 0: enabled but never in the step, n: every nth run -> (the particles,
    the device's velocity behind each step, (live, sorts) or None)"""
    vel = pr.velocity(dims, 651, cells=0.6)
    col = np.random.default_rng(653).random((dims[2], dims[1], dims[0], 4)).astype(f32)
    f = make(dims, jacobi_iters=ITERS)
    f.upload(fx.FIELD_VELOCITY, vel); f.upload(fx.FIELD_COLOR, col)
    f.SetObstacles(pr.box_mask(dims))
    f.SetOpenWalls(pr.Y_HI | pr.X_LO)
    if every is not None:
        f.SetParticleSort(True, every)
    f.SetParticles(ps.arrangement("random", dims, 4099, seed=13))
    f.SetParticleParams("midpoint", DRIFT, 0.7)
    dt = pr.time_step(dims)
    vels = []
    for i in range(steps):
        f.UpdateFrame(dt, i % 3)
        f.Simulate(i % 3)
        f.Synchronize()
        vels.append(f.download(fx.FIELD_VELOCITY))
    info = f.ParticleSortInfo() if every is not None else None
    order = f.ParticleOrder() if every else None
    part = f.GetParticles()
    f.Release()
    return part, vels, info, order


@pytest.mark.parametrize("dims", [(36, 36, 1), (20, 20, 12)])
def test_the_step_sorts_every_nth_run(dims):
    dt = pr.time_step(dims)
    prm = pr.params(scheme=pr.MIDPOINT, drift=DRIFT, lifetime=0.7)
    solid, faces = pr.box_mask(dims), pr.Y_HI | pr.X_LO
    rec0 = ps.arrangement("random", dims, 4099, seed=13)
    part, vels, info, order = stepped(dims, 2)
    want, last = rec0, None
    for i, v in enumerate(vels):                                             # the model's sort (runs 1 and 3) and move against the device's own velocity
        if i % 2 == 0:
            want, last, live = ps.sort(want, dims)
        want = pr.move(want, v, dt, prm, faces, solid)
    assert same_bits(part, want) and info == (live, 2) and np.array_equal(order, last)
    # every = 0 and sorting off: the step never sorts, the buffer is the move-only one
    plain = rec0
    for v in vels:
        plain = pr.move(plain, v, dt, prm, faces, solid)
    part0, vels0, info0, _ = stepped(dims, 0)
    assert same_bits(part0, plain) and info0 == (0, 0)
    partn, velsn, _, _ = stepped(dims, None)
    assert same_bits(partn, plain)
    for a, b, c in zip(vels, vels0, velsn):                                  # ... and the fields never know
        assert same_bits(a, b) and same_bits(a, c)
    assert not same_bits(part, plain)


# ---- 6: forced key width --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(20, 20, 12), (36, 36, 1)])
def test_passes_over_empty_high_digits_keep_the_order(dims, knob):
    """PSORT_KEY_BITS = 32 (a lab switch: the context runs on the lab build) plans four passes of eight bits on any grid: the passes over the
    all-zero high digits of a real grid's keys are executed here, not merely compiled"""
    knob("PSORT_KEY_BITS", "32")
    f = make(dims)
    f.SetParticleSort(True)
    for n in (4099, 65537):
        sort_and_check(f, ps.arrangement("random", dims, n, seed=17), dims, n)
    sort_and_check(f, ps.arrangement("one_cell", dims, 65537, seed=17), dims, "one_cell")
    f.Release()


# ---- 7: fx_set_particles while enabled ------------------------------------------------------------------------------------------------------
def test_set_particles_resizes_the_scratch():
    dims = (70, 70, 5)
    f = make(dims)
    f.SetParticleSort(True)
    assert f.ParticleSortInfo() == (0, 0)
    f.SortParticles()                                                        # no set: FX_OK and nothing done
    assert f.ParticleSortInfo() == (0, 0) and f.ParticleOrder().shape == (0,)
    for n in (257, 65537, 4099, 1):
        rec = ps.arrangement("random", dims, n, seed=19)
        sort_and_check(f, rec, dims, n)                                      # (sorts == 1 each time: the count starts again with the set)
        f.SortParticles()
        assert f.ParticleSortInfo()[1] == 2
    f.SetParticles(None)
    assert f.ParticleSortInfo()[1] == 0 and f.ParticlesDevice() == (0, 0)
    f.SortParticles()
    assert f.ParticleSortInfo()[1] == 0 and f.ParticleOrderDevice()[0] == 0 and f.ParticleOrderDevice()[1] != 0
    sort_and_check(f, ps.arrangement("live_dead", dims, 300, seed=19), dims, "again")
    f.Release()


# ---- 8: status codes and round trips --------------------------------------------------------------------------------------------------------
def test_status_codes_and_round_trips():
    lib = capi.load()
    dims = (20, 20, 12)
    f = make(dims)
    off = dict(enabled=False, every=0, flags=0)
    a, b = C.c_void_p(5), C.c_void_p(6)
    info = capi.ParticleSortInfo(16, 77, 78, 79)
    # the default: off -- the stage and the arrays are FX_E_STATE, the getters report it
    assert f.GetParticleSort() == off and f.ParticleSortInfo() == (0, 0)
    assert lib.fx_sort_particles(f._ctx, None) == capi.FX_E_STATE
    assert lib.fx_particle_order_device(f._ctx, C.byref(a), C.byref(b)) == capi.FX_E_STATE and (a.value, b.value) == (5, 6)
    rec = ps.arrangement("random", dims, 257, seed=23)
    f.SetParticles(rec)
    assert lib.fx_sort_particles(f._ctx, None) == capi.FX_E_STATE and same_bits(f.GetParticles(), rec)
    # round trips
    f.SetParticleSort(True, 3)
    mine = dict(enabled=True, every=3, flags=0)
    assert f.GetParticleSort() == mine
    f.SortParticles()
    want, order, live = ps.sort(rec, dims)
    assert same_bits(f.GetParticles(), want) and f.ParticleSortInfo() == (live, 1)
    # refused, the previous state staying in force
    for change in (dict(struct_size=12), dict(struct_size=20), dict(flags=1), dict(flags=0x80000000), dict(enabled=2), dict(enabled=0, every=1)):
        q = capi.ParticleSort(16, 0, 1, 0)
        for k, v in change.items():
            setattr(q, k, v)
        assert lib.fx_set_particle_sort(f._ctx, C.byref(q)) == capi.FX_E_INVALID and f.GetParticleSort() == mine, change
    assert f.ParticleSortInfo() == (live, 1)
    assert lib.fx_get_particle_sort(f._ctx, None) == capi.FX_E_INVALID and lib.fx_particle_sort_info(f._ctx, None, None) == capi.FX_E_INVALID
    assert lib.fx_particle_order_device(f._ctx, None, C.byref(b)) == capi.FX_E_INVALID and lib.fx_particle_order_device(f._ctx, C.byref(a), None) == capi.FX_E_INVALID
    assert (a.value, b.value) == (5, 6)
    # configuration on the particles' terms: kept across UpdateFrame, not digested
    f.UpdateFrame(f32(0.0), 1)
    f.Simulate(1)                                                            # dt = 0: the stage does not run, so nothing sorts
    before = [f.digest(k) for k in ALL_FIELDS]
    assert f.GetParticleSort() == mine and f.ParticleSortInfo() == (live, 1) and same_bits(f.GetParticles(), want)
    f.SetParticleSort(True, 0)
    assert f.ParticleSortInfo()[1] == 0 and f.GetParticleSort() == dict(enabled=True, every=0, flags=0)
    # disabling frees the scratch and returns the stage to FX_E_STATE; NULL is the default
    f.SetParticleSort(False)
    assert f.GetParticleSort() == off and lib.fx_sort_particles(f._ctx, None) == capi.FX_E_STATE
    assert lib.fx_particle_order_device(f._ctx, C.byref(a), C.byref(b)) == capi.FX_E_STATE and f.ParticleSortInfo() == (0, 0)
    f.SetParticleSort(True, 1)
    f.SetParticleSort(None)
    assert f.GetParticleSort() == off and lib.fx_sort_particles(f._ctx, None) == capi.FX_E_STATE
    assert same_bits(f.GetParticles(), want) and before == [f.digest(k) for k in ALL_FIELDS]
    # slab ranks: the setters and the stage refuse, the getters report the default
    ranks = []
    for z0, nz in ((0, 12), (12, 20)):
        r = fx.Fluid()
        assert r.Init(0, 0, (32, 32, 32), slab=(z0, nz), halo_advect=6, halo_jacobi=2)
        ranks.append(r)
    for r in ranks:
        q = capi.ParticleSort(16, 0, 1, 0)
        assert lib.fx_set_particle_sort(r._ctx, C.byref(q)) == capi.FX_E_INVALID and lib.fx_set_particle_sort(r._ctx, None) == capi.FX_E_INVALID
        assert lib.fx_sort_particles(r._ctx, None) == capi.FX_E_INVALID
        assert lib.fx_particle_order_device(r._ctx, C.byref(a), C.byref(b)) == capi.FX_E_INVALID
        assert r.GetParticleSort() == off and r.ParticleSortInfo() == (0, 0)
    # a render-only context: FX_E_STATE, whatever else is wrong with the call
    ro = fx.Fluid()
    assert ro.Init(64, 64, (32, 32, 8), render_only=True)
    q = capi.ParticleSort(16, 0, 1, 0)
    assert lib.fx_set_particle_sort(ro._ctx, C.byref(q)) == capi.FX_E_STATE and lib.fx_get_particle_sort(ro._ctx, C.byref(q)) == capi.FX_E_STATE
    assert lib.fx_sort_particles(ro._ctx, None) == capi.FX_E_STATE and lib.fx_particle_sort_info(ro._ctx, None, C.byref(info)) == capi.FX_E_STATE
    assert lib.fx_particle_order_device(ro._ctx, C.byref(a), C.byref(b)) == capi.FX_E_STATE and (info.live, info.sorts) == (77, 78)
    # Release() with scratch allocated is clean
    g = make(dims)
    g.SetParticleSort(True, 2)
    g.SetParticles(rec)
    g.SortParticles()
    for o in [f, ro, g] + ranks:
        o.Release()
