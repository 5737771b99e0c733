"""The numpy model of the particle spawners (tests/particle_spawn_ref.py) held to the known answers of the rule (include/fluidx_hip.h,
fx_set_particle_spawners), to the properties a caller relies on -- uniform draws, a ball that stays inside its ellipsoid, a rate that is kept
exactly, serials that do not depend on the pool -- and the built library held to the four new symbols.  No GPU."""
import ctypes as C

import numpy as np

import particle_spawn_ref as sr

f32, u64 = np.float32, np.uint64
DIMS = (16, 12, 8)


# ---- 1: known answers and uniformity ---------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_hash():
    assert [int(v) for v in sr.mix([0, 1, 2, 0xffffffff, 0x12345678])] == [0x0, 0x688990c0, 0xd1132181, 0x6768824a, 0xf5e71c96]
    assert [int(v) for v in sr.word(0, 0, [0, 1, 2, 2 ** 32 + 5], 0)] == [0x9c35e727, 0x6a392e23, 0x21cf48f2, 0x35c715c0]
    assert int(sr.word(7, 3, 41, 24)[0]) == 0x7bba45dd
    # u and a are exact: 24 bits, in [0, 1) and [-1, 1)
    k = np.arange(4096, dtype=u64)
    u, a = sr.unit(5, 2, k, 0), sr.sym(5, 2, k, 0)
    assert u.dtype == f32 and (u >= 0).all() and (u < 1).all() and (a >= -1).all() and (a < 1).all()
    assert np.array_equal(u.astype(np.float64) * 2 ** 24, (sr.word(5, 2, k, 0) >> np.uint32(8)).astype(np.float64))
    assert np.array_equal(a.astype(np.float64), 2 * u.astype(np.float64) - 1)


def test_the_box_draw_is_uniform():
    k = np.arange(4096, dtype=u64)
    worst_mean, lo, hi = 0.0, 4096, 0
    for seed in (0, 1, 12345):
        for s in (0, 15):
            a, fell = sr.draw(sr.spawner(seed=seed), s, k)
            assert not fell.any()
            worst_mean = max(worst_mean, float(np.abs(a.astype(np.float64).mean(axis=0)).max()))
            octant = (a[:, 0] >= 0) * 1 + (a[:, 1] >= 0) * 2 + (a[:, 2] >= 0) * 4
            n = np.bincount(octant, minlength=8)
            lo, hi = min(lo, int(n.min())), max(hi, int(n.max()))
    print("box draw: |mean| up to %.4f, octants %d - %d" % (worst_mean, lo, hi))
    assert worst_mean < 0.05 and 420 <= lo and hi <= 600


# ---- 2: the ball -----------------------------------------------------------------------------------------------------------------------------
def test_the_ball_stays_inside_its_ellipsoid():
    k = np.arange(1 << 16, dtype=u64)
    sp = sr.spawner(shape=sr.BALL, seed=3, center=(0.5, 0.4, 0.6), half_extent=(0.3, 0.2, 0.1))
    a, fell = sr.draw(sp, 1, k)
    share = float(fell.mean())
    print("ball: fallback share %.4f" % share)
    assert share < 0.01 and not a[fell].any()
    assert (np.asarray(sr.fma(a[:, 2], a[:, 2], sr.fma(a[:, 1], a[:, 1], (a[:, 0] * a[:, 0]).astype(f32))), f32) <= 1).all()
    rec = sr.records_of(sp, 1, k)
    q = (rec[:, :3].astype(np.float64) - np.array(sp["center"], f32).astype(np.float64)) / np.array(sp["half_extent"], f32).astype(np.float64)
    # up to the final rounding: the offsets' own sum of squares is rounded three times, the scaled position once, relative 2^-24 each
    assert ((q * q).sum(axis=1) <= 1 + 1e-5).all()
    assert (rec[:, 3] == 0).all()                                          # age_spread 0: every record is born with age +0
    # a 2-D grid does not draw z: the record sits on the centre's plane, and the test runs on x and y alone
    a2, _ = sr.draw(sp, 1, k, is3d=False)
    assert not a2[:, 2].any() and (a2[:, 0].astype(np.float64) ** 2 + a2[:, 1].astype(np.float64) ** 2 <= 1 + 1e-6).all()
    assert float((a2 != a).any(axis=1).mean()) > 0.2                       # more first tries pass than in 3-D


# ---- 3: the accumulator ----------------------------------------------------------------------------------------------------------------------
def test_a_quarter_birth_per_step_bears_one_record_every_fourth_step():
    sp = [sr.spawner(rate=16.0)]
    dt = f32(1.0 / 64)                                                     # rate * dt = 0.25 exactly
    st = sr.new_state(1)
    rec = np.zeros((64, 4), f32)
    rec[:, 3] = -1
    born = []
    for _ in range(12):
        rec = sr.step(rec, sp, st, dt, DIMS)
        born.append(st["born"])
    assert born == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3]
    assert st["serial"] == [3] and st["acc"] == [0] and st["dropped"] == 0
    # the cap: 2^26 births per step at the most, however large rate * dt
    n, acc = sr.births(sr.spawner(rate=3e38), 0, f32(3e38))
    assert n == 1 << 26 and acc == 0
    # a rate that is no multiple of 2^-16 per step is kept to 2^-17 per step
    n, acc = sr.births(sr.spawner(rate=1.0), 0, f32(1.0 / 3))
    assert n == 0 and abs(acc / 65536 - 1 / 3) <= 2.0 ** -17


# ---- 4: serials, dropping, blocking ----------------------------------------------------------------------------------------------------------
def pool(n, dead):
    rng = np.random.default_rng(n)
    rec = rng.random((n, 4)).astype(f32)
    rec[dead, 3] = -1
    return rec


def test_serials_advance_when_births_are_dropped():
    sp = [sr.spawner(rate=5.0, seed=1), sr.spawner(rate=3.0, seed=2, shape=sr.BALL)]
    dt = f32(1.0)
    rec = pool(40, [3, 7, 8, 20, 21, 39])                                  # D = 6 < n = 8: spawner 1 loses two of its three
    st = sr.new_state(2)
    out = sr.step(rec, sp, st, dt, DIMS)
    assert (st["born"], st["dropped"], st["blocked"]) == (6, 2, 0) and st["serial"] == [5, 3]
    assert np.array_equal(out[[3, 7, 8, 20, 21]], sr.records_of(sp[0], 0, np.arange(5)))
    assert np.array_equal(out[[39]], sr.records_of(sp[1], 1, [0]))
    live = np.setdiff1d(np.arange(40), [3, 7, 8, 20, 21, 39])
    assert np.array_equal(out[live].view(np.uint32), rec[live].view(np.uint32))
    # the next step has no dead slot at all: everything is dropped, the serials advance all the same
    out2 = sr.step(out, sp, st, dt, DIMS)
    assert np.array_equal(out2.view(np.uint32), out.view(np.uint32))
    assert (st["born"], st["dropped"]) == (6, 10) and st["serial"] == [10, 6]
    # a slot freed now takes the serial the model has: position is a function of (seed, s, k) alone
    out2[11, 3] = -1
    out3 = sr.step(out2, sp, st, dt, DIMS)
    assert np.array_equal(out3[[11]], sr.records_of(sp[0], 0, [10])) and st["serial"] == [15, 9] and st["dropped"] == 17


def test_a_blocked_slot_keeps_its_bits():
    sp = [sr.spawner(rate=64.0, seed=9, center=(0.5, 0.5, 0.5), half_extent=(0.5, 0.25, 0.25))]
    solid = np.zeros(DIMS[::-1], np.uint8)
    solid[:, :, DIMS[0] // 2:] = 1                                         # the +x half of the box
    rec = pool(100, np.arange(0, 100, 1))
    rec[:, 3] = np.where(np.arange(100) % 2 == 0, f32(-3.5), f32(np.nan))
    rec[5, :3] = np.array([0x7fc01234, 0xffc00001, 0x7f800001], np.uint32).view(f32)      # NaN payloads in a dead record
    st = sr.new_state(1)
    out = sr.step(rec, sp, st, f32(1.0), DIMS, solid=solid)
    assert st["born"] + st["blocked"] == 64 and 16 <= st["blocked"] <= 48 and st["dropped"] == 0
    want = sr.records_of(sp[0], 0, np.arange(64))
    hit = want[:, 0] * f32(DIMS[0]) >= DIMS[0] // 2
    assert int(hit.sum()) == st["blocked"]
    assert np.array_equal(out[:64][hit].view(np.uint32), rec[:64][hit].view(np.uint32))   # blocked: every bit kept, the birth is not retried
    assert np.array_equal(out[:64][~hit], want[~hit])
    assert np.array_equal(out[64:].view(np.uint32), rec[64:].view(np.uint32))


def test_births_skip_negative_zero_ages_and_take_nan_ages():
    rec = np.zeros((6, 4), f32)
    rec[:, 3] = [-0.0, np.nan, 0.0, -1e-30, 2.0, -np.inf]
    sp = [sr.spawner(rate=6.0, seed=4, age_spread=2.0)]
    st = sr.new_state(1)
    out = sr.step(rec, sp, st, f32(1.0), DIMS)
    assert (st["born"], st["dropped"]) == (3, 3)
    assert np.array_equal(out[[1, 3, 5]], sr.records_of(sp[0], 0, [0, 1, 2]))
    assert np.array_equal(out[[0, 2, 4]].view(np.uint32), rec[[0, 2, 4]].view(np.uint32)) and np.signbit(out[0, 3])
    assert (out[[1, 3, 5], 3] >= 0).all() and (out[[1, 3, 5], 3] < 2).all() and len(set(out[[1, 3, 5], 3])) == 3
    # the clamp acts where a box reaches over a wall, and stores +0 / 1
    sp = [sr.spawner(rate=1.0, center=(0.0, 1.0, 0.5), half_extent=(0.2, 0.2, 0.0))]
    r = sr.records_of(sp[0], 0, np.arange(256))
    assert (r[:, 0] == 0).sum() > 64 and not np.signbit(r[:, 0]).any() and (r[:, 1] == 1).sum() > 64 and (r[:, 2] == 0.5).all()
    assert ((r[:, :3] >= 0) & (r[:, :3] <= 1)).all()


# ---- 5: the built library --------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_spawner_calls_and_capi_binds_them():
    from fluidx12_amd import capi
    lib = capi.load()
    for name in ("fx_set_particle_spawners", "fx_get_particle_spawners", "fx_spawn_particles", "fx_particle_spawn_info"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    assert C.sizeof(capi.ParticleSpawner) == 48 and C.sizeof(capi.ParticleSpawnInfo) == 160
    assert capi.MAX_PARTICLE_SPAWNERS == 16 and (capi.SPAWN_BOX, capi.SPAWN_BALL) == (0, 1)
    # a NULL context is refused before anything is touched: the calls can be made without a GPU
    n = C.c_uint32(7)
    assert lib.fx_set_particle_spawners(None, None, 0) == capi.FX_E_INVALID
    assert lib.fx_get_particle_spawners(None, None, 0, C.byref(n)) == capi.FX_E_INVALID and n.value == 7
    assert lib.fx_spawn_particles(None, None) == capi.FX_E_INVALID
    assert lib.fx_particle_spawn_info(None, None, None) == capi.FX_E_INVALID
    import fluidx12_amd as fx
    for member in ("SetParticleSpawners", "GetParticleSpawners", "SpawnParticles", "ParticleSpawnInfo", "SetParticlePool"):
        assert callable(getattr(fx.Fluid, member)), member
