"""CPU checks of the solid obstacles (fx_set_obstacles): the C++ reference tests/obstacle_ref/ -- anchored to the oracle (an all-zero mask
changes no bit of the divergence, the relaxation and the projection), its code bytes against plain Python loops, and a plate across the box
that seals the half behind it.  tests/test_gpu_obstacles.py holds the kernels against this reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_u8 = C.POINTER(C.c_uint8)
_fpt = C.POINTER(C.c_float)

# ---- the reference: tests/obstacle_ref/ + the oracle's advection, built with the oracle's flags --------------------------------------
_SRCS = [os.path.join(ROOT, "tests", "obstacle_ref", "obstacle_ref.cpp"), os.path.join(ROOT, "oracle", "orc_sim.cpp")]
_DEPS = _SRCS + [os.path.join(ROOT, "oracle", h) for h in ("orc_common.h", "fx_oracle.h")]
_LIB = None


def obstacle_ref_lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "_build", "libobstacleref.so")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in _DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = ["-O3", "-std=c++17", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2"]   # oracle/Makefile
            subprocess.run(["g++"] + flags + ["-shared", "-o", out] + _SRCS + ["-lm"], check=True)
        _LIB = C.CDLL(out)
    return _LIB


def _fp(a):
    return a.ctypes.data_as(_fpt)


def _up(a):
    return a.ctypes.data_as(_u8)


def _mask(mask):
    return np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)


def ref_codes(mask):
    m = _mask(mask)
    Z, Y, X = m.shape
    code = np.empty_like(m)
    obstacle_ref_lib().obr_codes(_up(m), _up(code), X, Y, Z)
    return code


def ref_enforce(vel, col, mask):
    """-> (vel, col) with the solid cells at +0"""
    m = _mask(mask)
    Z, Y, X = m.shape
    v, c = np.array(vel, f32, order="C"), np.array(col, f32, order="C")
    obstacle_ref_lib().obr_enforce(_fp(v), _fp(c), _up(m), X, Y, Z)
    return v, c


def ref_divergence(vel, mask):
    m = _mask(mask)
    Z, Y, X = m.shape
    v = np.ascontiguousarray(vel, f32)
    b = np.empty((Z, Y, X), f32)
    obstacle_ref_lib().obr_divergence(_fp(v), _up(m), _fp(b), X, Y, Z)
    return b


def ref_jacobi(p, b, mask, n):
    m = _mask(mask)
    Z, Y, X = m.shape
    p, b = np.array(p, f32, order="C"), np.ascontiguousarray(b, f32)
    tmp = np.empty_like(p)
    obstacle_ref_lib().obr_jacobi(_fp(p), _fp(b), _up(m), _fp(tmp), X, Y, Z, int(n))
    return p


def ref_project(vel, p, mask, half=False):
    m = _mask(mask)
    Z, Y, X = m.shape
    v, p = np.ascontiguousarray(vel, f32), np.ascontiguousarray(p, f32)
    out = np.empty_like(v)
    obstacle_ref_lib().obr_project(_fp(v), _fp(p), _up(m), _fp(out), X, Y, Z, int(half))
    return out


class RefSim:
    """orc.Sim with a mask: the reference's whole step (the oracle's advection, then enforce, divergence, sweeps, projection)"""

    def __init__(self, X, Y, Z, mask, iters=40, address=0, half=False):
        self.s = orc.Sim(X, Y, Z, iters=iters, address=address, half=half)
        self.mask = _mask(mask).reshape(Z, Y, X)

    def step(self, dt=None):
        s = self.s
        dt = f32(s.default_dt() if dt is None else dt)
        if dt > 0:
            s.parity ^= 1
        p = s.parity
        obstacle_ref_lib().obr_step(_fp(s.vel[0]), _fp(s.vel[1]), _fp(s.col[1 - p]), _fp(s.col[p]), _fp(s.p), _fp(s.b), _fp(s.tmp), _up(self.mask),
                                    s.X, s.Y, s.Z, C.c_float(float(dt)), s.iters, s.address, int(s.half))

    velocity = property(lambda self: self.s.velocity)
    color = property(lambda self: self.s.color)
    pressure = property(lambda self: self.s.p)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the masks of the GPU tests ------------------------------------------------------------------------------------------------------
def random_mask(dims, seed=11, p=0.3):
    X, Y, Z = dims
    return (np.random.default_rng(seed).random((Z, Y, X)) < p).astype(np.uint8)


def ball_mask(dims, center=(0.5, 0.45, 0.5), radius=0.22):
    """cells whose centre lies within `radius` of `center` in texture space (2-D grids: a disc)"""
    X, Y, Z = dims
    z, y, x = np.meshgrid((np.arange(Z) + 0.5) / Z, (np.arange(Y) + 0.5) / Y, (np.arange(X) + 0.5) / X, indexing="ij")
    d2 = (x - center[0]) ** 2 + (y - center[1]) ** 2 + ((z - center[2]) ** 2 if Z > 1 else 0.0)
    return (d2 <= radius * radius).astype(np.uint8)


def plate_mask(dims):
    """a full-cross-section plate two cells thick at mid-y"""
    X, Y, Z = dims
    m = np.zeros((Z, Y, X), np.uint8)
    m[:, Y // 2:Y // 2 + 2, :] = 1
    return m


SEAL_DIMS, SEAL_STEPS, SEAL_ITERS = (24, 24, 24), 16, 20     # SEAL_STEPS: see test_a_plate_seals_the_far_half


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,z", [(20, 5), (36, 1), (64, 8)])
def test_an_all_zero_mask_is_the_oracle_bit_for_bit(n, z):
    rng = np.random.default_rng(7)
    vel = rng.standard_normal((3, z, n, n)).astype(f32)
    p = rng.standard_normal((z, n, n)).astype(f32)
    none = np.zeros((z, n, n), np.uint8)
    b = orc.divergence(vel)
    assert np.array_equal(bits(ref_divergence(vel, none)), bits(b))
    assert np.array_equal(bits(ref_jacobi(p, b, none, 5)), bits(orc.jacobi(p, b, 5)[0]))
    for half in (False, True):
        v = vel.astype(np.float16).astype(f32) if half else vel
        assert np.array_equal(bits(ref_project(v, p, none, half)), bits(orc.project(v, p, half)))
    col = rng.random((z, n, n, 4)).astype(f32)
    v, c = ref_enforce(vel, col, none)
    assert np.array_equal(bits(v), bits(vel)) and np.array_equal(bits(c), bits(col))


def test_code_bytes_are_the_plain_loops():
    X, Y, Z = dims = (12, 12, 5)
    m = random_mask(dims, seed=2)
    want = np.zeros((Z, Y, X), np.uint8)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                nb = [(max(x - 1, 0), y, z), (min(x + 1, X - 1), y, z), (x, max(y - 1, 0), z), (x, min(y + 1, Y - 1), z),
                      (x, y, max(z - 1, 0)), (x, y, min(z + 1, Z - 1))]
                k = sum(1 << i for i, (a, b, c) in enumerate(nb) if m[c, b, a])
                want[z, y, x] = k | (64 if m[z, y, x] else 0)
    got = ref_codes(m)
    assert np.array_equal(got, want)
    assert len(np.unique(got)) > 100                                  # a 30 % mask meets most of the 128 combinations
    # a 2-D grid has no z neighbours: the z bits stay 0 even though the clamped z index names the cell itself
    m2 = random_mask((12, 12, 1), seed=3)
    c2 = ref_codes(m2)
    assert not (c2 & 0x30).any() and np.array_equal((c2 >> 6) & 1, m2)


def test_the_rules_on_a_single_solid_cell():
    """one solid cell in a uniform field: what each rule does around it, by hand"""
    X = Y = 9
    Z = 5
    m = np.zeros((Z, Y, X), np.uint8)
    m[2, 4, 4] = 1
    vel = np.ones((3, Z, Y, X), f32)
    b = ref_divergence(vel, m)
    assert b[2, 4, 4] == 0 and b[2, 4, 3] == f32(-0.5) and b[2, 4, 5] == f32(0.5) and b[2, 3, 4] == f32(-0.5) and b[1, 4, 4] == f32(-0.5)
    assert b[2, 2, 2] == 0                                             # away from it: a uniform field has none
    p = np.arange(Z * Y * X, dtype=f32).reshape(Z, Y, X)
    q = ref_jacobi(p, np.zeros_like(p), m, 1)
    assert q[2, 4, 4] == 0
    L, R, U, D, F, B = p[2, 4, 2], p[2, 4, 3], p[2, 3, 3], p[2, 5, 3], p[1, 4, 3], p[3, 4, 3]      # the cell left of it: its +x neighbour reads as itself
    assert q[2, 4, 3] == f32(f32(f32(f32(f32(f32(L - 0) + R) + U) + D) + F) + B) * np.array([0x3e2aaaab], np.uint32).view(f32)[0]
    out = ref_project(vel, np.zeros_like(p), m)
    assert not out[:, 2, 4, 4].any()
    assert out[0, 2, 4, 3] == 0 and out[0, 2, 4, 5] == 0 and out[1, 2, 3, 4] == 0 and out[2, 1, 4, 4] == 0      # no flow into or out of it
    assert out[1, 2, 4, 3] == 1 and out[2, 2, 4, 3] == 1               # ... and free slip along it


def test_a_plate_seals_the_far_half():
    """24^3 from zero fields with the built-in impulse (at y = 0.1): behind a full plate at mid-y nothing ever moves.  SEAL_STEPS was chosen
    on the CPU from orc.Sim: without the plate the velocity beyond it is non-zero from the first step on and the first smoke arrives there in
    step 11 (colour 0.02); 16 steps leave a margin"""
    X, Y, Z = SEAL_DIMS
    m = plate_mask(SEAL_DIMS)
    far = slice(Y // 2 + 2, Y)
    with_plate, control = RefSim(X, Y, Z, m, iters=SEAL_ITERS), orc.Sim(X, Y, Z, iters=SEAL_ITERS)
    for _ in range(SEAL_STEPS):
        with_plate.step()
        control.step()
    assert control.color[:, far].max() > 0 and np.abs(control.velocity[:, :, far]).max() > 0
    assert not with_plate.velocity[:, :, far].any() and not with_plate.color[:, far].any()
    assert with_plate.color[:, :Y // 2].max() > 0                     # the smoke is there, in front of the plate
    solid = m.astype(bool)
    assert not bits(with_plate.velocity)[:, solid].any() and not bits(with_plate.color)[solid].any()      # +0, bit for bit
