"""Vorticity confinement without a GPU: the properties the numpy model (tests/vorticity_ref.py) must have -- it is the reference the
kernel is compared with bit for bit in tests/test_gpu_vorticity.py -- and the two entry points of the C ABI, through capi only."""
import numpy as np

import vorticity_ref as vr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_field(shape, seed):
    X, Y, Z = shape
    return (np.random.default_rng(seed).standard_normal((3, Z, Y, X)) * 0.5).astype(np.float32)


def test_rigid_rotation_is_left_alone_away_from_the_walls():
    """|w| of a rigid rotation is constant where the differences are central, so grad |w| = 0 exactly two cells off the walls (every value
    is a small multiple of 1/64: nothing rounds, the force is an exact zero); the one-sided differences at the walls change |w| there, and the shell moves"""
    n, c = 24, 12.0
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    u = np.stack([(z - c) / 64.0, np.zeros_like(z, float), (c - x) / 64.0]).astype(np.float32)      # (z - c, 0, -(x - c)) / 64, written without a -0.0 at x = c: u + 0 is +0
    out = vr.confine(u, 8.0, 2.0 / n)
    assert out.dtype == np.float32 and out.shape == u.shape
    core = (slice(None), slice(2, n - 2), slice(2, n - 2), slice(2, n - 2))
    assert np.array_equal(bits(out[core]), bits(u[core]))
    shell = np.ones(u.shape, bool)
    shell[core] = False
    assert (bits(out)[shell] != bits(u)[shell]).any()
    assert np.isfinite(out).all()


def test_x_mirror_equivariance_is_bitwise():
    for shape in ((16, 16, 16), (20, 20, 12), (40, 40, 1)):
        u = random_field(shape, 3)
        mirror = lambda f: np.stack([-f[0, :, :, ::-1], f[1, :, :, ::-1], f[2, :, :, ::-1]])
        a = vr.confine(mirror(u), 8.0, 0.05)
        b = mirror(vr.confine(u, 8.0, 0.05))
        assert np.array_equal(bits(a), bits(b)), shape


def test_2d_leaves_uz_alone():
    u = random_field((40, 40, 1), 5)
    out = vr.confine(u, 8.0, 1.0 / 40)
    assert np.array_equal(bits(out[2]), bits(u[2]))
    assert (bits(out[0]) != bits(u[0])).any() and (bits(out[1]) != bits(u[1])).any()
    assert np.isfinite(out).all()


def test_zero_field_stays_zero():
    for shape in ((16, 16, 16), (36, 36, 1)):
        X, Y, Z = shape
        out = vr.confine(np.zeros((3, Z, Y, X), np.float32), 8.0, 0.1)
        assert not out.any() and np.isfinite(out).all()


def test_eps_zero_is_the_identity():
    for shape in ((16, 16, 16), (72, 72, 20), (40, 40, 1)):
        u = random_field(shape, 7)
        assert np.array_equal(bits(vr.confine(u, 0.0, 0.1)), bits(u))


def test_fp32_model_tracks_the_fp64_model():
    """the float64 mode is the same formulas in double.  On random data of size 0.5 the guard 1e-6 is far below |grad m| and the force term
    (g x w) * eps * dt / |g| is O(1): each of its ~20 fp32 operations contributes about an ulp (6e-8), the differences that form w and g
    lose a few bits to cancellation -- 1e-4 is some hundred ulp of headroom over that, three orders below the term itself"""
    for shape in ((16, 16, 16), (72, 72, 20), (40, 40, 1)):
        u = random_field(shape, 11)
        a = vr.confine(u, 8.0, 2.0 / shape[1])
        b = vr.confine(u, 8.0, 2.0 / shape[1], dtype=np.float64)
        assert b.dtype == np.float64
        assert np.abs(a - b).max() < 1e-4


def test_fp16_storage_rounds_input_and_output():
    u = random_field((16, 16, 16), 13)
    out = vr.confine_stored(u, 8.0, 0.125, True)
    assert np.array_equal(out, out.astype(np.float16).astype(np.float32))
    u16 = u.astype(np.float16).astype(np.float32)
    assert np.array_equal(bits(out), bits(vr.confine(u16, 8.0, 0.125).astype(np.float16).astype(np.float32)))


# ---- the C ABI, through capi only -----------------------------------------------------------------------------------------------
def test_header_declares_both_functions():
    import os
    import re
    from fluidx12_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fluidx_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fx_set_vorticity_confinement\s*\(\s*fx_ctx\s*\*\s*\w+\s*,\s*float\s+\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+fx_confine_vorticity\s*\(\s*fx_ctx\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", src)
    for name in ("fx_set_vorticity_confinement", "fx_confine_vorticity"):
        assert name in capi.SYMBOLS
        assert hasattr(capi.load(), name)
    assert capi.ABI_VERSION == 7


def test_null_context_is_refused():
    from fluidx12_amd import capi
    lib = capi.load()
    assert lib.fx_set_vorticity_confinement(None, 1.0) == capi.FX_E_INVALID
    assert lib.fx_confine_vorticity(None, None) == capi.FX_E_INVALID
