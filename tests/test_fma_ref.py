"""tests/fma_ref.py, the fused multiply-add of every numpy model, against libm's fmaf, bit for bit (no device is needed): operands of one
scale, exponents 40 - 80 binades apart, subnormal addends and results, the constructed tie that a float64 sum rounded twice gets wrong with
its sign and operand-order variants -- and the advection case that tie first showed in."""
import ctypes
import itertools

import numpy as np
import pytest

import fma_ref

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def fmaf():
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3

    def call(a, b, c):
        return np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], f32)
    return call


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def twice_rounded(a, b, c):
    """what the models used before: the float64 sum rounded to float64, then to float32"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def scaled(rng, n, lo, hi):
    """float32 values with random signs, mantissas uniform, exponents uniform in [lo, hi]"""
    with np.errstate(under="ignore"):
        return (rng.uniform(1, 2, n) * np.exp2(rng.integers(lo, hi + 1, n).astype(f64)) * rng.choice([-1.0, 1.0], n)).astype(f32)


def check(fmaf, a, b, c):
    got, want = fma_ref.fma(a, b, c), fmaf(a, b, c)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, [(float(a[i]).hex(), float(b[i]).hex(), float(c[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:4]]


N = 20000


def test_operands_of_one_scale(fmaf):
    rng = np.random.default_rng(811)
    check(fmaf, scaled(rng, N, -3, 3), scaled(rng, N, -3, 3), scaled(rng, N, -6, 6))
    # a lerp's: fma(f, b - a, a) with f in [0, 1) -- heavy cancellation
    a, b = rng.standard_normal(N).astype(f32), rng.standard_normal(N).astype(f32)
    check(fmaf, rng.random(N).astype(f32), b - a, a)


@pytest.mark.parametrize("sign", [1, -1])
def test_exponents_forty_to_eighty_binades_apart(fmaf, sign):
    """the addend lies 40 - 80 binades below (above) the product: far below the float32 result's last place, but it decides a tie, and down to
    ~53 binades it reaches into the float64 sum"""
    rng = np.random.default_rng(812)
    a, b = scaled(rng, N, -10, 10), scaled(rng, N, -10, 10)
    gap = rng.integers(40, 81, N)
    e = np.floor(np.log2(np.abs(a.astype(f64) * b.astype(f64)))) - sign * gap
    c = (rng.uniform(1, 2, N) * np.exp2(e) * rng.choice([-1.0, 1.0], N)).astype(f32)
    assert np.isfinite(c).all() and (c != 0).all()
    check(fmaf, a, b, c)
    # products that sit EXACTLY on a float32 tie (12-bit factors squared), the small addend alone decides the side
    k = rng.integers(1, 1 << 11, N) * 2 + 1                    # odd: (1 + k 2^-12)^2 has its last set bit at 2^-24
    t = (1 + k * 2.0 ** -12).astype(f32)
    check(fmaf, t, t, c.astype(f32) * f32(2.0 ** -20) if sign > 0 else c)


def test_subnormal_addends_and_results(fmaf):
    rng = np.random.default_rng(813)
    tiny = (rng.standard_normal(N) * 2.0 ** -128).astype(f32)
    assert ((np.abs(tiny) > 0) & (np.abs(tiny) < np.finfo(f32).tiny)).mean() > 0.99
    check(fmaf, scaled(rng, N, -3, 3), scaled(rng, N, -3, 3), tiny)                          # a normal product and a subnormal addend
    check(fmaf, rng.random(N).astype(f32), (rng.standard_normal(N) * 2.0 ** -128).astype(f32), tiny)    # a lerp of subnormals: subnormal results
    check(fmaf, scaled(rng, N, -70, -60), scaled(rng, N, -70, -60), tiny)                    # the product itself rounds in the subnormal range
    check(fmaf, scaled(rng, N, -80, -70), scaled(rng, N, -80, -70), np.zeros(N, f32))        # ... and underflows to +-0


def test_the_constructed_tie(fmaf):
    """a = b = 1 + 2^-12, c = 2^-60: a * b = 1 + 2^-11 + 2^-24, half an ulp above 1 + 2^-11, and a hair more.  Signs and operand orders"""
    t, c = f32(1 + 2.0 ** -12), f32(2.0 ** -60)
    assert float(fma_ref.fma(t, t, c)).hex() == "0x1.0020020000000p+0" and float(fma_ref.fma(t, t, -c)).hex() == "0x1.0020000000000p+0"
    assert float(twice_rounded(t, t, c)).hex() == "0x1.0020000000000p+0"       # the double rounding this file is there to keep out
    cases = []
    for sa, sb, sc in itertools.product([1, -1], repeat=3):
        cases.append((sa * t, sb * t, sc * c))
    u = f32(1 + 2.0 ** -11 + 2.0 ** -24)                       # the tie as a product with 1: x * 1 + c, c * 1 + x, in both factor orders
    for sx, sc in itertools.product([1, -1], repeat=2):
        x = f32(2.0 ** -24) * sx
        big = f32(1 + 2.0 ** -11) * sx
        cases += [(f32(2.0 ** -12) * sx, f32(2.0 ** -12), big), (f32(2.0 ** -12), f32(2.0 ** -12) * sx, big)]    # 2^-24 + big: an exact tie, to even
        cases += [(x, f32(1), big), (f32(1), x, big)]
        cases += [(t * sx, t, sc * c), (t, t * sx, sc * c), (sc * c, f32(1), f32(1) * sx), (f32(1), sc * c, u * sx)]
    a, b, c3 = (np.array(v, f32) for v in zip(*cases))
    check(fmaf, a, b, c3)
    assert (bits(twice_rounded(a, b, c3)) != bits(fmaf(a, b, c3))).any()


def test_special_values(fmaf):
    v = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1e-45], f32)
    a, b, c = (x.ravel() for x in np.meshgrid(v, v, v, indexing="ij"))
    with np.errstate(all="ignore"):
        got, want = fma_ref.fma(a, b, c), fmaf(a, b, c)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])
    assert isinstance(fma_ref.fma(f32(2), f32(3), f32(1)), np.floating) and fma_ref.fma(f32(2), f32(3), f32(1)) == f32(7)


def test_the_advection_model_equals_the_oracle_where_the_double_rounding_did_not(monkeypatch):
    """129 x 129 x 12, clamp, the fp32 subnormal recipe of tests/advect_edges.py: the semi-Lagrangian model equals the oracle outside the impulse
    ball bit for bit.  With the float64 sum rounded twice in the sampler's lerps it does not: one velocity value -- component 0 at z 11, y 71,
    x 89 -- comes out an ulp off, the kind of difference the bit-for-bit GPU tests would have pinned on a kernel"""
    import advect_edges as ae
    import buoyancy_ref as br
    import maccormack_ref as mr
    dims = (129, 129, 12)
    c = ae.subnormal(dims, "clamp")
    far = c.far
    assert np.array_equal(bits(c.want_vel[:, far]), bits(c.orc_vel[:, far])) and np.array_equal(bits(c.want_col[far]), bits(c.orc_col[far]))
    monkeypatch.setattr(br, "fma", twice_rounded)
    ov, oc = mr.step(c.vel, c.col, c.dt, "clamp", impulse=False, scheme="semi-lagrangian")
    where = np.argwhere(bits(ov) != bits(c.want_vel)).tolist()
    print("twice rounded: differs at %s: %r against %r" % (where, [float(ov[tuple(w)]) for w in where], [float(c.orc_vel[tuple(w)]) for w in where]))
    assert where == [[0, 11, 71, 89]] and far[11, 71, 89] and np.array_equal(bits(oc), bits(c.want_col))
    assert bits(ov[0, 11, 71, 89]) != bits(c.orc_vel[0, 11, 71, 89])
