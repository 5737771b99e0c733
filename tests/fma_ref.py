"""The one fused multiply-add of the numpy models (emitter_ref, buoyancy_ref, maccormack_ref, open_ref, multigrid_ref): fmaf, correctly rounded.

Two float32 factors multiply exactly in float64 (48 significant bits).  Adding the addend in float64 and rounding that sum to float32 would
round twice: with a = b = 1 + 2^-12 and c = 2^-60 the float64 sum is 1 + 2^-11 + 2^-24 exactly -- c is lost --, a tie that goes to the even
0x1.002p+0, where fmaf gives 0x1.002002p+0.  So the float64 sum is rounded to ODD first (TwoSum gives its exact error; an inexact even sum moves
one place towards the error): a sum between two float32 values, or on their midpoint, keeps which side it lies on, and the single rounding to
float32 that follows -- 53 bits are more than 24 + 2 -- is the one fmaf makes.  tests/test_fma_ref.py holds it to libm's fmaf bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64


def fma(a, b, c):
    """fmaf(a, b, c) for float32 scalars or arrays: a float32 scalar or array"""
    p = np.asarray(a, f64) * np.asarray(b, f64)
    c = np.asarray(c, f64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                         # TwoSum: p + c = s + e exactly
        even = (np.asarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (e != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)[()]
