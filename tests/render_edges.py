"""Input recipes of tests/test_gpu_render_edges.py: colour fields that hold what the simulation can store and a caller can upload but no
render test has held -- alpha outside [0, 1] -- for the ray marches (csrc/fx_march.h), above all for the contract that the accelerated marches
(csrc/fx_render_accel.hip) equal the plain ones (csrc/fx_render.hip) bit for bit.  Inputs and conditions only, in the style of
tests/store_edges.py; tests/test_render_edges.py holds them to their conditions on the oracle alone (no GPU).

  part 1  one field per value class of alpha (CLASSES): NaN, +inf, negative, -0, (1, 1.25], > 1.25, binary16 subnormal, fp32 subnormal
  part 2  one field for the colour channels: ordinary alpha; rgb negative, above 1, 65504, +inf, subnormal, -0
  part 3  light settings (fx_set_light) under which every light-map word of an EMPTY volume is pack_r11g11b10 of three chosen values

A class field, bottom to top in y (the default light, fx_context.cpp: directional from (75, 75, -75), shines along (-1, -1, 1) -- a voxel's
shadow ray runs towards +x, +y, -z; the default camera at (4, 16, -40) looks down on the volume from the front):
  * the body: y blocks [0, dim), every x and z: alpha in [0.05, 0.9], rgb in [0, 1).  Its shadow rays climb through everything above it.
  * the dim layer: one layer of 4^3 blocks, alpha in [0.0005, 0.005] -- below the view march's 0.01 threshold, so whether a block of it is
    `visible` is decided by the class voxels embedded in it, one per block (DIM-EMBEDDED)
  * one layer of blocks of +0 (two where a step follows: the advection's filter smears a voxel one voxel wide on grids that are no power of two)
  * in that layer, in the corner x < 12, z < 8: the probe -- one voxel of alpha 0.875 with a class voxel next to it (class_field)
  * the top layer(s): +0 but for one class voxel per block column (ISOLATED): every other alpha of the 3 x 3 x 3 blocks around its block is
    bit-exact +0 or another voxel of the class, so whether those blocks count as occupied (`pos`) is decided by class voxels alone
Everything is binary16-representable (but the fp32 subnormals), so fp16 and fp32 contexts render the same numbers.

Which build kernel a grid reaches (launch_accel_build, fx_render_accel.hip): a field that was uploaded has no current alpha side volume:
k_occupancy_blocks<HALF, false> by storage, then the three-pass light volume (k_light_cells, k_light_classify; all_exact on 16^3 and 32^3,
eight taps per centre sample and short blocks at the far faces on 18 x 18 x 10).  After a render and one fx_simulate the advection has written
the side volume (fx_schedule.cpp advect_range: the frame before was rendered on the same stream with FX_OPT_RENDER_ACCEL on) and the build is
k_build_fill where X, Y and Z are powers of two (32^3), k_occupancy_blocks_a4 where X % 4 == 0 (36 x 36 x 12), k_occupancy_blocks<false, true>
otherwise (18 x 18 x 10).  The step runs with velocity 0, the impulse off and dt = 2^-10: a back-trace ends on its own voxel's centre, the
stored value is the filter's times the attenuation 1 - 0.2 dt.  The field the render then reads is the device's own: the GPU test downloads it
and asserts the class counts on it.  (The coarse mask level of grids above 256^3 reads the same occ[] through the same comparisons.)"""
import functools
from fractions import Fraction

import numpy as np

import emitter_ref as er
import maccormack_ref as mr
from store_edges import assert_conditions, bits, case, same_bits  # noqa: F401  (re-exported to the tests)

f32 = np.float32
FRESH_GRIDS = [(18, 18, 10), (16, 16, 16), (32, 32, 32)]
STEP_GRIDS = [(32, 32, 32), (36, 36, 12), (18, 18, 10)]
STEP_DT = f32(2.0 ** -10)
NL = 24                                                          # light samples (SetMaxSamples): enough for a shadow ray to cross the grid
NS = 48
VP = (96, 72)
# a light probe that tells directions apart: constant term and strong linear terms (9 x rgb)
SH = np.array([[2.0, 1.8, 1.6], [0.9, -0.7, 0.5], [0.6, 0.8, -0.9], [-0.8, 0.5, 0.7], [0.2, 0.1, 0.3], [0.1, 0.3, 0.2], [0.3, 0.2, 0.1], [0.1, 0.2, 0.2], [0.2, 0.1, 0.1]], f32)

# name -> (values the class voxels cycle through, fp32 storage only)
CLASSES = {
    "nan": ((np.nan,), False),
    "inf": ((np.inf,), False),
    "negative": ((-0.5, -0.0625, -3.0), False),
    "negzero": ((-0.0,), False),
    "gt1": ((1.125, 1.25, 1.0009765625), False),
    "gt125": ((2.0, 7.5, 300.0, 1.2509765625), False),
    "half_subnormal": ((2.0 ** -24, 1.5 * 2.0 ** -20, 2.0 ** -15, 1023 * 2.0 ** -24), False),
    "fp32_subnormal": ((2.0 ** -149, 2.0 ** -130, 2.0 ** -127), True),
}
FINITE = ["negative", "negzero", "gt1", "gt125", "half_subnormal", "fp32_subnormal"]


def storages(name):
    return ["fp32"] if CLASSES[name][1] else ["fp32", "fp16"]


def class_mask(alpha, name, stepped=False):
    """the voxels of class `name`.  stepped: on a field behind an advection, whose filter makes NaN of inf - inf and of 0 * inf"""
    a = np.asarray(alpha, f32)
    with np.errstate(invalid="ignore"):
        if name == "nan":
            return np.isnan(a)
        if name == "inf":
            return np.isposinf(a) | (np.isnan(a) if stepped else False)
        if name == "negative":
            return a <= -f32(2.0 ** -126) if not stepped else a < 0
        if name == "negzero":
            return bits(a) == 0x80000000
        if name == "gt1":
            return (a > 1) & (a <= f32(1.25))
        if name == "gt125":
            return (a > f32(1.25)) & np.isfinite(a)
        if name == "half_subnormal":
            return (a >= f32(2.0 ** -25 if stepped else 2.0 ** -24)) & (a < f32(2.0 ** -14))      # (stepped, fp32: the attenuation takes an ulp off 2^-24)
        if name == "fp32_subnormal":
            return (a > 0) & (a < f32(2.0 ** -126))
    raise KeyError(name)


def _blocks(flag):
    """[CZ][CY][CX]: any voxel of the 4^3 block (short at the far faces) has `flag`"""
    Z, Y, X = flag.shape
    p = np.zeros(((Z + 3) // 4 * 4, (Y + 3) // 4 * 4, (X + 3) // 4 * 4), bool)
    p[:Z, :Y, :X] = flag
    return p.reshape(p.shape[0] // 4, 4, p.shape[1] // 4, 4, p.shape[2] // 4, 4).any(axis=(1, 3, 5))


def _spread(b, lo, hi):
    """b over the blocks c + lo .. c + hi per axis (clipped at the faces)"""
    out = b.copy()
    for axis in range(3):
        acc = out.copy()
        for d in range(lo, hi + 1):
            if d == 0:
                continue
            sh = np.roll(out, -d, axis)
            idx = [slice(None)] * 3
            idx[axis] = slice(-d, None) if d > 0 else slice(0, -d)
            sh[tuple(idx)] = False
            acc |= sh
        out = acc
    return out


def _of_voxels(blockflag, shape):
    Z, Y, X = shape
    return np.repeat(np.repeat(np.repeat(blockflag, 4, 0), 4, 1), 4, 2)[:Z, :Y, :X]


def index_lists(alpha, name, stepped=False):
    """(isolated, dim_embedded): index arrays [n][3] (z, y, x) of the class voxels of the field `alpha` [Z][Y][X] for which
      isolated      every alpha of the 3 x 3 x 3 blocks around the voxel's block that is not of the class is bit-exact +0
      dim-embedded  every alpha of the voxel's block that is not of the class lies in (0, 0.005], and no alpha of the blocks c .. c + 1 --
                    what k_occupancy_dilate folds into the voxel's block -- that is not of the class exceeds 0.005 or is negative or NaN"""
    a = np.asarray(alpha, f32)
    cls = class_mask(a, name, stepped)
    other = ~cls
    iso = cls & ~_of_voxels(_spread(_blocks(other & (bits(a) != 0)), -1, 1), a.shape)
    with np.errstate(invalid="ignore"):
        dim_ok = (a > 0) & (a <= f32(0.005))
        low_ok = dim_ok | (bits(a) == 0)
    emb = cls & ~_of_voxels(_blocks(other & ~dim_ok), a.shape) & _of_voxels(_blocks(other & dim_ok), a.shape) \
        & ~_of_voxels(_spread(_blocks(other & ~low_ok), 0, 1), a.shape)
    return np.argwhere(iso), np.argwhere(emb)


def layers(dims, stepped):
    """y block layers (body blocks, dim block, first isolated block)"""
    CY = (dims[1] + 3) // 4
    top = 2 if CY >= 8 else 1
    gap = 2 if stepped else 1
    dim = CY - top - gap - 1
    assert dim >= 1
    return dim, dim, CY - top


def to_half(a):
    return np.asarray(a, f32).astype(np.float16).astype(f32)


@functools.lru_cache(maxsize=None)
def class_field(dims, name, stepped=False):
    """Case: col float32[Z][Y][X][4], the index lists by construction, and `without`: the field with every class voxel's alpha set to +0"""
    X, Y, Z = dims
    rng = np.random.default_rng(9100 + X + 7 * Z)
    nb, dimb, isob = layers(dims, stepped)
    col = np.zeros((Z, Y, X, 4), f32)
    yb = 4 * nb
    col[:, :yb, :, :3] = to_half(rng.random((Z, yb, X, 3)))
    col[:, :yb, :, 3] = to_half(0.05 + 0.85 * rng.random((Z, yb, X)))
    col[:, yb:yb + 4, :, :3] = to_half(rng.random((Z, 4, X, 3)))
    col[:, yb:yb + 4, :, 3] = to_half(0.0005 + 0.0045 * rng.random((Z, 4, X)))
    values = CLASSES[name][0]
    iso, emb = [], []
    k = 0
    for bz in range((Z + 3) // 4):
        for bx in range((X + 3) // 4):
            if bx <= 2 and bz <= 1:
                continue                                         # the probe's corner (below)
            x, z = min(4 * bx + bz % 4, X - 1), min(4 * bz + bx % 4, Z - 1)
            y = min(4 * isob + (bx + 2 * bz) % 4 + 4 * ((bx + bz) % 2), Y - 1)
            col[z, y, x] = (0.5, 0.25, 0.75, values[k % len(values)])           # an isolated voxel keeps a colour: alpha decides whether it shows
            iso.append((z, y, x))
            ye = yb + (bx + bz) % 4
            col[z, ye, x, 3] = values[(k + 1) % len(values)]
            emb.append((z, ye, x))
            k += 1
    # the probe: a lone voxel of smoke in the empty layer under the top one, in the corner the class voxels above leave free, with one class
    # voxel as its +x neighbour.  With a light probe set, the lit voxel's occlusion ray runs against its density gradient, or along its
    # position where the gradient is exactly 0 (CSRayMarchL.hlsl:61-64): the one place where a subnormal alpha decides more than a last bit
    # (x = 4, z = 2 and, on 18 x 18 x 10, y = 13: a voxel whose centre's texel coordinate comes out exact there too -- 4.5 / 18 = 0.25 --, so
    # that the six samples of the gradient are single taps on every fresh grid)
    yp = 4 * isob - 3
    col[2, yp, 4] = (0.75, 0.5, 0.25, 0.875)
    col[2, yp, 5, 3] = values[-1]
    without = col.copy()
    without[..., 3][class_mask(col[..., 3], name)] = 0.0
    iso, emb = np.array(iso), np.array(emb)
    got_iso, got_emb = index_lists(col[..., 3], name)
    as_set = lambda v: set(map(tuple, v.tolist()))
    what = "%s %s%s: " % (name, dims, " (a step follows)" if stepped else "")
    cond = [(what + "isolated voxels", float(len(as_set(iso) & as_set(got_iso))), ">=", 8.0),
            (what + "isolated voxels by construction that the field does not show isolated", float(len(as_set(iso) - as_set(got_iso))), "==", 0.0),
            (what + "dim-embedded voxels", float(len(as_set(emb) & as_set(got_emb))), ">=", 8.0),
            (what + "dim-embedded voxels by construction that the field does not show embedded", float(len(as_set(emb) - as_set(got_emb))), "==", 0.0),
            (what + "class voxels", float(class_mask(col[..., 3], name).sum()), "==", float(len(iso) + len(emb) + 1)),
            (what + "values binary16 does not hold", float(0 if CLASSES[name][1] else (bits(to_half(col)) != bits(col)).sum()), "==", 0.0)]
    return case(dims=dims, name=name, col=col, without=without, isolated=iso, embedded=emb, conditions=cond)


def stepped_model(c, half):
    """the colour field one semi-Lagrangian step at rest turns c.col into (velocity 0, impulse off, dt = STEP_DT): the model of what the
    device's advection stores -- the GPU test asserts its conditions on the device's own array, not on this one"""
    X, Y, Z = c.dims
    vel = np.zeros((3, Z, Y, X), f32)
    with np.errstate(all="ignore"):
        return mr.step(vel, c.col, STEP_DT, "clamp", impulse=False, half=half, scheme="semi-lagrangian")[1]


def stepped_conditions(alpha, c):
    """on a stepped field: the class is still there -- >= 8 isolated and >= 8 dim-embedded voxels (-0: none is left)"""
    what = "%s %s behind a step: " % (c.name, c.dims)
    if c.name == "negzero":
        # no -0 passes the advection: its filter is lerp(a, b, f) = fma(f, b - a, a), and between zeros b - a = +0, fma(f, +0, -0) = +0.
        # The case stays -- a field of +0 where the -0 were -- and says so
        return [(what + "alphas that are -0", float((bits(alpha) == 0x80000000).sum()), "==", 0.0)]
    iso, emb = index_lists(alpha, c.name, stepped=True)
    return [(what + "isolated voxels", float(len(iso)), ">=", 8.0), (what + "dim-embedded voxels", float(len(emb)), ">=", 8.0)]


# ---- part 2: the colour channels -----------------------------------------------------------------------------------------------------------
RGB_VALUES = (-0.5, -300.0, 1.5, 40.0, 65504.0, np.inf, 2.0 ** -24, 2.0 ** -16, -0.0, -(2.0 ** -20))


@functools.lru_cache(maxsize=None)
def colour_field(dims):
    """ordinary alpha -- a body of [0.05, 0.9] in the lower two thirds, +0 above --, every third voxel of the body with one rgb channel from
    RGB_VALUES.  2-D grids (the visualiser): the same over the whole plane"""
    X, Y, Z = dims
    rng = np.random.default_rng(9300 + X + 7 * Z)
    col = np.zeros((Z, Y, X, 4), f32)
    yb = Y if Z == 1 else 2 * Y // 3
    col[:, :yb, :, :3] = to_half(rng.random((Z, yb, X, 3)))
    col[:, :yb, :, 3] = to_half(0.05 + 0.85 * rng.random((Z, yb, X)))
    z, y, x = np.meshgrid(np.arange(Z), np.arange(yb), np.arange(X), indexing="ij")
    n = x + 5 * y + 11 * z
    pick = n % 3 == 0
    vals = np.array(RGB_VALUES, f32)[(n // 3) % len(RGB_VALUES)]
    for ch in range(3):
        sel = pick & ((n // 3) % 3 == ch)
        col[:, :yb, :, ch][sel] = vals[sel]
    rgb = col[..., :3]
    what = "colour field %s: " % (dims,)
    with np.errstate(invalid="ignore"):
        cond = [(what + "negative rgb", float((rgb < 0).sum()), ">=", 8.0), (what + "rgb above 1", float(((rgb > 1) & np.isfinite(rgb)).sum()), ">=", 8.0),
                (what + "rgb 65504", float((rgb == 65504).sum()), ">=", 8.0), (what + "rgb +inf", float(np.isposinf(rgb).sum()), ">=", 8.0),
                (what + "rgb binary16 subnormal", float(((np.abs(rgb) > 0) & (np.abs(rgb) < 2.0 ** -14)).sum()), ">=", 8.0),
                (what + "rgb -0", float((bits(rgb) == 0x80000000).sum()), ">=", 8.0),
                (what + "alpha outside {0} u [0.05, 0.9]", float(((col[..., 3] != 0) & ((col[..., 3] < f32(0.0499)) | (col[..., 3] > f32(0.9)))).sum()), "==", 0.0),
                (what + "values binary16 does not hold", float((bits(to_half(col)) != bits(col)).sum()), "==", 0.0)]
    return case(dims=dims, col=col, conditions=cond)


# ---- part 3: the packer --------------------------------------------------------------------------------------------------------------------
def plain_pack(v, m):
    """an unsigned float of 5 exponent bits (bias 15) and m mantissa bits from the format's definition: the finite code nearest to v, ties
    to the even code; what lies at or beyond half an ulp above the largest finite code stays the largest finite code; negative -> 0"""
    if np.isnan(v):
        return (31 << m) | 1
    if v <= 0:
        return 0
    if np.isinf(v):
        return 31 << m
    value = lambda c: Fraction(c, 1 << (14 + m)) if c < (2 << m) else Fraction((1 << m) + (c & ((1 << m) - 1))) * Fraction(2) ** ((c >> m) - 15 - m)
    q, top = Fraction(float(v)), (31 << m) - 1
    lo = max(c for c in range(top + 1) if value(c) <= q)
    if lo == top or q - value(lo) < value(lo + 1) - q:
        return lo
    return lo + 1 if q - value(lo) > value(lo + 1) - q or lo & 1 else lo


def plain_pack3(r, g, b):
    return plain_pack(r, 6) | (plain_pack(g, 6) << 11) | (plain_pack(b, 5) << 22)


def packer_values(m):
    """(branch, value) for a channel of m mantissa bits"""
    s = 2.0 ** -(14 + m)                                         # the smallest subnormal code = one ulp up to 2^-13
    top = 65536.0 - 2.0 ** (15 - m)                              # the largest finite code
    return [("zero", 0.0), ("smallest subnormal", s), ("tie below the smallest subnormal", s / 2), ("tie above the smallest subnormal", 1.5 * s),
            ("seam - 1 ulp", 2.0 ** -14 - s), ("seam", 2.0 ** -14), ("seam + 1 ulp", 2.0 ** -14 + s),
            ("tie to even", 1.0 + 2.0 ** -(m + 1)), ("tie to odd", 1.0 + 3 * 2.0 ** -(m + 1)), ("largest finite", top),
            ("first past the largest finite", top + 2.0 ** (14 - m)), ("above 65536", 1.0e5), ("ordinary", 3.0 * np.pi)]


def light_value(color, ambient):
    """fx_march.h light_value on an empty voxel without a light probe (shadow = 1): fmaf(1, color.w * color[a], ambient.w * ambient[a])"""
    c, a = np.asarray(color, f32), np.asarray(ambient, f32)
    return er.fma(f32(1.0), c[3] * c[:3], a[3] * a[:3])


@functools.lru_cache(maxsize=None)
def packer_lights():
    """[(what, colour (r, g, b, intensity), ambient (r, g, b, intensity), expected float32[3])]: red runs through the list of the 6-bit
    channels forwards, green backwards, blue through the 5-bit list.  Every second entry puts the value together from colour and ambient
    (the two halves are binary fractions: the sum is exact), the others from the colour alone"""
    v6, v5 = packer_values(6), packer_values(5)
    out = []
    for k in range(len(v6)):
        want = np.array([v6[k][1], v6[-1 - k][1], v5[k][1]], f32)
        if k % 2:
            half = (want * f32(0.5)).astype(f32)
            color, ambient = (float(half[0]), float(half[1]), float(half[2]), 1.0), (float(want[0] - half[0]), float(want[1] - half[1]), float(want[2] - half[2]), 1.0)
        else:
            color, ambient = (float(want[0]) / 2, float(want[1]) / 2, float(want[2]) / 2, 2.0), (0.0, 0.0, 0.0, 0.0)
        out.append(("%s | %s | %s" % (v6[k][0], v6[-1 - k][0], v5[k][0]), color, ambient, want))
    return out
