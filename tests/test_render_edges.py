"""The recipes of tests/render_edges.py, held to their conditions on the oracle alone (no GPU): every class field has its isolated and its
dim-embedded voxels, the class takes part in the oracle's light volume and cube map (for -0: provably does not), the fields survive the step
that tests/test_gpu_render_edges.py puts in front of the side-volume kernels, and the packer list reaches every branch it names."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import render_edges as re_
from oracle import orc

f32 = np.float32
CLASS_CASES = [(d, n) for d in re_.FRESH_GRIDS for n in re_.CLASSES]


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def frame_of(dims):
    view, proj, eye = orc.default_camera(*re_.VP)
    fr, lod, rs, mask, _ = orc.update_frame(view, proj, eye, re_.VP[0], re_.VP[1], dims[0], re_.NS)
    return fr, lod, rs, mask


@functools.lru_cache(maxsize=None)
def oracle_render(dims, name, without, use_sh):
    """(light map, cube map) of the oracle for a class field, or for its copy with the class voxels at +0"""
    c = re_.class_field(dims, name)
    col = c.without if without else c.col
    fr, lod, rs, mask = frame_of(dims)
    for i, v in enumerate(re_.SH.reshape(27)):
        fr.sh[i] = v
    lm = orc.raymarch_light(col, fr, re_.NL, use_sh, 2)
    _, cu = orc.raymarch_view(col, lm, fr, dims[0] >> lod, mask, rs, re_.NL, use_sh, True)
    return lm, cu


@pytest.mark.parametrize("dims,name", CLASS_CASES, ids=ids)
def test_class_fields_meet_their_conditions(dims, name):
    c = re_.class_field(dims, name)
    re_.assert_conditions(c)
    # the lists the helper returns are lists of voxels of the class, and the field without the class differs in exactly those alphas
    alpha = c.col[..., 3]
    for v in np.concatenate([c.isolated, c.embedded]):
        assert re_.class_mask(alpha, name)[tuple(v)]
    changed = re_.bits(c.col) != re_.bits(c.without)
    assert not changed[..., :3].any() and np.array_equal(changed[..., 3], re_.class_mask(alpha, name) & (re_.bits(alpha) != 0))
    assert not re_.bits(c.without[..., 3])[re_.class_mask(alpha, name)].any()


@pytest.mark.parametrize("dims,name", CLASS_CASES, ids=ids)
def test_the_class_takes_part_in_the_oracle_render(dims, name):
    """light map and cube map with the class voxels against the same field with +0 in their place: they differ for every class but -0,
    and for -0 they are equal -- which is what makes skipping a block of -0 legal.  Without and with the light probe; the two subnormal classes show with the probe only"""
    c = re_.class_field(dims, name)
    for use_sh in (False, True):
        lm, cu = oracle_render(dims, name, False, use_sh)
        lm0, cu0 = oracle_render(dims, name, True, use_sh)
        words = int((re_.bits(lm) != re_.bits(lm0)).any(axis=-1).sum())
        texels = int((cu != cu0).any(axis=-1).sum())
        print("%s %s%s: %d isolated, %d dim-embedded voxels; %d light-map words and %d cube texels differ; %d words NaN-coded" %
              (name, dims, " with the light probe" if use_sh else "", len(c.isolated), len(c.embedded), words, texels, int(np.isnan(lm).any(axis=-1).sum())))
        assert cu0[..., 3].max() > 30                              # the body is seen
        if name == "negzero":
            assert words == 0 and texels == 0
        elif use_sh or name not in ("half_subnormal", "fp32_subnormal"):
            assert words >= 1 and texels >= 1
        # (a subnormal alpha changes no word through a ray -- fma(-d, 0.8, 1) is 1 or an ulp below --: without the probe there is nothing
        # to assert for the two subnormal classes; with it, the probe voxel's occlusion ray turns: render_edges.class_field)


@pytest.mark.parametrize("dims", re_.STEP_GRIDS, ids=ids)
@pytest.mark.parametrize("name", list(re_.CLASSES))
def test_class_fields_survive_the_step_at_rest(dims, name):
    """the model of the step (velocity 0, impulse off, dt = 2^-10) leaves >= 8 isolated and >= 8 dim-embedded voxels of the class (of -0: none, by the filter's arithmetic)"""
    c = re_.class_field(dims, name, True)
    re_.assert_conditions(c)
    for storage in re_.storages(name):
        col = re_.stepped_model(c, storage == "fp16")
        re_.assert_conditions(re_.case(conditions=re_.stepped_conditions(col[..., 3], c)))


@pytest.mark.parametrize("dims", [(32, 32, 32), (36, 36, 1)], ids=ids)
def test_colour_field_meets_its_conditions(dims):
    re_.assert_conditions(re_.colour_field(dims))


def test_the_packer_list_reaches_every_branch():
    """every entry on orc_pack_r11g11b10 against the plain packer, and per channel width the branch its name states"""
    lights = re_.packer_lights()
    assert len(lights) >= 12
    for what, color, ambient, want in lights:
        assert min(color) >= 0 and min(ambient) >= 0 and np.isfinite(color + ambient).all()      # what fx_set_light takes
        got = re_.light_value(color, ambient)
        assert re_.same_bits(got, want), what
        word = orc.lib().orc_pack_r11g11b10(float(want[0]), float(want[1]), float(want[2]))
        assert word == re_.plain_pack3(*want), (what, hex(word), hex(re_.plain_pack3(*want)))
    for m in (6, 5):
        v = dict(re_.packer_values(m))
        code = {k: re_.plain_pack(f32(x), m) for k, x in v.items()}
        s, one = Fraction(1, 1 << (14 + m)), 15 << m
        assert code["zero"] == 0 and code["smallest subnormal"] == 1
        assert Fraction(v["tie below the smallest subnormal"]) == s / 2 and code["tie below the smallest subnormal"] == 0      # RNE to 0
        assert Fraction(v["tie above the smallest subnormal"]) == 3 * s / 2 and code["tie above the smallest subnormal"] == 2  # RNE to 2
        assert (code["seam - 1 ulp"], code["seam"], code["seam + 1 ulp"]) == ((1 << m) - 1, 1 << m, (1 << m) + 1)
        assert code["tie to even"] == one and code["tie to odd"] == one + 2
        assert code["largest finite"] == (31 << m) - 1 and Fraction(v["largest finite"]) == Fraction(65536) - Fraction(1 << (15 - m))
        assert code["first past the largest finite"] == (31 << m) - 1 and code["above 65536"] == (31 << m) - 1
        assert v["above 65536"] > 65536
        # the device's packer has a subnormal branch below 2^-14 and a normal one from there on: both sides of the seam are in the list
        assert sum(0 < x < 2.0 ** -14 for x in v.values()) >= 4 and sum(x >= 2.0 ** -14 for x in v.values()) >= 7
    for v, m in ((np.nan, 6), (np.inf, 5), (-1.0, 6), (-0.0, 5)):
        w = orc.lib().orc_pack_r11g11b10(*(float(v) if m == 6 else 0.0,) * 2, float(v) if m == 5 else 0.0)
        assert w == (re_.plain_pack(v, 6) | (re_.plain_pack(v, 6) << 11) if m == 6 else re_.plain_pack(v, 5) << 22)
