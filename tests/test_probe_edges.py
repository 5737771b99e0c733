"""The premises of tests/test_gpu_probe_edges.py without a GPU: the oracle's BC6H decoder against an independent one, the recipes of
tests/probe_edges.py against their own conditions, and the oracle's SH projection and container walk against plain restatements.

  part 1  orc.bc6h_decode_blocks against Pillow's decoder as recorded in tests/golden/bc6h_independent.npz (written by
          tools/make_bc6h_independent_golden.py; Pillow is not imported here): 8 bits, values below 1, every mode and partition
  part 2  the recipes: clipped blocks that matter, block counts of the chain, subnormal partial sums, the binary16 classes
  part 3  orc.sh_transform against the float64 model, and what a NaN or an inf texel may poison
  part 4  orc.dds_bc6h_cube against blocks decoded one by one and put in place by hand"""
import os

import numpy as np
import pytest

import probe_edges as pe
from oracle import orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HALF_STEP_BELOW_ONE = 1.0 - 2.0 ** -11                       # the binary16 before 1


# ---- part 1: the independent decoder ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pin():
    fix = np.load(os.path.join(GOLD, "bc6h_independent.npz"))
    blocks, rgb8 = fix["blocks"], fix["rgb8"]
    halves, modes = orc.bc6h_decode_blocks(blocks)
    return dict(blocks=blocks, rgb8=rgb8.astype(int), value=pe.half_bits_as_f32(halves), modes=modes, cap=4 * float(fix["differing_share"]))


def test_independent_fixture_is_the_recipe_and_covers_every_mode_and_partition(pin):
    assert np.array_equal(pin["blocks"], pe.independent_blocks())          # the fixture was made from the committed recipe
    assert np.array_equal(pin["modes"], pe.block_mode(pin["blocks"]))
    modes, part = pin["modes"], pe.block_partition(pin["blocks"])
    hist = np.zeros((11, 32), int)
    two = (modes >= 1) & (modes <= 10)
    np.add.at(hist, (modes[two], part[two]), 1)
    assert (hist[1:] > 0).all(), np.argwhere(hist[1:] == 0)
    assert all((modes == m).sum() >= pe.GRID_FEW for m in (0, 11, 12, 13, 14))
    assert 0 < pin["cap"] < 0.02                                           # a structural error moves whole blocks: far more than this


@pytest.mark.parametrize("mode", range(15))
def test_oracle_bc6h_agrees_with_the_independent_decoder(pin, mode):
    sel = pin["modes"] == mode
    v, theirs = pin["value"][sel], pin["rgb8"][sel]
    ours = pe.to_8bit(v).astype(int)
    step = np.abs(ours - theirs)
    share, inside = float((step > 0).mean()), float(((v > 0) & (v < 1)).mean())
    print("mode %d: %d blocks, largest difference %d, differing share %.2e (cap %.2e), inside (0, 1) %.2f" % (mode, sel.sum(), step.max(), share, pin["cap"], inside))
    assert step.max() <= 1
    assert (theirs[v >= 1] == 255).all()
    assert (v[theirs == 255] >= HALF_STEP_BELOW_ONE).all()
    assert share <= pin["cap"]
    if mode:
        assert inside > 0.25                                               # where 8 bits still carry information
    else:
        assert not v.any() and not theirs.any()                            # the reserved modes are black in both


# ---- part 2: the recipes ------------------------------------------------------------------------------------------------------------------
def test_grid_cube_has_clipped_blocks_whose_dropped_texels_differ():
    blocks = pe.grid_cube_blocks()
    flat = blocks.reshape(-1, 16)
    grid = pe.mode_partition_blocks()
    assert {b.tobytes() for b in grid} <= {b.tobytes() for b in flat}      # the whole mode x partition grid is in the cube
    nb = (pe.GRID_EDGE + 3) // 4
    assert nb == 9 and pe.GRID_EDGE - 4 * (nb - 1) == 2
    differ = modes_seen = 0
    for f in range(6):
        halves, modes = orc.bc6h_decode_blocks(blocks[f])
        tex = halves.reshape(nb, nb, 4, 4, 3)
        edge = [(by, bx) for by in range(nb) for bx in range(nb) if by == nb - 1 or bx == nb - 1]
        assert len(edge) == 17
        for by, bx in edge:
            keep = np.zeros((4, 4), bool)
            keep[:2 if by == nb - 1 else 4, :2 if bx == nb - 1 else 4] = True
            t = tex[by, bx]
            # a decoder that wrote the dropped texels would write something else than what belongs there
            differ += not {tuple(p) for p in t[~keep]} <= {tuple(p) for p in t[keep]}
        modes_seen |= int(sum(1 << m for m in modes.reshape(nb, nb)[[by for by, _ in edge], [bx for _, bx in edge]]))
    assert differ >= 6 * 12, differ
    assert bin(modes_seen).count("1") >= 10                                # the clipped blocks are a mix of modes


def test_chain_and_partial_cubes_have_the_block_counts_of_their_sizes():
    chain = pe.chain_blocks()
    assert len(chain) == pe.CHAIN_MIPS == 6 and pe.mip_edges(pe.CHAIN_EDGE, 6) == [32, 16, 8, 4, 2, 1]
    for m, c in enumerate(chain):
        assert c.shape == (6, max(1, (pe.CHAIN_EDGE >> m) // 4) ** 2, 16)
    assert len({c.tobytes()[:96] for c in chain}) == 6                     # a seed per mip: a wrong mip offset reads other blocks
    assert len(pe.chain_cube()) == 148 + 6 * 16 * (64 + 16 + 4 + 1 + 1 + 1)
    for n in pe.PARTIAL_EDGES:
        assert len(pe.partial_cube(n)) == 148 + 6 * 16 * ((n + 3) // 4) ** 2 and n % 4
    assert len(pe.grid_cube()) == 148 + 6 * 16 * 81


def test_half_classes_reach_every_channel_of_the_top_mip():
    chain = pe.half_class_chain()
    assert [c.shape for c in chain] == [(6, 5, 5, 4), (6, 2, 2, 4), (6, 1, 1, 4)]
    for ch in range(3):
        assert set(chain[0][..., ch].ravel()) == set(pe.HALF_CLASSES.values())
    want = pe.half_bits_to_f32_bits(np.array(list(pe.HALF_CLASSES.values()), np.uint16))
    named = dict(zip(pe.HALF_CLASSES, want))
    assert named["smallest subnormal"] == np.float32(2.0 ** -24).view(np.uint32) and named["65504"] == np.float32(65504).view(np.uint32)
    assert named["-0"] == 0x80000000 and named["-inf"] == 0xFF800000
    assert named["quiet NaN"] == 0x7FC02000 and named["signalling NaN"] == 0x7FAAA000      # payloads in place, the signalling one not quieted
    for name, b in pe.HALF_CLASSES.items():                               # the oracle's own conversion agrees on the numbers
        if "NaN" not in name:
            assert np.float32(orc.lib().orc_f16_to_f32(b)).view(np.uint32) == named[name], name


@pytest.mark.parametrize("n", pe.SH_VALUE_SIZES)
def test_subnormal_recipe_makes_subnormal_partial_sums_and_a_nonzero_result(n):
    cube = pe.sh_cube(n, "subnormal")
    tiny = float(np.finfo(np.float32).tiny)
    assert 0 < cube.min() and cube.max() <= 1.0000001e-38
    w, terms = pe.sh_terms64(cube)
    total = 6 * n * n
    padded = np.zeros(((total + 31) // 32 * 32, 9, 3))
    padded[:total] = terms
    partial = np.abs(padded.reshape(-1, 32, 9, 3).sum(axis=1))             # what k_sh_cubemap stores, to fp32 rounding
    print("N %d: subnormal share of the products %.2f, of the 32-texel partial sums %.2f" % (n, (np.abs(terms) < tiny).mean(), (partial < tiny).mean()))
    # the products are subnormal but for the brightest texels; 32 of them add up to a normal number in the coefficients that do not cancel
    # (L00 first) and stay subnormal in the others -- both kinds of partial sum are there
    assert (np.abs(terms) < tiny).mean() > 0.9 and (terms != 0).mean() > 0.9
    assert 0.25 < ((partial < tiny) & (partial > 0)).mean() < 0.75
    got = orc.sh_transform(cube)
    assert (got != 0).all() and (np.abs(got) < tiny).all()                 # every coefficient is itself a subnormal: nothing a flush would keep
    flushed = orc.sh_transform(np.where(cube < tiny, 0, cube).astype(np.float32))
    assert not np.array_equal(pe.bits(flushed), pe.bits(got))


# ---- part 3: the oracle's SH against float64 ------------------------------------------------------------------------------------------------
def test_sh_size_list_takes_the_paths_it_names():
    assert list(pe.SH_SIZES) == [1, 2, 3, 5, 7, 20, 33, 75]
    assert pe.sh_passes(1) == [6, 1] and pe.sh_passes(2) == [24, 1] and pe.sh_passes(3) == [54, 2, 1]
    assert pe.sh_passes(5) == [150, 5, 1] and pe.sh_passes(7) == [294, 10, 1] and pe.sh_passes(20) == [2400, 75, 3, 1]
    assert pe.sh_passes(33) == [6534, 205, 7, 1] and pe.sh_passes(75) == [33750, 1055, 33, 2, 1]
    assert all(len(pe.sh_passes(n)) < 5 for n in range(1, 74))             # three sum passes begin at N = 74 (more than 1024 groups)
    assert all(6 * n * n % 32 for n in (1, 2, 3, 5, 7, 33, 75)) and 6534 % 256 and (6534 + 31) // 32 % 8


CASES = [(n, "random") for n in pe.SH_SIZES] + [(n, k) for n in pe.SH_VALUE_SIZES for k in pe.SH_FINITE if k != "random"]


@pytest.mark.parametrize("n,kind", CASES)
def test_oracle_sh_equals_the_float64_model(n, kind):
    cube = pe.sh_cube(n, kind)
    got, want = orc.sh_transform(cube), pe.sh_model64(cube)
    if kind in ("zero", "negzero"):
        assert not want.any() and not pe.bits(got).any()                   # 27 words of +0, from -0 radiance too
        return
    err = pe.sh_error(got, want)
    print("N %d %s: error %.2e of the largest coefficient (bar %.2e)" % (n, kind, err, pe.SH_ORACLE_ERROR_BAR))
    assert err <= pe.SH_ORACLE_ERROR_BAR
    if kind == "peak":
        assert np.isfinite(got).all() and got[0].min() > 10


@pytest.mark.parametrize("poison", ["nan", "inf", "both"])
@pytest.mark.parametrize("n", pe.SH_VALUE_SIZES)
def test_a_nonfinite_texel_poisons_its_own_colour_channel_only(n, poison):
    cube = pe.sh_cube(n, "nonfinite", poison)
    assert pe.NAN_TEXEL[0] != pe.INF_TEXEL[0] and pe.NAN_TEXEL[3] != pe.INF_TEXEL[3]
    got = orc.sh_transform(cube)
    clean = orc.sh_transform(np.where(np.isfinite(cube), cube, 0).astype(np.float32))
    bad = {"nan": [pe.NAN_TEXEL[3]], "inf": [pe.INF_TEXEL[3]], "both": [pe.NAN_TEXEL[3], pe.INF_TEXEL[3]]}[poison]
    for ch in range(3):
        if ch in bad:
            assert not np.isfinite(got[:, ch]).any(), (ch, got[:, ch])
        else:
            assert np.array_equal(pe.bits(got[:, ch]), pe.bits(clean[:, ch])), ch
    if poison != "inf":
        assert np.isnan(got[:, pe.NAN_TEXEL[3]]).all()
    if poison != "nan":
        assert np.isinf(got[:, pe.INF_TEXEL[3]]).all()                     # one inf term and finite others: +-inf by the basis function's sign


# ---- part 4: the oracle's container walk ----------------------------------------------------------------------------------------------------
def by_hand(blocks, n):
    """[6][blocks][16] -> float32[6][n][n][3] and the mode histogram, block by block"""
    faces, hist = [], np.zeros(15, int)
    for f in range(6):
        halves, modes = orc.bc6h_decode_blocks(blocks[f])
        faces.append(pe.half_bits_as_f32(pe.assemble_face(halves, n)))
        hist += np.bincount(modes, minlength=15)
    return np.stack(faces), hist


def test_oracle_cube_walk_clips_the_grid_cube_like_blocks_put_in_place_by_hand():
    want, hist = by_hand(pe.grid_cube_blocks(), pe.GRID_EDGE)
    got, got_hist = orc.dds_bc6h_cube(pe.grid_cube(), 0)
    assert got.shape == (6, 34, 34, 3) and np.array_equal(pe.bits(got), pe.bits(want)) and np.array_equal(got_hist, hist)
    assert (hist > 0).all()


@pytest.mark.parametrize("n", pe.PARTIAL_EDGES)
def test_oracle_cube_walk_on_partial_blocks(n):
    want, _ = by_hand(pe.partial_cube_blocks(n), n)
    got, _ = orc.dds_bc6h_cube(pe.partial_cube(n), 0)
    assert got.shape == (6, n, n, 3) and np.array_equal(pe.bits(got), pe.bits(want))


def test_oracle_cube_walk_finds_every_mip_of_the_chain():
    dds = pe.chain_cube()
    for m, blocks in enumerate(pe.chain_blocks()):
        n = pe.CHAIN_EDGE >> m
        want, _ = by_hand(blocks, n)
        got, _ = orc.dds_bc6h_cube(dds, m)
        assert got.shape == (6, n, n, 3) and np.array_equal(pe.bits(got), pe.bits(want)), m
    with pytest.raises(ValueError):
        orc.dds_bc6h_cube(dds, pe.CHAIN_MIPS)
    one = bytearray(dds)
    one[pe.HEADER_MIPS:pe.HEADER_MIPS + 4] = bytes(4)                      # a mip count of 0 reads as one mip: faces follow each other directly
    got, _ = orc.dds_bc6h_cube(bytes(one), 0)
    flat = np.frombuffer(dds, np.uint8)[148:148 + 6 * 64 * 16].reshape(6, 64, 16)
    assert np.array_equal(pe.bits(got), pe.bits(by_hand(flat, 32)[0]))
