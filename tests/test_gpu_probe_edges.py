"""The light probe's path off its happy path, BIT FOR BIT against the oracle -- there is no tolerance in this file.

k_bc6h_decode and the container walk behind fx_dds_decode_cube (fx_bc6h.hip, fx_api.cpp) have been compared with the oracle on cubes whose
edge is a multiple of 4 and on files of one mip; k_sh_cubemap / k_sh_sum / k_sh_normalize (fx_sh.hip) on powers of two with radiance in
[0, 4) and a tolerance of 1e-5.  Here, on the inputs of tests/probe_edges.py:

  part 1  decode: the clip of partial blocks (n = 34 with every mode x partition; n = 1, 2, 3, 5, 6, 10) after a larger cube has been through
          the same staging buffer; every mip of a chain 32 .. 1 and the refusals around it; the uncompressed formats at n = 5, 2, 1 with the
          binary16 classes and 0 / 255
  part 2  SH: every size at which the kernels take another path, every value class (HDR peak, +0, -0, fp32 subnormals, NaN and inf), one
          context reused across sizes, the refusals, and Init(<dds>) + TransformSH end to end

fx_sh.hip promises the oracle's fp32 sums -- the same pairing, uncontracted, denormals kept, IEEE division and square root --, so a word
that differs is a finding; where the oracle has a NaN the device must have one, and every other word is equal.  What the oracle is held to
without a GPU is in tests/test_probe_edges.py."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi
from oracle import orc

import probe_edges as pe
from probe_edges import bits

pytestmark = pytest.mark.gpu


def fluid():
    f = fx.Fluid()
    assert f.Init(64, 64, (16, 16, 16)), f.last_status
    return f


def probe():
    return fx.LightProbe(fluid())


def explain(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    return "%d of %d differ; first at %s: got %r (%#x) want %r (%#x)" % (len(bad), got.size, i, got[i], bits(got)[i], want[i], bits(want)[i])


def assert_same(got, want, what=""):
    """equal words; where the oracle has a NaN, a NaN"""
    assert got is not None and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]), (what, explain(got, want))


def sh_on(p, cube):
    assert p.Init(cube)
    p.TransformSH()
    return p.GetSH().copy()


# ---- part 1: decode -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def larger_cube():
    """40 x 40 of random blocks: more staging than any cube below needs, all of it written"""
    return pe.bc6h_cube_dds(40, [np.random.default_rng(11).integers(0, 256, (6, 100, 16), dtype=np.uint8)])


@pytest.mark.parametrize("n", [pe.GRID_EDGE] + pe.PARTIAL_EDGES)
def test_partial_blocks_are_clipped(n, larger_cube):
    """the last block row and column keep 1, 2 or 3 texels of 4; what the staging buffer held before does not show"""
    dds = pe.grid_cube() if n == pe.GRID_EDGE else pe.partial_cube(n)
    want, hist = orc.dds_bc6h_cube(dds, 0)
    if n == pe.GRID_EDGE:
        assert (hist > 0).all()
    p = probe()
    assert p.decode_dds(larger_cube).shape == (6, 40, 40, 3)
    assert_same(p.decode_dds(dds), want, n)
    assert_same(probe().decode_dds(dds), want, (n, "fresh context"))


def test_every_mip_of_a_chain_decodes():
    dds = pe.chain_cube()
    size, mips = C.c_uint32(), C.c_uint32()
    assert capi.load().fx_dds_cube_info(dds, len(dds), C.byref(size), C.byref(mips)) == capi.FX_OK
    assert (size.value, mips.value) == (pe.CHAIN_EDGE, pe.CHAIN_MIPS) == (32, 6)
    p = probe()
    for m in range(pe.CHAIN_MIPS):
        assert_same(p.decode_dds(dds, mip=m), orc.dds_bc6h_cube(dds, m)[0], m)
    for m in reversed(range(pe.CHAIN_MIPS)):                              # small after large: the staging buffer is not cleared in between
        assert_same(p.decode_dds(dds, mip=m), orc.dds_bc6h_cube(dds, m)[0], m)
    assert p.decode_dds(dds, mip=pe.CHAIN_MIPS) is None


def test_chain_headers_at_their_limits():
    dds = pe.chain_cube()
    p = probe()

    def with_mips(k):
        b = bytearray(dds)
        b[pe.HEADER_MIPS:pe.HEADER_MIPS + 4] = int(k).to_bytes(4, "little")
        return bytes(b)

    one = with_mips(0)                                                    # a mip count of 0 reads as one mip: the faces follow each other directly
    assert_same(p.decode_dds(one), orc.dds_bc6h_cube(one, 0)[0])
    assert p.decode_dds(one, mip=1) is None
    assert p.decode_dds(with_mips(7)) is None                             # 32 >> 6 = 0: no such level
    assert p.decode_dds(dds[:-16]) is None                                # the last block cut off
    assert p.decode_dds(dds[:-1]) is None
    f = p._fluid
    out = np.full(6 * 32 * 32 * 3 + 1, 7.0, np.float32)
    ptr = out.ctypes.data_as(C.POINTER(C.c_float))
    for floats in (out.size, out.size - 2):                               # out_floats one off either way
        assert f._lib.fx_dds_decode_cube(f._ctx, dds, len(dds), 0, ptr, floats) == capi.FX_E_INVALID
    assert (out == 7.0).all()
    assert f._lib.fx_dds_decode_cube(f._ctx, dds, len(dds), 0, ptr, out.size - 1) == capi.FX_OK
    assert_same(out[:-1].reshape(6, 32, 32, 3), orc.dds_bc6h_cube(dds, 0)[0])


def float_chain(rng, scale):
    """float32 rgb at n = 5, 2, 1 with -0, a subnormal, both infinities and two NaN payloads among random values"""
    special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC01234, 0x7FA00001], np.uint32).view(np.float32)
    chain = []
    for e in pe.mip_edges(5, 3):
        c = (rng.random((6, e, e, 3)) * scale).astype(np.float32)
        c.reshape(-1)[::5][:len(special)] = special[:len(c.reshape(-1)[::5])]
        chain.append(c)
    return chain


@pytest.mark.parametrize("fmt,legacy", [("rgba32f", False), ("rgb32f", False), ("rgba16f", False), ("rgba8", False), ("rgba16f", True), ("rgba32f", True)])
def test_uncompressed_cubes_of_odd_edge_carry_every_value_class(fmt, legacy):
    """n = 5 with mips 5, 2, 1 (max(n >> m, 1): no level is half the one above it)"""
    rng = np.random.default_rng(12)
    if fmt == "rgba16f":
        chain = list(pe.half_class_chain())
        want = [pe.half_bits_to_f32_bits(c[..., :3]) for c in chain]      # numpy's float16 -> float32; NaN payloads shifted into place
    elif fmt == "rgba8":
        chain = [rng.integers(0, 256, (6, e, e, 4), dtype=np.uint8) for e in pe.mip_edges(5, 3)]
        for c in chain:
            c[0, 0, 0, :3], c[5, -1, -1, :3] = (0, 255, 0), (255, 0, 255)
        want = [bits(c[..., :3].astype(np.float32) / np.float32(255)) for c in chain]
        assert want[2][0, 0, 0, 1] == bits(np.float32(1)) and want[2][0, 0, 0, 0] == 0
    else:
        chain = float_chain(rng, 4.0)
        want = [bits(c) for c in chain]
    dds = pe.linear_cube_dds(chain, fmt, legacy=legacy)
    p = probe()
    for m, w in enumerate(want):
        got = p.decode_dds(dds, mip=m)
        assert got is not None and got.shape == w.shape and np.array_equal(bits(got), w), (fmt, m, explain(got, w.view(np.float32)))
    assert p.decode_dds(dds, mip=3) is None
    assert p.decode_dds(dds[:-1]) is None


# ---- part 2: SH -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(pe.SH_SIZES))
def test_sh_equals_oracle_at_every_size(n):
    cube = pe.sh_cube(n)
    assert_same(sh_on(probe(), cube), orc.sh_transform(cube), (n, pe.SH_SIZES[n]))


@pytest.mark.parametrize("kind", pe.SH_VALUES)
@pytest.mark.parametrize("n", pe.SH_VALUE_SIZES)
def test_sh_equals_oracle_on_every_value_class(n, kind):
    cube = pe.sh_cube(n, kind)
    want = orc.sh_transform(cube)
    got = sh_on(probe(), cube)
    if kind in ("zero", "negzero"):
        assert not bits(want).any() and not bits(got).any()               # 27 words of +0
    if kind == "subnormal":
        assert want.all() and (np.abs(want) < np.finfo(np.float32).tiny).all()          # a kernel that flushed would return zeros
    if kind == "nonfinite":
        assert np.isnan(want[:, pe.NAN_TEXEL[3]]).all() and np.isinf(want[:, pe.INF_TEXEL[3]]).all() and np.isfinite(want[:, 1]).all()
    assert_same(got, want, (n, kind))


def test_sh_on_a_reused_context():
    """the scratch buffers are reallocated when the size changes, and the staging buffer is the decoder's too"""
    fresh = {n: sh_on(probe(), pe.sh_cube(n)) for n in (20, 3, 75)}
    p = probe()
    for k, n in enumerate((20, 3, 75, 3, 20)):
        if k == 3:
            assert_same(p.decode_dds(pe.grid_cube()), orc.dds_bc6h_cube(pe.grid_cube(), 0)[0])
        assert_same(sh_on(p, pe.sh_cube(n)), fresh[n], (k, n))
        assert_same(fresh[n], orc.sh_transform(pe.sh_cube(n)), n)


def test_sh_refuses_sizes_outside_its_range():
    """n = 0 and n = 4097 are refused before anything is read or allocated: the cube handed over is one texel"""
    p = probe()
    f = p._fluid
    want = sh_on(p, pe.sh_cube(3))
    cube = np.ones((6, 1, 1, 3), np.float32)
    out = np.full(27, 7.0, np.float32)
    fp = C.POINTER(C.c_float)
    for n in (0, 4097):
        assert f._lib.fx_sh_transform(f._ctx, cube.ctypes.data_as(fp), n, out.ctypes.data_as(fp)) == capi.FX_E_INVALID
    assert (out == 7.0).all()
    assert_same(sh_on(p, pe.sh_cube(3)), want)                            # and the context is as it was


@pytest.mark.parametrize("mip", [0, 3, 5])
def test_probe_from_a_chain_mip_end_to_end(mip):
    """LightProbe.Init(<dds bytes>, mip) + TransformSH = the oracle's SH of the oracle's decode, at n = 32, 4, 1"""
    dds = pe.chain_cube()
    cube = orc.dds_bc6h_cube(dds, mip)[0]
    assert cube.shape[1] == 32 >> mip
    p = probe()
    assert p.Init(dds, mip=mip)
    p.TransformSH()
    assert_same(p.GetSH(), orc.sh_transform(cube), mip)
