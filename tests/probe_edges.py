"""Input recipes of tests/test_gpu_probe_edges.py: the light probe's path -- the DDS container and BC6H decode (csrc/fx_bc6h.hip,
fx_dds_decode_cube) and the SH projection (csrc/fx_sh.hip, fx_sh_transform) -- off the happy path of powers of two, one mip and radiance in
[0, 4).

  part 1  containers: a BC6H cube and an uncompressed cube of any edge and mip count, their headers written from scratch
  part 2  BC6H blocks: one for every two-region mode x partition, some for every one-region and reserved mode (the n = 34 cube, whose last
          block row and column are clipped to 2 texels), cubes of partial blocks only, one full mip chain 32 .. 1
  part 3  SH: the sizes at which k_sh_cubemap / k_sh_sum take another path, the value classes, and a float64 model without a tree
  part 4  the binary16 patterns an RGBA16F cube carries

tests/test_probe_edges.py holds the recipes and the oracle to their conditions without a GPU; the GPU test compares the kernels with the
oracle bit for bit.  Recipes are cached and read-only.  Nothing here imports the oracle or touches a GPU at import."""
import functools
import struct

import numpy as np

f32 = np.float32


def frozen(a):
    a.setflags(write=False)                                  # shared among tests: nobody changes a recipe
    return a


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- part 1: containers -------------------------------------------------------------------------------------------------------------------
DXGI = {"bc6h": 95, "rgba32f": 2, "rgb32f": 6, "rgba16f": 10, "rgba8": 28}
D3DFMT = {"rgba16f": 113, "rgba32f": 116}                    # legacy FourCC codes (D3DFMT_A16B16G16R16F, D3DFMT_A32B32G32R32F)
HEADER_MIPS = 28                                             # byte offset of dwMipMapCount


def mip_edges(n, mips):
    return [max(n >> m, 1) for m in range(mips)]


def dds_header(n, mips, fmt, top_bytes, cube=True, legacy=False):
    """magic + DDS_HEADER (+ DDS_HEADER_DXT10) of an n x n texture with `mips` levels, as the DirectX documentation lays them out"""
    h = bytearray(128)
    h[0:4] = b"DDS "
    flags = 0x1007 | 0x80000 | (0x20000 if mips > 1 else 0)  # CAPS | HEIGHT | WIDTH | PIXELFORMAT | LINEARSIZE (| MIPMAPCOUNT)
    struct.pack_into("<IIIIIII", h, 4, 124, flags, n, n, top_bytes, 0, mips)
    struct.pack_into("<II", h, 76, 32, 4)                    # DDS_PIXELFORMAT: size, DDPF_FOURCC
    caps = 0x1000 | (0x8 if cube or mips > 1 else 0) | (0x400000 if mips > 1 else 0)    # TEXTURE (| COMPLEX) (| MIPMAP)
    struct.pack_into("<II", h, 108, caps, 0xFE00 if cube else 0)                        # caps2: CUBEMAP, all six faces
    if legacy:
        struct.pack_into("<I", h, 84, D3DFMT[fmt])
        return bytes(h)
    h[84:88] = b"DX10"
    return bytes(h) + struct.pack("<IIIII", DXGI[fmt], 3, 4 if cube else 0, 1, 0)       # format, TEXTURE2D, TEXTURECUBE, array size, misc2


def bc6h_blocks_per_mip(n, mips):
    return [((e + 3) // 4) ** 2 for e in mip_edges(n, mips)]


def bc6h_cube_dds(n, chain):
    """a DDS cube map in BC6H_UF16 of edge n; chain[m] = uint8[6][blocks of mip m][16], blocks row-major, ((n >> m) + 3) / 4 a side"""
    mips = len(chain)
    chain = [np.ascontiguousarray(c, np.uint8) for c in chain]
    for c, nb in zip(chain, bc6h_blocks_per_mip(n, mips)):
        assert c.shape == (6, nb, 16), (c.shape, nb)
    body = b"".join(c[f].tobytes() for f in range(6) for c in chain)                    # each face is followed by its mip chain
    return dds_header(n, mips, "bc6h", chain[0][0].size) + body


def bc6h_image_dds(blocks, bw, bh):
    """a plain 2-D BC6H_UF16 texture of bw x bh blocks (no cube, one mip): the form any DDS reader takes"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(bw * bh, 16)
    h = bytearray(dds_header(4 * bw, 1, "bc6h", blocks.size, cube=False))
    struct.pack_into("<II", h, 12, 4 * bh, 4 * bw)           # height, width
    return bytes(h) + blocks.tobytes()


def linear_cube_dds(chain, fmt, legacy=False):
    """a DDS cube map in an uncompressed format; chain[m] = [6][e][e][..] with e = max(n >> m, 1): float rgb (alpha becomes 1), or the
    stored texels themselves -- uint16[..][4] binary16 bit patterns for rgba16f, uint8[..][4] for rgba8"""
    n, mips = chain[0].shape[1], len(chain)
    assert [c.shape[:3] for c in chain] == [(6, e, e) for e in mip_edges(n, mips)]

    def enc(c):
        if fmt == "rgba16f" and c.dtype == np.uint16 or fmt == "rgba8" and c.dtype == np.uint8:
            assert c.shape[-1] == 4
            return c.astype("<u2" if fmt == "rgba16f" else np.uint8).tobytes()
        assert c.shape[-1] == 3
        rgba = np.concatenate([c, np.ones(c.shape[:-1] + (1,), f32)], axis=-1)
        if fmt == "rgba32f":
            return rgba.astype("<f4").tobytes()
        if fmt == "rgb32f":
            return c.astype("<f4").tobytes()
        if fmt == "rgba16f":
            return rgba.astype("<f2").tobytes()
        return np.rint(np.clip(rgba, 0, 1) * 255).astype(np.uint8).tobytes()

    body = [[enc(c[f]) for c in chain] for f in range(6)]
    return dds_header(n, mips, fmt, len(body[0][0]), legacy=legacy) + b"".join(b"".join(face) for face in body)


# ---- part 2: BC6H blocks ------------------------------------------------------------------------------------------------------------------
# the low block bits of the 14 modes in the order of the format's table (mode 1 .. 14); all two-region modes have an 82-bit header that
# ends in the partition d[4:0] at bits 77 .. 81 (then 46 index bits), the one-region modes a 65-bit one and no partition
TWO_REGION = [(2, 0x00), (2, 0x01), (5, 0x02), (5, 0x06), (5, 0x0A), (5, 0x0E), (5, 0x12), (5, 0x16), (5, 0x1A), (5, 0x1E)]
ONE_REGION = [(5, 0x03), (5, 0x07), (5, 0x0B), (5, 0x0F)]
RESERVED = [(5, 0x13), (5, 0x17), (5, 0x1B), (5, 0x1F)]
PARTITION_BIT = 77
GRID_EDGE = 34                                               # 9 x 9 blocks a face, the last row and column clipped to 2 texels
GRID_FEW = 8                                                 # blocks for each one-region and each reserved mode


def block_ints(blocks):
    return [int.from_bytes(b.tobytes(), "little") for b in np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)]


def block_mode(blocks):
    """mode 1 .. 14 in the order of the table, 0 = reserved: from the low bits alone"""
    table = {(nb, v): k + 1 for k, (nb, v) in enumerate(TWO_REGION + ONE_REGION)}
    return np.array([table.get((2, v & 3), table.get((5, v & 31), 0)) for v in block_ints(blocks)])


def block_partition(blocks):
    """bits 77 .. 81 (meaningful in the two-region modes 1 .. 10)"""
    return np.array([(v >> PARTITION_BIT) & 31 for v in block_ints(blocks)])


def forced_block(rng, mode, partition=None):
    """a random 128-bit payload with the mode bits (and the partition bits) forced"""
    v = int.from_bytes(rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), "little")
    nbits, value = mode
    v = (v & ~((1 << nbits) - 1)) | value
    if partition is not None:
        v = (v & ~(31 << PARTITION_BIT)) | (partition << PARTITION_BIT)
    return np.frombuffer(v.to_bytes(16, "little"), np.uint8)


@functools.lru_cache(None)
def mode_partition_blocks():
    """uint8[384][16]: 10 two-region modes x 32 partitions, then GRID_FEW for each one-region mode, then GRID_FEW for each reserved value"""
    rng = np.random.default_rng(6001)
    out = [forced_block(rng, m, p) for m in TWO_REGION for p in range(32)]
    out += [forced_block(rng, m) for m in ONE_REGION + RESERVED for _ in range(GRID_FEW)]
    return frozen(np.stack(out))


@functools.lru_cache(None)
def grid_cube_blocks():
    """uint8[6][81][16]: the mode x partition grid, then a second draw of two-region blocks up to 6 x 81, shuffled so that the clipped
    row and column of every face hold a mix of modes"""
    rng = np.random.default_rng(6002)
    grid = mode_partition_blocks()
    nb = ((GRID_EDGE + 3) // 4) ** 2
    more = [forced_block(rng, TWO_REGION[k % 10], int(rng.integers(0, 32))) for k in range(6 * nb - len(grid))]
    blocks = np.concatenate([grid, np.stack(more)])
    return frozen(blocks[rng.permutation(len(blocks))].reshape(6, nb, 16))


@functools.lru_cache(None)
def grid_cube():
    return bc6h_cube_dds(GRID_EDGE, [grid_cube_blocks()])


PARTIAL_EDGES = [1, 2, 3, 5, 6, 10]                          # one block clipped to 1, 2, 3 texels; 2 x 2 blocks clipped to 1 and 2; 3 x 3 to 2


@functools.lru_cache(None)
def partial_cube_blocks(n):
    return frozen(np.random.default_rng(6100 + n).integers(0, 256, (6, ((n + 3) // 4) ** 2, 16), dtype=np.uint8))


@functools.lru_cache(None)
def partial_cube(n):
    return bc6h_cube_dds(n, [partial_cube_blocks(n)])


CHAIN_EDGE, CHAIN_MIPS = 32, 6                               # 32, 16, 8, 4, 2, 1: 64, 16, 4, 1, 1, 1 blocks a face


@functools.lru_cache(None)
def chain_blocks():
    counts = bc6h_blocks_per_mip(CHAIN_EDGE, CHAIN_MIPS)
    return tuple(frozen(np.random.default_rng(6200 + m).integers(0, 256, (6, nb, 16), dtype=np.uint8)) for m, nb in enumerate(counts))


@functools.lru_cache(None)
def chain_cube():
    return bc6h_cube_dds(CHAIN_EDGE, list(chain_blocks()))


def assemble_face(halves, n):
    """uint16[blocks][16][3] of one image, blocks row-major -> uint16[n][n][3]: every block's 4 x 4 texels in place, the texels past the
    edge dropped"""
    nb = (n + 3) // 4
    assert halves.shape == (nb * nb, 16, 3)
    full = halves.reshape(nb, nb, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(4 * nb, 4 * nb, 3)
    return full[:n, :n]


def half_bits_as_f32(h):
    return np.ascontiguousarray(h, np.uint16).view(np.float16).astype(f32)


# the independent decoder's fixture (tools/make_bc6h_independent_golden.py): the grid, then this many random blocks
INDEPENDENT_RANDOM = 2048


@functools.lru_cache(None)
def independent_blocks():
    rnd = np.random.default_rng(6300).integers(0, 256, (INDEPENDENT_RANDOM, 16), dtype=np.uint8)
    return frozen(np.concatenate([mode_partition_blocks(), rnd]))


def to_8bit(v):
    """how an 8-bit decoder shows a float texel: floor(clip(v, 0, 1) * 255)"""
    return np.floor(np.clip(np.asarray(v, np.float64), 0, 1) * 255).astype(np.uint8)


# ---- part 3: SH ---------------------------------------------------------------------------------------------------------------------------
# 6 N^2 texels in groups of 32, eight groups to a workgroup; a sum pass for every further factor of 32
SH_SIZES = {
    1: "the ss = 0 branch, 6 texels in one group",
    2: "24 texels: one partly filled group",
    3: "54 texels: groups straddle faces, two groups",
    5: "150 texels: 5 groups, a lone, partly filled sum pass",
    7: "294 texels: 10 groups, a lone, partly filled sum pass",
    20: "2400 texels: 75 groups -> 3 -> 1",
    33: "6534 texels: 205 groups -> 7 -> 1, last workgroup partly live",
    75: "33750 texels: 1055 -> 33 -> 2 -> 1: three sum passes (they begin at N = 74), every count odd or partly filled",
}
SH_VALUE_SIZES = [20, 33]
SH_FINITE = ["random", "peak", "zero", "negzero", "subnormal"]
SH_VALUES = SH_FINITE + ["nonfinite"]
NAN_TEXEL = (1, 2, 1, 0)                                     # face, iy, ix, colour channel
INF_TEXEL = (4, 2, 1, 2)                                     # off the face's axes, so that no basis function is 0 there


def sh_passes(n):
    """element counts of the projection and of every sum pass"""
    counts = [6 * n * n]
    while counts[-1] > 1:
        counts.append((counts[-1] + 31) // 32)
    return counts


@functools.lru_cache(None)
def sh_cube(n, kind="random", poison="both"):
    """float32[6][n][n][3] radiance of one value class"""
    rng = np.random.default_rng(6400 + n)
    shape = (6, n, n, 3)
    if kind == "random":
        c = (rng.random(shape) * 4).astype(f32)
    elif kind == "peak":                                     # one texel at the largest binary16 in an otherwise black cube
        c = np.zeros(shape, f32)
        c[2, n // 3, n // 2] = 65504.0
    elif kind == "zero":
        c = np.zeros(shape, f32)
    elif kind == "negzero":
        c = np.full(shape, -0.0, f32)
    elif kind == "subnormal":                                # 1e-40 .. 1e-38 log-uniform: below or at the smallest normal, 1.18e-38
        c = (10.0 ** rng.uniform(-40, -38, shape)).astype(f32)
    elif kind == "nonfinite":
        c = (rng.random(shape) * 4).astype(f32)
        if poison in ("both", "nan"):
            c[NAN_TEXEL] = np.nan
        if poison in ("both", "inf"):
            c[INF_TEXEL] = np.inf
    else:
        raise ValueError(kind)
    return frozen(c)


def sh_terms64(cube):
    """float64: every texel's weight dOmega[6 n n] and its weighted basis products [6 n n][9][3] (CSSHCubeMap.hlsl:33-96 with the shader's
    fp32 constants)"""
    cube = np.asarray(cube, np.float64)
    n = cube.shape[1]
    iy, ix = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    px, py, pz = ix - n / 2 + 0.5, -(iy - n / 2 + 0.5), np.full((n, n), n / 2)
    dirs = [(pz, py, -px), (-pz, py, px), (px, pz, -py), (px, -pz, py), (px, py, pz), (-px, py, -pz)]      # CubeMap.hlsli:5-24
    d = np.stack([np.stack(t, axis=-1) for t in dirs])
    x, y, z = np.moveaxis(d / np.sqrt((d * d).sum(-1, keepdims=True)), -1, 0)
    ss = 2 * (1 - 1 / n) / (n - 1) if n > 1 else 0.0
    u, v = ix * ss + (1 / n - 1), iy * ss + (1 / n - 1)
    diff = 1 + u * u + v * v
    w = np.broadcast_to(4 / (np.sqrt(diff) * diff), (6, n, n))
    k = [float(f32(s)) for s in ("0.282094806", "0.488602519", "1.09254849", "0.946174681", "0.31539157", "0.546274245")]
    basis = np.stack([np.full_like(x, k[0]), -k[1] * y, k[1] * z, -k[1] * x, k[2] * y * x, -k[2] * y * z, k[3] * z * z - k[4], -k[2] * x * z,
                      k[5] * (x * x - y * y)], axis=-1)      # SHMath.hlsli:37-66
    terms = (w[..., None] * cube)[..., None, :] * basis[..., :, None]
    return w.reshape(-1), terms.reshape(-1, 9, 3)


def sh_model64(cube):
    """the SH projection as a plain float64 sum, in numpy's association order and with no tree: float64[9][3]"""
    w, terms = sh_terms64(cube)
    total = w.sum()
    return (float(f32(12.566371)) / total if total > 0 else 0.0) * terms.sum(axis=0)     # CSSHNormalize.hlsl:11-18


def sh_error(got, want64):
    """the largest difference, relative to the largest coefficient magnitude"""
    return float(np.abs(np.asarray(got, np.float64) - want64).max() / np.abs(want64).max())


# orc.sh_transform against sh_model64, measured on the CPU oracle (an fp32 tree sum of at most 33750 terms has no tighter derivable bound
# worth stating): the worst sh_error over SH_SIZES with random radiance and over the finite value classes at SH_VALUE_SIZES; the bar is
# four times that
SH_ORACLE_ERROR_SEEN = 1.9e-7
SH_ORACLE_ERROR_BAR = 4 * SH_ORACLE_ERROR_SEEN

# ---- part 4: binary16 -----------------------------------------------------------------------------------------------------------------------
HALF_CLASSES = {
    "+0": 0x0000, "-0": 0x8000,
    "smallest subnormal": 0x0001, "largest subnormal": 0x03FF, "negative subnormal": 0x83FF,
    "smallest normal": 0x0400, "1": 0x3C00, "65504": 0x7BFF,
    "+inf": 0x7C00, "-inf": 0xFC00,
    "quiet NaN": 0x7E01, "signalling NaN": 0x7D55,
}


def half_bits_to_f32_bits(h):
    """uint16 -> uint32: numpy's float16 -> float32 for the numbers; a NaN's sign and payload as bits shifted into place (no quieting)"""
    h = np.ascontiguousarray(h, np.uint16)
    out = h.view(np.float16).astype(f32).view(np.uint32).copy()
    nan = ((h & 0x7C00) == 0x7C00) & ((h & 0x03FF) != 0)
    wide = h.astype(np.uint32)
    out[nan] = (((wide & 0x8000) << 16) | 0x7F800000 | ((wide & 0x03FF) << 13))[nan]
    return out


@functools.lru_cache(None)
def half_class_chain(n=5, mips=3):
    """uint16[6][e][e][4] per mip: HALF_CLASSES cycled through the texels, each channel three classes ahead of the one before it, so that
    every mip of 12 texels or more has every class in every channel position"""
    pats = np.array(list(HALF_CLASSES.values()), np.uint16)
    chain, k = [], 0
    for e in mip_edges(n, mips):
        texel, channel = np.meshgrid(np.arange(6 * e * e), np.arange(4), indexing="ij")
        chain.append(frozen(pats[(texel + 3 * channel + k) % len(pats)].reshape(6, e, e, 4)))
        k += 6 * e * e
    return tuple(chain)
