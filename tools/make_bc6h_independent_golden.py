#!/usr/bin/env python3
"""Writes tests/golden/bc6h_independent.npz: an independent decoder's view of BC6H_UF16 blocks, which pins the oracle's decoder
(oracle/orc_bc6h.cpp) -- and through it the kernel's -- to something neither was written beside.

The blocks are tests/probe_edges.py's own: one for every two-region mode x partition, some for every one-region and reserved mode, and
2048 random ones.  They are wrapped as a plain 2-D BC6H_UF16 DDS and decoded by Pillow (PIL.DdsImagePlugin), which returns 8-bit RGB:
values below 1 keep 8 bits, values of 1 and more saturate.  The fixture holds the blocks, Pillow's pixels per block, the Pillow version and
the share of channel values on which floor(clip(oracle, 0, 1) * 255) differs from Pillow's at all (by one step: Pillow goes through
float arithmetic of its own) -- overall, and the largest share of any one mode, which is what the test's per-mode cap is four times of
(the one-step differences gather in the modes with endpoints of 11 bits and more).  tests/test_probe_edges.py reads the fixture only;
Pillow is needed here and nowhere else.

    python tools/make_bc6h_independent_golden.py            # needs Pillow with BC6H support (>= 10.1)
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "bc6h_independent.npz")
BLOCKS_WIDE = 64


def main():
    try:
        import PIL
        from PIL import Image
    except ImportError:
        print("Pillow is not installed: the fixture is written only where it is")
        return 1
    import probe_edges as pe
    from oracle import orc

    blocks = pe.independent_blocks()
    assert len(blocks) % BLOCKS_WIDE == 0
    bw, bh = BLOCKS_WIDE, len(blocks) // BLOCKS_WIDE
    im = Image.open(io.BytesIO(pe.bc6h_image_dds(blocks, bw, bh)))
    assert im.mode == "RGB" and im.size == (4 * bw, 4 * bh), (im.mode, im.size)
    px = np.asarray(im, np.uint8)
    rgb8 = px.reshape(bh, 4, bw, 4, 3).transpose(0, 2, 1, 3, 4).reshape(len(blocks), 16, 3)      # [block][texel, row-major][rgb]

    halves, modes = orc.bc6h_decode_blocks(blocks)
    ours = pe.to_8bit(pe.half_bits_as_f32(halves))
    step = np.abs(ours.astype(int) - rgb8.astype(int))
    overall = float((step > 0).mean())
    per_mode = [float((step[modes == m] > 0).mean()) for m in range(15)]
    print("%d blocks, Pillow %s: largest difference %d step(s), share of differing values %.3e" % (len(blocks), PIL.__version__, step.max(), overall))
    for m in range(15):
        print("  mode %2d: %4d blocks, largest difference %d, share %.3e" % (m, (modes == m).sum(), step[modes == m].max(), per_mode[m]))
    np.savez_compressed(OUT, blocks=blocks, rgb8=rgb8, pillow_version=np.array(PIL.__version__), differing_share=np.array(max(per_mode)),
                        differing_share_overall=np.array(overall))
    print("wrote %s (%d bytes)" % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
