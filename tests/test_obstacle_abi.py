"""The C ABI surface of the solid obstacles (fx_set_obstacles / fx_get_obstacles / fx_enforce_obstacles) without a device: the header as C and
C++, the ctypes and C++ mirrors, the refusals that need no context, and the host side of the enforce launch (its tiles over the solids'
bounding box), linked into a small program."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_as_c_with_the_obstacle_calls(tmp_path):
    src = tmp_path / "obstacle_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'static int (*set_)(fx_ctx*, void*, const uint8_t*, size_t, uint32_t) = fx_set_obstacles;\n'
                   'static int (*get_)(fx_ctx*, uint8_t*, size_t, uint64_t*) = fx_get_obstacles;\n'
                   'static int (*enforce_)(fx_ctx*, void*) = fx_enforce_obstacles;\n'
                   'int main(void) { (void)set_; (void)get_; (void)enforce_;\n'
                   '  return FX_OBSTACLES_DEVICE == 0x1u && sizeof(uint8_t) == 1 && sizeof(uint64_t) == 8 && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        # the constants, evaluated: a program of their own (the three calls above need the library to link)
        val = tmp_path / "obstacle_values.c"
        val.write_text('#include "fluidx_hip.h"\nint main(void) { return FX_OBSTACLES_DEVICE == 0x1u && FX_OBSTACLES_DEVICE == FX_DEPTH_DEVICE && FX_ABI_VERSION == 7 ? 0 : 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(val), "-o", str(tmp_path / "values")], check=True)
        assert subprocess.run([str(tmp_path / "values")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_mirrors_carry_the_three_calls():
    from fluidx12_amd import capi
    import fluidx12_amd as fx
    for name in ("fx_set_obstacles", "fx_get_obstacles", "fx_enforce_obstacles"):
        assert name in capi.SYMBOLS
    assert capi.OBSTACLES_DEVICE == 1 and capi.ABI_VERSION == 7
    assert capi.SYMBOLS["fx_set_obstacles"][1][3:] == [C.c_size_t, C.c_uint32]
    for name in ("SetObstacles", "GetObstacles", "EnforceObstacles"):
        assert callable(getattr(fx.Fluid, name))
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetObstacles", "GetObstacles", "EnforceObstacles", "fx_set_obstacles", "fx_get_obstacles", "fx_enforce_obstacles"):
        assert name in hpp, name
    from fluidx12_amd import build
    assert "fx_obstacle.hip" in build.SOURCES


def test_refusals_that_need_no_device():
    from fluidx12_amd import capi
    lib = capi.load()
    mask = (C.c_uint8 * 8)()
    n = C.c_uint64(7)
    assert lib.fx_set_obstacles(None, None, mask, 8, 0) == capi.FX_E_INVALID
    assert lib.fx_set_obstacles(None, None, None, 0, 0) == capi.FX_E_INVALID
    assert lib.fx_get_obstacles(None, mask, 8, C.byref(n)) == capi.FX_E_INVALID and n.value == 7
    assert lib.fx_enforce_obstacles(None, None) == capi.FX_E_INVALID


PROBE = r"""
// obstacle_enforce_tiles through its own declaration (fx_internal.h): lo x y z, hi x y z
#include "fx_internal.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
	if (argc < 7) return 2;
	int lo[3], hi[3], x0 = -1, y0 = -1, tx = -1, ty = -1;
	for (int a = 0; a < 3; ++a) { lo[a] = atoi(argv[1 + a]); hi[a] = atoi(argv[4 + a]); }
	const long long wgs = fx::obstacle_enforce_tiles(lo, hi, &x0, &y0, &tx, &ty);
	printf("%lld %d %d %d %d\n", wgs, x0, y0, tx, ty);
	return 0;
}
"""


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    """the host function out of fx_obstacle.hip, compiled as the library's sources are: no device is needed to run it"""
    from fluidx12_amd import build
    d = tmp_path_factory.mktemp("obstacle_tiles")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.run([build.hipcc()] + build.FLAGS + ["-I", build.CSRC, "-x", "hip", str(src), os.path.join(build.CSRC, "fx_obstacle.hip"),
                    os.path.join(build.CSRC, "fx_knobs.cpp"), "-o", str(exe)], check=True, capture_output=True)

    def call(lo, hi):
        out = subprocess.run([str(exe)] + [str(v) for v in tuple(lo) + tuple(hi)], check=True, capture_output=True, text=True).stdout.split()
        return tuple(int(v) for v in out)
    return call


def test_enforce_tiles_follow_the_box_not_the_grid(tiles):
    # a ball of radius 0.15 at the centre of 256^3: cells 90 .. 166 per axis
    wgs, x0, y0, tx, ty = tiles((90, 90, 90), (167, 167, 167))
    assert (x0, y0, tx, ty) == (64, 88, 2, 20) and wgs == 2 * 20 * 77      # x 64..191 in two tiles; rows 88..167 in fours; of the grid's 65536 tiles
    assert tiles((0, 0, 0), (1, 1, 1)) == (1, 0, 0, 1, 1)
    assert tiles((63, 3, 5), (65, 5, 6)) == (4, 0, 0, 2, 2)                  # a box across a tile corner
    assert tiles((64, 4, 0), (128, 8, 3)) == (3, 64, 4, 1, 1)               # exactly one tile, three planes
    for empty in (((0, 0, 0), (0, 0, 0)), ((5, 5, 5), (5, 9, 9)), ((3, 3, 3), (9, 9, 2))):
        assert tiles(*empty)[0] == 0
