"""CPU checks of the moving obstacles (fx_set_obstacle_bodies): the numpy model tests/moving_obstacle_ref.py -- anchored to the resting
obstacles' reference (no bodies, or bodies that hold no solid cell, change no bit), the rules on single cells worked by hand, a plate that
pushes the air in front of it -- and the C ABI surface without a device: the header as C, the ctypes and C++ mirrors, the refusals that need
no context.  tests/test_gpu_moving_obstacles.py holds the kernels against this model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import moving_obstacle_ref as mv
import test_obstacle_ref as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1: at rest the model is the resting reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(20, 20, 5), (36, 36, 1)])
def test_at_rest_the_model_is_the_obstacle_reference_bit_for_bit(dims):
    X, Y, Z = dims
    rng = np.random.default_rng(71)
    vel = rng.standard_normal((3, Z, Y, X)).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    p = rng.standard_normal((Z, Y, X)).astype(f32)
    m = ob.random_mask(dims)
    m[:, 4:9, 11:17] = 0                                               # a pocket of fluid: the boxes below hold cells, none of them solid
    pocket = mv.body((11.0 / X, 4.0 / Y, 0.0), (17.0 / X, 9.0 / Y, 1.0), linear=(3.0, -2.0, 1.0), angular=(0.5, -4.0, 7.0))
    nowhere = mv.body((2.0, 2.0, 2.0), (3.0, 3.0, 3.0), linear=(9.0, 9.0, 9.0))            # outside the texture
    assert (mv.body_of((Z, Y, X), [pocket, nowhere]) == 0).sum() == 5 * 6 * Z and not m[mv.body_of((Z, Y, X), [pocket, nowhere]) >= 0].any()
    for bodies in ([], [pocket, nowhere]):
        wv, wc = ob.ref_enforce(vel, col, m)
        gv, gc = mv.ref_enforce(vel, col, m, bodies)
        assert same_bits(gv, wv) and same_bits(gc, wc)
        assert same_bits(mv.ref_divergence(wv, m, bodies), ob.ref_divergence(wv, m))
        for half in (False, True):
            v = wv.astype(np.float16).astype(f32) if half else wv
            assert same_bits(mv.ref_project(v, p, m, bodies, 0, half), ob.ref_project(v, p, m, half))


# ---- 2: the rules on single cells, by hand ------------------------------------------------------------------------------------------------
SHAPE = (5, 9, 9)                                                      # Z, Y, X


def centre(i, n):
    return f32(f32(i) + f32(0.5)) / f32(n)


def box_of_cells(x, y, z, shape=SHAPE):
    """a box that holds exactly the cells x[0]..x[1], y[0]..y[1], z[0]..z[1] (cell bounds: centres lie strictly inside)"""
    Z, Y, X = shape
    return (x[0] / X, y[0] / Y, z[0] / Z), ((x[1] + 1.0) / X, (y[1] + 1.0) / Y, (z[1] + 1.0) / Z)


def test_a_solid_cell_moving_along_x_beside_a_fluid_cell():
    Z, Y, X = SHAPE
    m = np.zeros(SHAPE, np.uint8)
    m[2, 4, 4] = 1
    lo, hi = box_of_cells((4, 4), (4, 4), (2, 2))
    bodies = [mv.body(lo, hi, linear=(0.75, 0.0, 0.0))]
    vel = np.ones((3,) + SHAPE, f32)
    col = np.ones(SHAPE + (4,), f32)
    v1, c1 = mv.ref_enforce(vel, col, m, bodies)
    assert tuple(v1[:, 2, 4, 4]) == (f32(0.75), 0, 0) and not bits(c1[2, 4, 4]).any()
    assert same_bits(np.delete(v1.reshape(3, -1), 2 * 81 + 4 * 9 + 4, 1), np.ones((3, 5 * 81 - 1), f32))      # fluid cells keep their bits
    b = mv.ref_divergence(v1, m, bodies)
    # left of it: dd_x = -1 + 0.75; right of it: -0.75 + 1; above / in front: the wall's w_y = w_z = 0 where the fluid has 1
    assert b[2, 4, 3] == f32(-0.125) and b[2, 4, 5] == f32(0.125) and b[2, 3, 4] == f32(-0.5) and b[1, 4, 4] == f32(-0.5)
    assert b[2, 4, 4] == 0 and b[2, 2, 2] == 0
    out = mv.ref_project(v1, np.zeros(SHAPE, f32), m, bodies)
    assert tuple(out[:, 2, 4, 4]) == (f32(0.75), 0, 0)
    assert out[0, 2, 4, 3] == f32(0.75) and out[0, 2, 4, 5] == f32(0.75)          # the normal component is the wall's
    assert out[1, 2, 3, 4] == 0 and out[2, 1, 4, 4] == 0                           # ... which is 0 along y and z
    assert out[1, 2, 4, 3] == 1 and out[2, 2, 4, 3] == 1                           # free slip along it


def test_a_fluid_cell_between_two_bodies_takes_the_mean():
    m = np.zeros(SHAPE, np.uint8)
    m[2, 4, 3] = m[2, 4, 5] = 1
    a = mv.body(*box_of_cells((3, 3), (4, 4), (2, 2)), linear=(0.5, 0.0, 0.0))
    c = mv.body(*box_of_cells((5, 5), (4, 4), (2, 2)), linear=(-0.125, 0.0, 0.0))
    vel = np.zeros((3,) + SHAPE, f32)
    out = mv.ref_project(vel, np.zeros(SHAPE, f32), m, [a, c])
    assert out[0, 2, 4, 4] == f32(0.5) * (f32(0.5) + f32(-0.125))
    assert out[0, 2, 4, 2] == f32(0.5) and out[0, 2, 4, 6] == f32(-0.125)         # one solid neighbour: its w_x
    b = mv.ref_divergence(vel, m, [a, c])
    assert b[2, 4, 4] == f32(0.5) * (f32(-0.5) + f32(-0.125))                      # the two walls close in on the cell


def test_the_first_box_wins_and_a_solid_in_no_box_rests():
    m = np.zeros(SHAPE, np.uint8)
    m[2, 4, 4] = m[2, 4, 5] = m[0, 0, 0] = 1
    first = mv.body(*box_of_cells((4, 4), (4, 4), (2, 2)), linear=(1.0, 2.0, 3.0))
    second = mv.body(*box_of_cells((4, 5), (4, 4), (2, 2)), linear=(-1.0, -2.0, -3.0))
    who = mv.body_of(SHAPE, [first, second])
    assert who[2, 4, 4] == 0 and who[2, 4, 5] == 1 and who[0, 0, 0] == -1 and (who >= 0).sum() == 2
    v1, _ = mv.ref_enforce(np.ones((3,) + SHAPE, f32), np.ones(SHAPE + (4,), f32), m, [first, second])
    assert tuple(v1[:, 2, 4, 4]) == (1, 2, 3) and tuple(v1[:, 2, 4, 5]) == (-1, -2, -3)
    assert not bits(v1[:, 0, 0, 0]).any()                                         # +0, bit for bit
    v2, _ = mv.ref_enforce(np.ones((3,) + SHAPE, f32), np.ones(SHAPE + (4,), f32), m, [second, first])
    assert tuple(v2[:, 2, 4, 4]) == (-1, -2, -3)
    # a closed box: a centre ON its bound belongs to it
    on = mv.body((float(centre(4, 9)), float(centre(4, 9)), float(centre(2, 5))), (float(centre(5, 9)), float(centre(4, 9)), float(centre(2, 5))))
    assert (mv.body_of(SHAPE, [on]) == 0).sum() == 2
    # a 2-D grid ignores z
    flat = mv.body((0.0, 0.0, 5.0), (1.0, 1.0, 6.0))
    assert (mv.body_of((1, 9, 9), [flat]) == 0).all() and (mv.body_of(SHAPE, [flat]) == -1).all()


def test_pure_rotation_about_a_pivot_inside_the_body():
    Z, Y, X = SHAPE
    m = np.zeros(SHAPE, np.uint8)
    m[1:4, 3:6, 3:6] = 1
    pivot = (float(centre(4, X)), float(centre(4, Y)), float(centre(2, Z)))
    spin = mv.body(*box_of_cells((3, 5), (3, 5), (1, 3)), angular=(0.0, 0.0, 2.0), pivot=pivot)
    w = mv.wall_velocity(SHAPE, [spin])
    assert not w[:, 2, 4, 4].any()                                                # the pivot's cell does not move
    rx, ry = centre(5, X) - f32(pivot[0]), centre(5, Y) - f32(pivot[1])
    assert w[0, 2, 5, 4] == -f32(2.0) * ry and w[1, 2, 4, 5] == f32(2.0) * rx      # w = omega x r: one rounding each (the addend is 0)
    assert w[0, 2, 3, 4] == -w[0, 2, 5, 4] and w[1, 2, 4, 3] == -w[1, 2, 4, 5] and not w[2].any()
    # all three axes, in the header's fma order
    tumble = mv.body(*box_of_cells((3, 5), (3, 5), (1, 3)), linear=(0.25, -0.5, 1.0), angular=(3.0, -5.0, 7.0), pivot=pivot)
    w = mv.wall_velocity(SHAPE, [tumble])
    r = [centre(5, X) - f32(pivot[0]), centre(3, Y) - f32(pivot[1]), centre(3, Z) - f32(pivot[2])]
    fm = mv.fma
    assert w[0, 3, 3, 5] == fm(f32(-5.0), r[2], fm(f32(-7.0), r[1], f32(0.25)))
    assert w[1, 3, 3, 5] == fm(f32(7.0), r[0], fm(f32(-3.0), r[2], f32(-0.5)))
    assert w[2, 3, 3, 5] == fm(f32(3.0), r[1], fm(f32(5.0), r[0], f32(1.0)))
    # 2-D: only angular_z acts, w_z = +0
    w2 = mv.wall_velocity((1, Y, X), [tumble])
    assert w2[0, 0, 3, 5] == fm(f32(-7.0), r[1], f32(0.25)) and w2[1, 0, 3, 5] == fm(f32(7.0), r[0], f32(-0.5)) and not bits(w2[2]).any()
    # the enforce pass stores it, the projection leaves it
    v1, _ = mv.ref_enforce(np.zeros((3,) + SHAPE, f32), np.zeros(SHAPE + (4,), f32), m, [spin])
    solid = m.astype(bool)
    wspin = mv.wall_velocity(SHAPE, [spin])
    assert same_bits(v1[:, solid], wspin[:, solid])
    assert same_bits(mv.ref_project(v1, np.zeros(SHAPE, f32), m, [spin])[:, solid], wspin[:, solid])
    half = mv.ref_enforce(np.zeros((3,) + SHAPE, f32), np.zeros(SHAPE + (4,), f32), m, [tumble], half=True)[0]
    assert same_bits(half[:, solid], w[:, solid].astype(np.float16).astype(f32))   # rounded once to the storage


# ---- 3: a plate pushes the air in front of it -----------------------------------------------------------------------------------------
PLATE_DIMS, PLATE_X, PLATE_W = (32, 32, 8), (10, 11), 0.4             # two cells thick, in the left half: the wall damping is 1 around it


def plate_scene(dims=PLATE_DIMS):
    X, Y, Z = dims
    m = np.zeros((Z, Y, X), np.uint8)
    m[2:Z - 2, 8:24, PLATE_X[0]:PLATE_X[1] + 1] = 1
    lo, hi = box_of_cells(PLATE_X, (8, 23), (2, Z - 3), (Z, Y, X))
    return m, [mv.body(lo, hi, linear=(PLATE_W, 0.0, 0.0))]


def test_a_plate_pushes_the_air_in_front_of_it():
    X, Y, Z = PLATE_DIMS
    m, bodies = plate_scene()
    zero_v, zero_c, zero_p = np.zeros((3, Z, Y, X), f32), np.zeros((Z, Y, X, 4), f32), np.zeros((Z, Y, X), f32)
    v1, _, b, q, out = mv.ref_step(zero_v, zero_c, zero_p, m, bodies, 20)
    _, _, b0, q0, out0 = mv.ref_step(zero_v, zero_c, zero_p, m, [], 20)
    lead = (slice(2, Z - 2), slice(8, 24), PLATE_X[1] + 1)            # the fluid cells on the leading face
    trail = (slice(2, Z - 2), slice(8, 24), PLATE_X[0] - 1)
    assert (out[0][lead] == f32(PLATE_W)).all() and (out[0][trail] == f32(PLATE_W)).all()
    assert (b[lead] == f32(0.5) * -f32(PLATE_W)).all() and (b[trail] == f32(0.5) * f32(PLATE_W)).all()      # compression ahead, suction behind
    assert not b0.any() and not q0.any() and not out0.any()           # the resting model: nothing moves at all
    assert (q[lead] > 0).all() and (q[trail] < 0).all()               # high pressure ahead of the plate, low behind
    solid = m.astype(bool)
    assert (out[0][solid] == f32(PLATE_W)).all() and not out[1:][:, solid].any()
    # the air two cells ahead is pushed along by the pressure gradient
    assert (out[0][2:Z - 2, 8:24, PLATE_X[1] + 2] > 0).all()


# ---- 4: the C ABI surface ---------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_with_the_body_calls(tmp_path):
    src = tmp_path / "bodies_probe.c"
    src.write_text('#include "fluidx_hip.h"\n'
                   'static int (*set_)(fx_ctx*, const fx_obstacle_body*, uint32_t) = fx_set_obstacle_bodies;\n'
                   'static int (*get_)(fx_ctx*, fx_obstacle_body*, uint32_t, uint32_t*) = fx_get_obstacle_bodies;\n'
                   'int main(void) { (void)set_; (void)get_; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "probe.o")], check=True)
        val = tmp_path / "bodies_values.c"
        val.write_text('#include <stddef.h>\n#include "fluidx_hip.h"\n'
                       'int main(void) { return sizeof(fx_obstacle_body) == 68 && FX_MAX_OBSTACLE_BODIES == 16u && FX_ABI_VERSION == 7\n'
                       '  && offsetof(fx_obstacle_body, box_lo) == 8 && offsetof(fx_obstacle_body, box_hi) == 20 && offsetof(fx_obstacle_body, linear) == 32\n'
                       '  && offsetof(fx_obstacle_body, angular) == 44 && offsetof(fx_obstacle_body, pivot) == 56 ? 0 : 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(val), "-o", str(tmp_path / "values")], check=True)
        assert subprocess.run([str(tmp_path / "values")]).returncode == 0
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_mirrors_carry_the_two_calls():
    from fluidx12_amd import capi
    import fluidx12_amd as fx
    for name in ("fx_set_obstacle_bodies", "fx_get_obstacle_bodies"):
        assert name in capi.SYMBOLS
    assert capi.MAX_OBSTACLE_BODIES == 16 and capi.ABI_VERSION == 7 and C.sizeof(capi.ObstacleBody) == 68
    assert [n for n, _ in capi.ObstacleBody._fields_] == ["struct_size", "flags", "box_lo", "box_hi", "linear", "angular", "pivot"]
    assert capi.SYMBOLS["fx_set_obstacle_bodies"][1][1:] == [C.POINTER(capi.ObstacleBody), C.c_uint32]
    for name in ("SetObstacleBodies", "GetObstacleBodies"):
        assert callable(getattr(fx.Fluid, name))
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for name in ("SetObstacleBodies", "GetObstacleBodies", "fx_set_obstacle_bodies", "fx_get_obstacle_bodies"):
        assert name in hpp, name
    from fluidx12_amd import build
    assert "fx_obstacle.hip" in build.SOURCES and "fx_obstacle_moving.hip" not in build.SOURCES      # one file holds the resting and the moving rules
    demo = open(os.path.join(ROOT, "examples", "fluidx_demo.cpp")).read()
    assert "-obstacleVelocity" in demo and "SetObstacleBodies" in demo


def test_refusals_that_need_no_device():
    from fluidx12_amd import capi
    lib = capi.load()
    one = (capi.ObstacleBody * 1)()
    one[0].struct_size = C.sizeof(capi.ObstacleBody)
    n = C.c_uint32(7)
    assert lib.fx_set_obstacle_bodies(None, one, 1) == capi.FX_E_INVALID
    assert lib.fx_set_obstacle_bodies(None, None, 0) == capi.FX_E_INVALID
    assert lib.fx_get_obstacle_bodies(None, one, 1, C.byref(n)) == capi.FX_E_INVALID and n.value == 7
