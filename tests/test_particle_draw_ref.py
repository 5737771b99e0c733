"""The particle draw (fx_set_particle_draw), CPU side: the C ABI surface and the numpy model of tests/particle_draw_ref.py -- vectorised against
plain loops, the footprint's weights, the edge of the viewport, the scene depth, the colour ramp, every cull class, and the conditions the GPU
tests' inputs are chosen under (the occlusion is neither trivially 0 nor trivially 1).  The occlusion itself is not restated: it comes from the
depth-aware CPU reference (test_depth_ref.ref_direct)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import particle_draw_ref as pd
from oracle import orc
from test_depth_ref import analytic_depth, smoke_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
X = 32
VP = (200, 150)
NS, NL = 48, 16
LIFETIME = 2.0
DRAW = {"color": (1.0, 0.6, 0.2, 3.0), "end_color": (0.4, 0.1, 0.05, 1.5)}


def camera(vp, inside=False):
    import fluidx12_amd as fx
    view, proj, eye = pd.inside_camera(*vp) if inside else fx.default_camera(*vp)
    view, proj = np.ascontiguousarray(view, f32).reshape(16), np.ascontiguousarray(proj, f32).reshape(16)
    fr = orc.update_frame(view, proj, eye, vp[0], vp[1], X, NS)[0]
    return view, proj, eye, fr, orc.world_view_proj_inverse(view, proj), pd.forward_wvp(view, proj)


_CACHE = {}


def drawn(n, vp=VP, inside=False, empty=False, dead_every=5):
    """(records, projection, T) of the n-record set in the smoke scene (or an empty volume), computed once"""
    key = (n, vp, inside, empty, dead_every)
    if key not in _CACHE:
        view, proj, eye, fr, wvp_i, M = camera(vp, inside)
        col = np.zeros((X, X, X, 4), f32) if empty else smoke_scene(X)
        rec = pd.records(n, LIFETIME, dead_every=dead_every)
        P = pd.project(rec, M, vp[0], vp[1])
        _CACHE[key] = (rec, P, pd.transmittance(P, col, fr, wvp_i, vp[0], vp[1], NS, NL), M)
    return _CACHE[key]


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_abi_offers_particle_draw():
    from fluidx12_amd import capi
    import fluidx12_amd as fx
    src = open(os.path.join(ROOT, "include", "fluidx_hip.h")).read()
    for name in ("fx_set_particle_draw", "fx_get_particle_draw", "fx_draw_particles", "fx_particle_splats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.load(), name)
    assert C.sizeof(capi.ParticleDraw) == 40
    assert "sizeof(fx_particle_draw) = 40" in src
    assert int(re.search(r"#define\s+FX_ABI_VERSION\s+(\d+)", src).group(1)) == capi.ABI_VERSION == 7
    lib = capi.load()
    assert lib.fx_set_particle_draw(None, None) == capi.FX_E_INVALID
    assert lib.fx_get_particle_draw(None, None) == capi.FX_E_INVALID
    assert lib.fx_draw_particles(None, None, 0) == capi.FX_E_INVALID
    assert lib.fx_particle_splats(None, None, None, 0) == capi.FX_E_INVALID
    for m in ("SetParticleDraw", "GetParticleDraw", "DrawParticles", "ParticleSplats"):
        assert callable(getattr(fx.Fluid, m)), m
    hpp = open(os.path.join(ROOT, "fluidx12_amd", "csrc", "Fluid.hpp")).read()
    for m in ("SetParticleDraw", "GetParticleDraw", "DrawParticles", "ParticleSplats"):
        assert m in hpp, m


# ---- the camera the model projects with is the host's ---------------------------------------------------------------------------------------------
def test_forward_matrix_inverts_the_inverse():
    """M restates fx_update_frame's fp32 product; against the oracle's inverse it is the identity to fp32 accuracy"""
    view, proj, eye, fr, wvp_i, M = camera(VP)
    I = M.reshape(4, 4).T.astype(np.float64) @ wvp_i.T.astype(np.float64)
    assert np.abs(I - np.eye(4)).max() < 1e-4


# ---- the conditions on the inputs ------------------------------------------------------------------------------------------------------------------
def test_the_inputs_make_the_occlusion_matter():
    rec, P, T, M = drawn(4099, dead_every=0)
    assert np.all(P["cls"] == pd.DRAWN)                               # every point of the unit cube is on screen under the default camera
    assert int(pd.layers_of(P, VP[0]).max()) + 1 <= pd.MAX_LAYERS
    assert len(np.unique(P["py"] * VP[0] + P["px"])) > 2500
    mid = ((T > 0.05) & (T < 0.95)).mean()
    one = (T == 1).mean()
    print("middle band %.3f, exactly one %.3f, min %.4f" % (mid, one, T.min()))
    assert mid >= 0.25 and one >= 0.25
    rec, P, T, M = drawn(4099)                                        # the set the GPU tests draw: one record in five dead
    on = P["cls"] == pd.DRAWN
    assert (P["cls"] == pd.DEAD).sum() == 4099 // 5 and on.sum() == 4099 - 4099 // 5
    assert ((T[on] > 0.05) & (T[on] < 0.95)).mean() >= 0.25 and (T[on] == 1).mean() >= 0.25


# ---- vectorised == loops -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,inside", [(1, False), (257, False), (4099, False), (4099, True)])
def test_vectorised_equals_loops(n, inside):
    rec, P, T, M = drawn(n, inside=inside)
    W, H = VP
    a = pd.splats(rec, P, T, LIFETIME, W, H)
    b = pd.splats_loops(rec, M, W, H, T, LIFETIME)
    assert np.array_equal(a, b) and a.any()
    if n == 257:
        target = np.random.default_rng(1).integers(0, 256, (H, W, 4)).astype(np.uint8)
        tf_a, t_a = pd.resolve(a, DRAW, target)
        tf_b, t_b = pd.resolve_loops(a, DRAW, target)
        assert np.array_equal(tf_a.view(np.uint32), tf_b.view(np.uint32)) and np.array_equal(t_a, t_b)
        hit = (a[..., 0] | a[..., 1]) != 0
        assert np.array_equal(t_a[~hit], target[~hit]) and np.array_equal(t_a[..., 3], target[..., 3])      # alpha 0: the target's alpha stays
        assert (t_a[hit, :3] >= target[hit, :3]).all() and (t_a[hit, :3] > target[hit, :3]).any()          # ... and the blend only adds


def test_special_values_go_where_the_rule_says():
    """positions the clamp has to catch, ages on the edge of the live test: the loops and the vectorised model agree, nothing lands off the array"""
    import particle_ref as pr
    view, proj, eye, fr, wvp_i, M = camera(VP)
    pts = pr.edge_points((X, X, X))
    rec = np.concatenate([pts, np.zeros((len(pts), 1), f32)], axis=1).astype(f32)
    rec[::3, 3] = f32(-0.0)
    rec[1::7, 3] = f32(np.nan)
    rec[2::7, 3] = f32(np.inf)
    P = pd.project(rec, M, *VP)
    T = np.linspace(0, 1, len(rec)).astype(f32)
    assert np.array_equal(pd.splats(rec, P, T, LIFETIME, *VP), pd.splats_loops(rec, M, VP[0], VP[1], T, LIFETIME))
    assert (P["cls"] == pd.DEAD).sum() == np.isnan(rec[:, 3]).sum()      # -0.0 and +inf are live, a NaN is dead
    assert (P["cls"] == pd.DRAWN).sum() == len(rec) - np.isnan(rec[:, 3]).sum()   # every clamped position is a point of the cube, on screen


# ---- the footprint ---------------------------------------------------------------------------------------------------------------------------------
def one_record_at(Xp, Yp, W, H, T=1.0, age=0.0):
    """the splat of one record whose projection is forced to (Xp, Yp): the footprint and the amounts alone"""
    P = {"cls": np.array([pd.DRAWN]), "X": np.array([Xp], f32), "Y": np.array([Yp], f32)}
    return pd.splats(np.array([[0, 0, 0, age]], f32), P, np.array([T], f32), LIFETIME, W, H)


def test_a_particle_on_a_pixel_centre_puts_everything_into_that_pixel():
    acc = one_record_at(17.5, 9.5, 40, 30, T=0.625)
    qb = int(0.625 * 32768 + 0.5)
    assert acc[9, 17, 0] == qb << 22 and acc.sum() == qb << 22


def test_the_four_weights_sum_to_two_to_the_fourteen():
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.random(5000) * 40, [0.0, 0.5, 39.5, np.nextafter(f32(40), f32(0)), 17.0, 17.25]]).astype(f32)
    i0, w0, w1 = pd.foot_axis(xs)
    assert np.all(w0 + w1 == 128) and np.all((w0 >= 0) & (w1 >= 0))
    assert np.all((i0 >= -1) & (i0 + 1 <= 40))
    j0, v0, v1 = pd.foot_axis(xs[::-1])
    assert np.all((w0 + w1) * (v0 + v1) == 1 << 14)
    acc = one_record_at(17.3, 9.8, 40, 30)                            # inside: the whole amount arrives
    assert acc.sum() == pd.ONE and (acc[..., 0] != 0).sum() == 4


def test_a_footprint_at_the_edge_loses_exactly_the_dropped_weights():
    W, H = 40, 30
    for Xp, Yp in ((0.2, 9.8), (39.9, 9.8), (17.3, 0.1), (17.3, 29.7), (0.1, 0.3), (39.8, 29.9)):
        acc = one_record_at(Xp, Yp, W, H)
        (ix,), (wx0,), (wx1,) = pd.foot_axis(np.array([Xp], f32))
        (iy,), (wy0,), (wy1,) = pd.foot_axis(np.array([Yp], f32))
        kept_x = (wx0 if 0 <= ix < W else 0) + (wx1 if 0 <= ix + 1 < W else 0)
        kept_y = (wy0 if 0 <= iy < H else 0) + (wy1 if 0 <= iy + 1 < H else 0)
        assert kept_x * kept_y < 1 << 14
        assert int(acc.sum()) == (32768 * 256) * int(kept_x * kept_y)


# ---- the occlusion's trivial case ---------------------------------------------------------------------------------------------------------------
def test_an_empty_volume_dims_nothing():
    rec, P, T, M = drawn(257, empty=True)
    assert np.all(T == 1)
    acc = pd.splats(rec, P, T, LIFETIME, *VP)
    on = P["cls"] == pd.DRAWN
    ix, _, _ = pd.foot_axis(P["X"][on])
    iy, _, _ = pd.foot_axis(P["Y"][on])
    assert np.all((ix >= 0) & (ix + 1 < VP[0]) & (iy >= 0) & (iy + 1 < VP[1]))      # every footprint is on screen
    assert int(acc.sum()) == int(on.sum()) << 37


# ---- the scene depth ---------------------------------------------------------------------------------------------------------------------------
def test_a_particle_behind_a_depth_plane_is_culled_and_one_on_it_is_drawn():
    rec, P, T, M = drawn(257)
    W, H = VP
    k = int(np.nonzero(P["cls"] == pd.DRAWN)[0][0])
    cz, px, py = P["cz"][k], P["px"][k], P["py"][k]
    for d, cls in ((cz, pd.DRAWN), (np.nextafter(cz, f32(0)), pd.HIDDEN), (np.nextafter(cz, f32(2)), pd.DRAWN), (f32(np.nan), pd.HIDDEN)):
        depth = np.ones((H, W), f32)
        depth[py, px] = d
        assert pd.project(rec, M, W, H, depth)["cls"][k] == cls
    view, proj, eye, fr, wvp_i, M = camera(VP)
    depth = analytic_depth(proj, W, H, plane=(0.3, 0.2, float(np.linalg.norm(eye))))
    Q = pd.project(rec, M, W, H, depth)
    hidden = Q["cls"] == pd.HIDDEN
    assert 0.2 < hidden.sum() / (P["cls"] == pd.DRAWN).sum() < 0.8
    a = pd.splats(rec, Q, T, LIFETIME, W, H)
    assert np.array_equal(a, pd.splats_loops(rec, M, W, H, T, LIFETIME, depth))
    assert int(a.sum()) < int(pd.splats(rec, P, T, LIFETIME, W, H).sum())


# ---- the colour ramp -------------------------------------------------------------------------------------------------------------------------------
def test_end_color_takes_over_linearly_in_qs():
    ages = np.array([0.0, 0.25, 0.5, 1.0, 1.99, 2.0, 3.0, np.inf], f32)
    young, old = pd.amounts(np.full(len(ages), 0.5, f32), ages, LIFETIME)
    qs = np.array([0, 32, 64, 128, 255, 256, 256, 256])
    assert np.array_equal(old, 16384 * qs) and np.array_equal(young, 16384 * (256 - qs))
    young, old = pd.amounts(np.full(len(ages), 0.5, f32), ages, 0.0)       # immortal particles never age
    assert not old.any() and np.all(young == 16384 * 256)
    for age, qs_ in zip(ages[:6], qs[:6]):
        acc = one_record_at(17.5, 9.5, 40, 30, age=age)
        src = pd.source(acc, DRAW)[9, 17]
        k0 = np.array(DRAW["color"][:3], f32) * f32(DRAW["color"][3])
        k1 = np.array(DRAW["end_color"][:3], f32) * f32(DRAW["end_color"][3])
        want = (k0.astype(np.float64) * (256 - qs_) + k1.astype(np.float64) * qs_) / 256
        assert np.allclose(src, want, rtol=1e-6, atol=0)


# ---- every cull class -----------------------------------------------------------------------------------------------------------------------------
def test_the_inside_camera_makes_every_cull_class_non_empty():
    rec, P, T, M = drawn(4099, inside=True)
    counts = {c: int((P["cls"] == c).sum()) for c in range(6)}
    print(counts)
    for c in (pd.DRAWN, pd.DEAD, pd.BEHIND, pd.Z_OUT, pd.X_OUT, pd.Y_OUT):
        assert counts[c] > 0, (c, counts)
    on = P["cls"] == pd.DRAWN
    assert ((T[on] > 0.05) & (T[on] < 0.95)).mean() > 0.5               # the eye sits in the smoke: no particle is seen undimmed
