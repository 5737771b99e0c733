"""The obstacle draw on the GPU (fx_set_obstacle_draw / fx_draw_obstacles / fx_obstacle_hits, csrc/fx_obstacle_draw.hip) against the numpy
model tests/obstacle_draw_ref.py: hits words, depth bits, FX_FIELD_TARGET_FLOAT bit for bit, FX_FIELD_TARGET byte for byte.

Every case at most 32^3: the scene of tests/test_obstacle_draw_ref.py (a ball, a slab on two walls, a beam through two walls) on 32^3,
30 x 30 x 18 (ragged bricks) and 32 x 32 x 16; viewports 200 x 150 and 67 x 41 (rows that are no multiple of a wave's 8 x 8 tile) and 65 x 65
for the axis-aligned camera.  The model runs with the context's own inverse matrix (fx_frame_info) and is computed once per case.

Not run: the refusal of a grid of 2^32 cells or more -- such a context takes hundreds of gigabytes; odraw_guard's test is one line."""
import ctypes as C

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi

import obstacle_draw_ref as od
import particle_draw_ref as pd
import voxelize_ref as vr
from test_depth_ref import analytic_depth, smoke_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
VP, SMALL, AXIS = (200, 150), (67, 41), (65, 65)
CUBE = (32, 32)
NS, NL = 48, 16
ALBEDO = (0.8, 0.7, 0.6, 2.0)
OTHER = (0.1, 0.9, 0.3, 0.7)
CLEAR = (0.2, 0.4, 0.6, 0.5)
ALL_FIELDS = (fx.FIELD_VELOCITY, fx.FIELD_VELOCITY1, fx.FIELD_COLOR, fx.FIELD_COLOR_PREV, fx.FIELD_PRESSURE, fx.FIELD_DIVERGENCE)
LIGHTS = {"directional": {"kind": "directional", "position": (-30.0, 50.0, -20.0), "color": (0.2, 0.9, 0.5, 4.0), "ambient": (0.5, 0.4, 0.9, 0.7)},
          "point": {"kind": "point", "position": (2.0, 6.0, -7.0), "color": (1.0, 0.8, 0.6, 6.0)}}


def make(grid=CUBE, vp=VP, cam="default", light=None, mask=True, draw=ALBEDO, accel=1, frame=True, col=None):
    X, Z = grid
    f = fx.Fluid()
    assert f.Init(vp[0], vp[1], (X, X, Z)), f.last_status
    f.SetMaxSamples(NS, NL)
    f.set_option(capi.OPT_RENDER_ACCEL, accel)
    if col is not None:
        f.upload(fx.FIELD_COLOR, col)
    if frame:
        f.UpdateFrame(0.0, 0, *od.cameras(cam, *vp))
    if light is not None:
        f.SetLight(light["position"], light["kind"], light.get("color"), light.get("ambient"))
    if mask is True:
        f.SetObstacles(od.scene_mask(X, Z))
    elif mask is not None and mask is not False:
        f.SetObstacles(mask)
    if draw is not None:
        f.SetObstacleDraw(draw)
    return f


def model_frame(f, grid, vp, cam, light=None):
    view, proj, eye = od.cameras(cam, *vp)
    return od.frame(view, proj, eye, vp[0], vp[1], grid[0], wvp_i=np.array(list(f.frame_info().world_view_proj_i), f32), light=light)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def depth_buffer(f):
    """the depth-out buffer read through the device pointer"""
    W, H = f.viewport
    p = f.ObstacleDepthPointer()
    assert p
    f.Synchronize()
    out = np.empty((H, W), f32)
    hip_memcpy = capi.load().hipMemcpy                                    # (the HIP runtime the library links: found through the library's handle)
    hip_memcpy.argtypes, hip_memcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert hip_memcpy(out.ctypes.data, p, out.nbytes, 2) == 0             # hipMemcpyDeviceToHost
    return out


def cleared(f):
    f.ClearRenderTarget(CLEAR)
    f.Synchronize()
    return f.download(fx.FIELD_TARGET)


def check_picture(f, S, fr, vp, albedo=ALBEDO, scene=None, scene_dev=None):
    """clear, draw, compare everything the draw stores -> the model's draw"""
    pre = cleared(f)
    assert pre.any()
    f.DrawObstacles(0, scene_dev)
    f.Synchronize()
    want = od.draw(S, fr, vp[0], vp[1], albedo, pre, scene)
    tf, target, depth = f.download(fx.FIELD_TARGET_FLOAT), f.download(fx.FIELD_TARGET), depth_buffer(f)
    dr = want["cast"]["drawn"].reshape(vp[1], vp[0])
    print("picture: drawn %d, float words that differ %d, target bytes that differ %d, depth words that differ %d" % (
        int(dr.sum()), int((tf.view(np.uint32) != want["target_float"].view(np.uint32)).sum()), int((target != want["target"]).sum()),
        int((depth.view(np.uint32) != want["depth"].view(np.uint32)).sum())))
    assert same_bits(tf, want["target_float"])
    assert same_bits(target, want["target"])
    assert same_bits(depth, want["depth"])
    assert np.array_equal(target[~dr], pre[~dr])                          # pixels not drawn keep their bytes
    return want


# ---- 1: hits and depth against the model ---------------------------------------------------------------------------------------------------------
CASES = [(g, vp, cam) for g in (CUBE, (30, 18), (32, 16)) for vp in (VP, SMALL) for cam in ("default", "opposite", "inside")] + \
        [(g, AXIS, "axis") for g in (CUBE, (30, 18), (32, 16))]


@pytest.mark.parametrize("grid,vp,cam", CASES)
def test_hits_and_depth_are_the_models(grid, vp, cam):
    f = make(grid, vp, cam)
    want = od.draw(od.scene_mask(*grid), model_frame(f, grid, vp, cam), vp[0], vp[1], ALBEDO)
    hits, depth = f.ObstacleHits()
    C_ = want["cast"]
    print(grid, vp, cam, "rays %d hits %d drawn %d, words that differ %d, depth words that differ %d" % (
        int(C_["rays"]["ok"].sum()), int(C_["hit"].sum()), int(C_["drawn"].sum()), int((hits != want["hits"]).sum()),
        int((depth.view(np.uint32) != want["depth"].view(np.uint32)).sum())))
    assert C_["hit"].sum() > 100
    assert same_bits(hits, want["hits"])
    assert same_bits(depth, want["depth"])
    f.Release()


def test_the_eye_inside_a_solid_block_gives_face_code_6():
    vp, grid = SMALL, (30, 18)
    f = make(grid, vp, "inside", mask=None)
    fr = model_frame(f, grid, vp, "inside")
    q = od.local_point(fr, fr["eye"])
    x, y, z = [min(max(int(np.floor((float(q[a]) * 0.5 + 0.5) * n)), 0), n - 1) for a, n in enumerate((30, 30, 18))]
    S = od.scene_mask(*grid)
    S[max(z - 3, 0):z + 4, max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = True
    f.SetObstacles(S)
    want = check_picture(f, S, fr, vp)
    assert (want["cast"]["face"] == 6).all() and want["cast"]["start"].all()
    hits, depth = f.ObstacleHits()
    assert same_bits(hits, want["hits"]) and same_bits(depth, want["depth"])
    f.Release()


# ---- 2: the picture against the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", [None, "directional", "point", "on a hit"])
@pytest.mark.parametrize("grid,vp", [(CUBE, VP), ((30, 18), SMALL)])
def test_the_picture_is_the_models(grid, vp, light):
    S = od.scene_mask(*grid)
    if light == "on a hit":                                               # a point light exactly on a hit point: it casts no ray there
        f = make(grid, vp)
        C_ = od.cast(S, model_frame(f, grid, vp, "default"), vp[0], vp[1])
        f.Release()
        k = np.nonzero(C_["drawn"] & ~C_["start"])[0]
        p = C_["p"][k[len(k) // 2]]
        L = {"kind": "point", "position": tuple(float(v) for v in (p * f32(10)).astype(f32))}
    else:
        L = LIGHTS.get(light)
    f = make(grid, vp, light=L)
    want = check_picture(f, S, model_frame(f, grid, vp, "default", L), vp)
    assert want["cast"]["drawn"].sum() > 100
    lit = want["target_float"].reshape(-1, 4)[want["cast"]["drawn"]]
    # faces towards and away from the light differ (the reference's light (75, 75, -75) lights the three faces this camera sees alike)
    assert len(np.unique(lit.view(np.uint32), axis=0)) >= (1 if light is None else 3)
    f.Release()


# ---- 3: the caller's scene depth -------------------------------------------------------------------------------------------------------------------
def test_a_scene_depth_hides_the_hits_behind_it():
    import torch
    grid, vp = CUBE, VP
    S = od.scene_mask(*grid)
    f = make(grid, vp)
    fr = model_frame(f, grid, vp, "default")
    view, proj, eye = od.cameras("default", *vp)
    scene = analytic_depth(proj, vp[0], vp[1], plane=(0.3, 0.2, float(np.linalg.norm(eye))))
    dev = torch.from_numpy(scene).to("cuda:0")
    torch.cuda.synchronize()
    want = check_picture(f, S, fr, vp, scene=scene, scene_dev=dev)
    C_ = want["cast"]
    hidden, shown = int((C_["hit"] & ~C_["drawn"]).sum()), int(C_["drawn"].sum())
    print("hit %d hidden %d drawn %d" % (int(C_["hit"].sum()), hidden, shown))
    assert hidden >= 0.05 * C_["hit"].sum() and shown >= 0.05 * C_["hit"].sum()
    hits, depth = f.ObstacleHits(0, dev)
    assert same_bits(hits, want["hits"]) and same_bits(depth, want["depth"])
    hid = (C_["hit"] & ~C_["drawn"]).reshape(vp[1], vp[0])
    assert ((hits[hid] >> np.uint64(63)) == 1).all() and (((hits[hid] >> np.uint64(62)) & np.uint64(1)) == 0).all()
    assert np.array_equal(depth[hid], scene[hid])                         # depth-out = the plane's depth
    # the depth-out buffer itself is refused as the scene
    p = f.ObstacleDepthPointer()
    assert f._lib.fx_draw_obstacles(f._ctx, None, 0, C.c_void_p(p)) == capi.FX_E_INVALID
    f.Release()


# ---- 4: composition with the renders and the particle draw ------------------------------------------------------------------------------------------
_SMOKE = []


def smoke():
    if not _SMOKE:
        _SMOKE.append(smoke_scene(32))
    return _SMOKE[0]


def rendered(f, flags):
    f.Render(0, flags)
    if flags & fx.Fluid.RAY_MARCH_CUBEMAP:
        f.RenderCube(0)
    f.Synchronize()
    return f.download(fx.FIELD_TARGET), f.download(fx.FIELD_TARGET_FLOAT)


@pytest.mark.parametrize("flags", [fx.Fluid.RAY_MARCH_DIRECT, fx.Fluid.RAY_MARCH_CUBEMAP])
def test_the_attached_depth_ends_the_marches_at_the_solid(flags):
    a, b = make(col=smoke()), make(col=smoke())
    for f in (a, b):
        cleared(f)
        f.DrawObstacles(0)
    a.AttachObstacleDepth()
    depth = depth_buffer(a)
    assert (depth < 1).sum() > 2000
    b.SetSceneDepth(depth)                                                # the host form: the same values, copied
    ta, fa = rendered(a, flags)
    tb, fb = rendered(b, flags)
    assert same_bits(ta, tb) and same_bits(fa, fb)
    # without the depth the smoke behind the solids shows: more alpha in sum
    b.SetSceneDepth(None)
    cleared(b)
    b.DrawObstacles(0)
    _, free = rendered(b, flags)
    print("alpha with depth %.3f, without %.3f" % (float(fa[..., 3].sum()), float(free[..., 3].sum())))
    assert fa[..., 3].sum() < free[..., 3].sum()
    # a second frame on the same stream: the draw rewrites the buffer the renders read in place
    cleared(a)
    a.DrawObstacles(0)
    ta2, fa2 = rendered(a, flags)
    assert same_bits(ta2, ta) and same_bits(fa2, fa)
    a.SetSceneDepth(None)
    a.Release()
    b.Release()


def test_the_particle_draw_culls_what_lies_behind_the_solids():
    f = make()                                                            # no smoke: every particle's transmittance is 1
    f.DrawObstacles(0)
    f.AttachObstacleDepth()
    depth = depth_buffer(f)
    rec = pd.records(4099, 2.0)
    f.SetParticleParams(lifetime=2.0)
    f.SetParticles(rec)
    f.SetParticleDraw((1.0, 0.6, 0.2, 3.0))
    view, proj, eye = od.cameras("default", *VP)
    M = pd.forward_wvp(view, proj)
    P = pd.project(rec, M, VP[0], VP[1], depth)
    free = pd.project(rec, M, VP[0], VP[1])
    print("particles drawn %d of %d, hidden %d" % (int((P["cls"] == pd.DRAWN).sum()), int((free["cls"] == pd.DRAWN).sum()), int((P["cls"] == pd.HIDDEN).sum())))
    assert (P["cls"] == pd.HIDDEN).sum() > 100 and (P["cls"] == pd.DRAWN).sum() > 100
    got = f.ParticleSplats()
    assert np.array_equal(got, pd.splats(rec, P, np.ones(len(rec), f32), 2.0, VP[0], VP[1]))
    f.SetSceneDepth(None)
    assert np.array_equal(f.ParticleSplats(), pd.splats(rec, free, np.ones(len(rec), f32), 2.0, VP[0], VP[1]))
    f.Release()


# ---- 5: the mask changes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["mask", "meshes"])
def test_a_mask_set_between_two_draws_is_seen_by_the_second(how):
    grid, vp = (30, 18), VP
    dims = (30, 30, 18)
    f = make(grid, vp)
    fr = model_frame(f, grid, vp, "default")
    A = od.scene_mask(*grid)
    check_picture(f, A, fr, vp)
    if how == "mask":
        B = od.scene_mask(*grid, ball=False)
        B[2:9, 20:27, 3:11] = True
        f.SetObstacles(B)
    else:
        rep = f.SetObstacleMeshes([vr.box_mesh(vr.cell_centre(dims, (6, 5, 4)), vr.cell_centre(dims, (22, 24, 13))) + (None,),
                                   vr.uv_sphere((0.7, 0.75, 0.3), 0.17) + (None,)])
        assert rep["solid_cells"] > 500
        B = f.GetObstacles()[0] != 0
    assert not np.array_equal(A, B)
    want = check_picture(f, B, fr, vp)
    hits, depth = f.ObstacleHits()
    assert same_bits(hits, want["hits"]) and same_bits(depth, want["depth"])
    assert not np.array_equal(want["hits"], od.draw(A, fr, vp[0], vp[1], ALBEDO)["hits"])
    # an all-zero mask, then none: every word 0, the target untouched, depth 1.0 -- or the caller's scene depth
    import torch
    scene = analytic_depth(od.cameras("default", *vp)[1], vp[0], vp[1], plane=(0.3, 0.2, 40.0))
    dev = torch.from_numpy(scene).to("cuda:0")
    torch.cuda.synchronize()
    for mask in (np.zeros_like(A), None):
        f.SetObstacles(mask)
        for sc, sd in ((None, None), (scene, dev)):
            pre = cleared(f)
            f.DrawObstacles(0, sd)
            f.Synchronize()
            assert np.array_equal(f.download(fx.FIELD_TARGET), pre)
            assert not f.download(fx.FIELD_TARGET_FLOAT).view(np.uint32).any()
            assert same_bits(depth_buffer(f), np.ones((vp[1], vp[0]), f32) if sc is None else sc)
            hits, depth = f.ObstacleHits(0, sd)
            assert not hits.any() and same_bits(depth, np.ones((vp[1], vp[0]), f32) if sc is None else sc)
    f.SetObstacles(A)                                                     # ... and back
    check_picture(f, A, fr, vp)
    f.Release()


# ---- 6: the simulation is untouched ------------------------------------------------------------------------------------------------------------------
def test_the_draw_changes_nothing_of_the_simulation():
    rng = np.random.default_rng(12)
    vel = (rng.standard_normal((3, 32, 32, 32)) * 0.1).astype(f32)
    a, b = make(col=smoke()), make(col=smoke(), draw=None)
    for f in (a, b):
        f.upload(fx.FIELD_VELOCITY, vel)
    before = [a.digest(k) for k in ALL_FIELDS]
    mask = a.GetObstacles()
    cleared(a)
    a.DrawObstacles(0)
    a.ObstacleHits()
    a.Synchronize()
    assert [a.digest(k) for k in ALL_FIELDS] == before
    after = a.GetObstacles()
    assert np.array_equal(mask[0], after[0]) and mask[1] == after[1]
    for step in range(3):
        for f in (a, b):
            f.UpdateFrame(f.default_time_step(), 0, *od.cameras("default", *VP))
            f.Simulate(0)
        a.DrawObstacles(0)
        assert [a.digest(k) for k in ALL_FIELDS] == [b.digest(k) for k in ALL_FIELDS]
    a.Release()
    b.Release()


def test_render_accel_on_and_off_give_the_same_words():
    got = []
    for accel in (1, 0):
        f = make(accel=accel, col=smoke())
        cleared(f)
        f.Render(0, fx.Fluid.OPTIMIZED)                                   # a rendered frame: the render's side volumes are live
        f.Synchronize()
        got.append(f.ObstacleHits())
        f.Release()
    assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1]) and got[0][0].any()


# ---- 7: lifecycle ------------------------------------------------------------------------------------------------------------------------------------
def test_off_and_on_again_equals_a_fresh_context():
    S = od.scene_mask(*CUBE)
    f = make()
    fr = model_frame(f, CUBE, VP, "default")
    check_picture(f, S, fr, VP)
    f.SetObstacleDraw(None)
    assert f.GetObstacleDraw() == {"albedo": (0.0,) * 4, "flags": 0}
    assert f.ObstacleDepthPointer() is None
    assert f._lib.fx_draw_obstacles(f._ctx, None, 0, None) == capi.FX_E_STATE
    f.SetObstacleDraw(OTHER)
    assert f.GetObstacleDraw() == {"albedo": tuple(f32(v) for v in OTHER), "flags": 0}
    want = check_picture(f, S, fr, VP, OTHER)
    g = make(draw=OTHER)
    want2 = check_picture(g, S, fr, VP, OTHER)
    assert same_bits(want["target"], want2["target"])
    f.SetObstacleDraw(ALBEDO)                                             # a second set replaces the albedo and keeps drawing
    check_picture(f, S, fr, VP)
    f.Release()
    g.Release()


def test_a_draw_set_before_any_render_allocates_the_target():
    f = make()                                                            # no render, no clear: the setter allocated the target, zeroed
    f.DrawObstacles(0)
    f.Synchronize()
    want = od.draw(od.scene_mask(*CUBE), model_frame(f, CUBE, VP, "default"), VP[0], VP[1], ALBEDO)
    assert same_bits(f.download(fx.FIELD_TARGET), want["target"]) and same_bits(f.download(fx.FIELD_TARGET_FLOAT), want["target_float"])
    assert same_bits(depth_buffer(f), want["depth"])
    f.Release()


def test_the_draw_is_booked_as_resolve_time_and_not_as_a_render():
    f = make()
    f.timing_enable(True)
    f.DrawObstacles(0)
    f.Synchronize()
    t = f.timing_read()
    assert t.resolve_ms > 0 and t.renders == 0 and t.view_ms == 0
    f.Release()


# ---- 8: what is refused, and that it leaves the state in force ------------------------------------------------------------------------------------------
def struct_of(albedo=ALBEDO, size=None, flags=0):
    s = capi.ObstacleDraw()
    s.struct_size, s.flags = C.sizeof(capi.ObstacleDraw) if size is None else size, flags
    s.albedo = (C.c_float * 4)(*albedo)
    return s


def test_bad_arguments_are_refused_and_leave_the_state_in_force():
    S = od.scene_mask(*CUBE)
    f = make(draw=None)
    lib, ctx = f._lib, f._ctx
    W, H = VP
    hits, depth = np.zeros((H, W), np.uint64), np.zeros((H, W), f32)
    p64, pf = hits.ctypes.data_as(C.POINTER(C.c_uint64)), depth.ctypes.data_as(C.POINTER(C.c_float))
    # while the draw is off
    assert lib.fx_draw_obstacles(ctx, None, 0, None) == capi.FX_E_STATE
    assert lib.fx_obstacle_hits(ctx, None, 0, None, p64, pf, W * H) == capi.FX_E_STATE
    assert f.GetObstacleDraw() == {"albedo": (0.0,) * 4, "flags": 0}
    assert f.ObstacleDepthPointer() is None
    f.SetObstacleDraw(ALBEDO)
    fr = model_frame(f, CUBE, VP, "default")
    in_force = f.GetObstacleDraw()
    assert in_force == {"albedo": tuple(f32(v) for v in ALBEDO), "flags": 0}
    ptr = f.ObstacleDepthPointer()
    bad = [struct_of(size=20), struct_of(size=28), struct_of(flags=1), struct_of(flags=0x80000000)]
    for k in range(4):
        for v in (np.nan, np.inf, -np.inf, -1.0):
            a = list(OTHER)
            a[k] = v
            bad.append(struct_of(a))
    for s in bad:
        assert lib.fx_set_obstacle_draw(ctx, C.byref(s)) == capi.FX_E_INVALID
        assert f.GetObstacleDraw() == in_force and f.ObstacleDepthPointer() == ptr
    assert lib.fx_get_obstacle_draw(ctx, None) == capi.FX_E_INVALID
    assert lib.fx_obstacle_depth_device(ctx, None) == capi.FX_E_INVALID
    for n in (0, W * H - 1, W * H + 1, W * H * 2):
        assert lib.fx_obstacle_hits(ctx, None, 0, None, p64, pf, n) == capi.FX_E_INVALID
    assert lib.fx_draw_obstacles(ctx, None, capi.FRAME_COUNT, None) == capi.FX_E_INVALID
    assert lib.fx_obstacle_hits(ctx, None, capi.FRAME_COUNT, None, p64, pf, W * H) == capi.FX_E_INVALID
    assert lib.fx_draw_obstacles(ctx, None, 0, C.c_void_p(ptr)) == capi.FX_E_INVALID
    assert lib.fx_obstacle_hits(ctx, None, 0, C.c_void_p(ptr), p64, pf, W * H) == capi.FX_E_INVALID
    out, dp = capi.ObstacleDraw(), C.c_void_p()
    for fn, args in (("fx_set_obstacle_draw", (None,)), ("fx_get_obstacle_draw", (C.byref(out),)), ("fx_draw_obstacles", (None, 0, None)),
                     ("fx_obstacle_depth_device", (C.byref(dp),)), ("fx_obstacle_hits", (None, 0, None, p64, pf, W * H))):
        assert getattr(lib, fn)(None, *args) == capi.FX_E_INVALID
    assert f.GetObstacleDraw() == in_force
    assert lib.fx_obstacle_hits(ctx, None, 0, None, None, None, W * H) == capi.FX_OK      # either host pointer may be NULL
    assert lib.fx_obstacle_hits(ctx, None, 0, None, p64, None, W * H) == capi.FX_OK
    want = check_picture(f, S, fr, VP)                                    # ... and the draw still draws
    assert same_bits(hits, want["hits"])
    f.Release()
    ok = struct_of()
    # before any fx_update_frame gave a camera: refused the way fx_render refuses it
    g = make(frame=False)
    assert g._lib.fx_draw_obstacles(g._ctx, None, 0, None) == capi.FX_E_STATE
    assert g._lib.fx_obstacle_hits(g._ctx, None, 0, None, p64, pf, W * H) == capi.FX_E_STATE
    assert g._lib.fx_render(g._ctx, None, 0, 0) == capi.FX_E_STATE
    g.Release()
    # contexts that cannot draw: a 2-D grid, no viewport, a slab (the getters report the default there), render-only
    default = {"albedo": (0.0,) * 4, "flags": 0}
    flat = fx.Fluid()
    assert flat.Init(64, 64, (32, 32, 1))
    blind = fx.Fluid()
    assert blind.Init(0, 0, (32, 32, 32))
    slab = fx.Fluid()
    assert slab.Init(0, 0, (32, 32, 32), slab=(0, 12), halo_advect=6, halo_jacobi=2)
    for c, n in ((flat, 64 * 64), (blind, 0), (slab, 0)):
        assert c._lib.fx_set_obstacle_draw(c._ctx, C.byref(ok)) == capi.FX_E_INVALID
        assert c._lib.fx_set_obstacle_draw(c._ctx, None) == capi.FX_E_INVALID
        assert c._lib.fx_draw_obstacles(c._ctx, None, 0, None) == capi.FX_E_INVALID
        assert c._lib.fx_obstacle_hits(c._ctx, None, 0, None, p64, pf, n) == capi.FX_E_INVALID
        assert c.GetObstacleDraw() == default and c.ObstacleDepthPointer() is None
        c.Release()
    ro = fx.Fluid()
    assert ro.Init(W, H, (32, 32, 32), render_only=True)
    assert ro._lib.fx_set_obstacle_draw(ro._ctx, C.byref(ok)) == capi.FX_E_STATE
    assert ro._lib.fx_get_obstacle_draw(ro._ctx, C.byref(out)) == capi.FX_E_STATE
    assert ro._lib.fx_draw_obstacles(ro._ctx, None, 0, None) == capi.FX_E_STATE
    assert ro._lib.fx_obstacle_depth_device(ro._ctx, C.byref(dp)) == capi.FX_E_STATE
    assert ro._lib.fx_obstacle_hits(ro._ctx, None, 0, None, p64, pf, W * H) == capi.FX_E_STATE
    ro.Release()
