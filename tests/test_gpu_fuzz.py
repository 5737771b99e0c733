"""Seeded random-configuration parity tests: the hand-picked shapes of test_gpu_sim.py / test_gpu_slabs.py cover the
cases the reference's defaults hit; these draw grid extents, storage, addressing, sweep counts / modes, fusion, slab cuts,
halo widths and schedules at random (fixed seeds, so a failure reproduces) and hold the same bars:
  * one full step from a random state: HIP vs oracle (bit-exact where no transcendental is on the path);
  * random z-slab decompositions vs the single-domain HIP run: bit-identical.
No optional setter is called here: the trajectories of the optional stages are held by tests/test_gpu_step_model.py against tests/step_ref.py."""
import os

import numpy as np
import pytest

import fluidx12_amd as fx
from fluidx12_amd import capi
from oracle import orc

pytestmark = pytest.mark.gpu
f32 = np.float32
# FLUIDX_FUZZ_SEEDS=N widens every seed range to N (a soak run; the default ranges run in seconds)
SOAK = int(os.environ.get("FLUIDX_FUZZ_SEEDS", "0"))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.sqrt((b ** 2).sum())
    d = np.sqrt(((a - b) ** 2).sum())
    return d / n if n > 0 else d


def draw_single(seed):
    rng = np.random.default_rng(1000 + seed)
    S = int(rng.choice([8, 12, 20, 24, 32, 36, 44, 52, 64, 72, 100, 128]))
    Z = 1 if rng.random() < 0.2 else int(rng.integers(2, 41))
    return dict(dims=(S, S, Z), storage=str(rng.choice(["fp32", "fp16"])), address=str(rng.choice(["clamp", "mirror"])),
                mode=str(rng.choice(["fixed", "faithful"])), iters=int(rng.integers(1, 25)), fuse=int(rng.choice([0, 1, 2, 3, 4])),
                scale=float(rng.choice([0.2, 1.0, 3.0])), rng=rng)


def draw_wide(seed):
    """rows of 256 cells and more, a few planes deep: the four-sweep band kernels on thin ranges (k_jacobi_strip4o from six planes,
    k_jacobi_strip4t's x tiles -- 512 cells as three of them below 96 planes --, chunks of four planes, remainders in threes, twos, ones)"""
    rng = np.random.default_rng(9000 + seed)
    S = int(rng.choice([256, 256, 260, 264, 288, 320, 384, 512, 512, 516]))
    Z = 1 if rng.random() < 0.12 else int(rng.integers(2, 25))
    return dict(dims=(S, S, Z), storage=str(rng.choice(["fp32", "fp16"])), address=str(rng.choice(["clamp", "mirror"])),
                mode=str(rng.choice(["fixed", "fixed", "faithful"])), iters=int(rng.integers(1, 18)), fuse=int(rng.choice([0, 0, 1, 2, 3, 4])),
                scale=float(rng.choice([0.2, 1.0, 3.0])), rng=rng)


def draw_deep(seed):
    """... and 40 to 110 planes deep: where the launchers change their minds (X = 512 as three tiles up to 96 planes, runs or the octet's
    grid of whole pieces by the planes per CU, z chunks by the depth)"""
    rng = np.random.default_rng(11000 + seed)
    S = int(rng.choice([192, 224, 252, 256, 264, 320, 384, 512]))              # (192..252: one tile with its upper lanes off, from 3.1 M cells)
    Z = int(rng.integers(40, 111))
    return dict(dims=(S, S, Z), storage="fp32", address=str(rng.choice(["clamp", "mirror"])), mode="fixed", iters=int(rng.integers(4, 10)),
                fuse=int(rng.choice([0, 0, 0, 4])), scale=float(rng.choice([0.2, 1.0])), rng=rng)


@pytest.mark.parametrize("seed", range(SOAK // 40 or 6))
def test_random_deep_wide_step_matches_oracle(seed):
    check_random_step(draw_deep(seed))


@pytest.mark.parametrize("seed", range(SOAK // 8 or 10))
def test_random_wide_step_matches_oracle(seed):
    check_random_step(draw_wide(seed))


@pytest.mark.parametrize("seed", range(SOAK or 24))
def test_random_step_matches_oracle(seed):
    check_random_step(draw_single(seed))


def check_random_step(c):
    X, Y, Z = c["dims"]
    rng = c["rng"]
    half = c["storage"] == "fp16"
    vel = (rng.standard_normal((3, Z, Y, X)) * c["scale"]).astype(f32)
    col = rng.random((Z, Y, X, 4)).astype(f32)
    p0 = rng.standard_normal((Z, Y, X)).astype(f32)
    if Z == 1:
        vel[2] = 0
    if half:                                               # the state must be storable
        vel, col = vel.astype(np.float16).astype(f32), col.astype(np.float16).astype(f32)
    f = fx.Fluid()
    assert f.Init(800, 800, c["dims"], storage=c["storage"], advect_address=c["address"], jacobi_mode=c["mode"],
                  jacobi_iters=c["iters"], jacobi_fuse=c["fuse"]), (c, f.last_status)
    f.upload(fx.FIELD_VELOCITY, vel)
    f.upload(fx.FIELD_COLOR, col)
    f.upload(fx.FIELD_PRESSURE, p0)
    s = orc.Sim(X, Y, Z, iters=c["iters"], mode=int(c["mode"] == "faithful"), address=int(c["address"] == "mirror"), half=half)
    s.vel[0][:] = vel
    s.col[s.parity][:] = col
    s.p[:] = p0
    dt = f32(f.default_time_step())
    for k in range(2):
        f.UpdateFrame(dt, k)
        f.Simulate(k)
        s.step()
        if k == 0 and half:
            # one step: the only freedom is the exp2 ulp inside the impulse ball flipping the binary16 rounding of a stored
            # value (measured over 1000 seeds: 999 within 1e-5, one at 1.5e-5); the conversion itself is a separate RNE
            # step on both sides -- a fused multiply-convert (v_fma_mixlo_f16) was what this test caught
            f.Synchronize()
            assert rel_l2(f.download(fx.FIELD_VELOCITY), s.velocity) < 1e-4, c
            assert rel_l2(f.download(fx.FIELD_COLOR), s.color) < 1e-4, c
    f.Synchronize()
    gv, gc, gp = f.download(fx.FIELD_VELOCITY), f.download(fx.FIELD_COLOR), f.download(fx.FIELD_PRESSURE)
    # two steps: a flipped half moves the second step's back-trace and, in faithful mode, freeze decisions
    tol = 1e-3 if half else 1e-5
    assert np.isfinite(gv).all() and np.isfinite(gc).all() and np.isfinite(gp).all(), c
    assert rel_l2(gv, s.velocity) < tol, c
    assert rel_l2(gc, s.color) < tol, c
    assert rel_l2(gp, s.p) < tol, c
    assert f.frame_info().frame_parity == s.parity
    if half:
        assert np.array_equal(gv.astype(np.float16).astype(f32), gv)


def draw_slabs(seed):
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(2, 5))
    hj = int(rng.integers(1, 9))
    ha = int(rng.integers(6, 13))
    H = max(hj, ha)
    # uneven cuts, every slab at least H planes (a halo may only span the direct neighbour)
    sizes = [H + int(rng.integers(0, 20)) for _ in range(n)]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    # X = Y >= Z keeps the z reach (|v_z| * dt * Z = 2 |v_z| Z / Y cells) inside the 6..12-plane advect halo for these few steps
    S = max(32, (int(cuts[-1]) + 3) // 4 * 4)
    if rng.random() < 0.5:
        S = 1 << int(np.ceil(np.log2(S)))                 # power-of-two extents take the fast advect / strip Jacobi kernels
    return dict(dims=(S, S, int(cuts[-1])), slabs=[(int(cuts[i]), int(sizes[i])) for i in range(n)], hj=hj, ha=ha,
                storage=str(rng.choice(["fp32", "fp16"])), mode=str(rng.choice(["fixed", "fixed", "faithful"])),
                iters=int(rng.integers(2, 21)), fuse=int(rng.choice([0, 1, 2, 3, 4])), overlap=int(rng.integers(0, 4)),
                rnd=int(rng.integers(1, hj + 1)), steps=int(rng.integers(2, 5)))


def draw_wide_slabs(seed):
    """... on rows of 256 cells and more: thin slabs whose rounds run the four-sweep band kernels on shrinking ranges of a few planes"""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(2, 4))
    hj = int(rng.integers(1, 9))
    ha = int(rng.integers(6, 11))
    H = max(hj, ha)
    sizes = [H + int(rng.integers(0, 12)) for _ in range(n)]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    S = int(rng.choice([256, 264, 320, 512]))
    return dict(dims=(S, S, int(cuts[-1])), slabs=[(int(cuts[i]), int(sizes[i])) for i in range(n)], hj=hj, ha=ha,
                storage=str(rng.choice(["fp32", "fp16"])), mode=str(rng.choice(["fixed", "fixed", "fixed", "faithful"])),
                iters=int(rng.integers(2, 21)), fuse=int(rng.choice([0, 0, 1, 2, 3, 4])), overlap=int(rng.integers(0, 4)),
                rnd=int(rng.integers(1, hj + 1)), steps=int(rng.integers(2, 4)))


@pytest.mark.parametrize("seed", range(SOAK // 8 or 10))
def test_random_wide_slab_decomposition_is_bit_identical(seed):
    check_random_slabs(draw_wide_slabs(seed))


@pytest.mark.parametrize("seed", range(SOAK or 24))
def test_random_slab_decomposition_is_bit_identical(seed):
    check_random_slabs(draw_slabs(seed))


def check_random_slabs(c):
    kw = dict(storage=c["storage"], jacobi_mode=c["mode"], jacobi_iters=c["iters"])
    ref = fx.Fluid()
    assert ref.Init(800, 800, c["dims"], jacobi_fuse=1, **kw), (c, ref.last_status)
    fl = []
    for z0, nz in c["slabs"]:
        f = fx.Fluid()
        assert f.Init(800, 800, c["dims"], slab=(z0, nz), halo_advect=c["ha"], halo_jacobi=c["hj"], jacobi_fuse=c["fuse"], **kw), (c, f.last_status)
        fl.append(f)
    fx.comm_init_local(fl)
    for f in fl:
        f.set_option(capi.OPT_OVERLAP, c["overlap"])
        f.set_option(capi.OPT_JACOBI_ROUND, c["rnd"])
    dt = f32(ref.default_time_step())
    rng2 = np.random.default_rng(c["hj"] * 131 + c["iters"] * 17 + c["dims"][2])
    for k in range(c["steps"]):
        if k and rng2.random() < 0.5:                      # the schedule is an option at run time: whatever the steps before left behind must serve the next one
            o2, r2 = int(rng2.integers(0, 4)), int(rng2.integers(1, c["hj"] + 1))
            for f in fl:
                f.set_option(capi.OPT_OVERLAP, o2)
                f.set_option(capi.OPT_JACOBI_ROUND, r2)
        ref.UpdateFrame(dt, k % 3)
        ref.Simulate(k % 3)
        fl[0].UpdateFrame(dt, k % 3)
        fl[0].Simulate(k % 3)
    ref.Synchronize()
    fl[0].Synchronize()                                   # raises FX_E_HALO if a back-trace left the exchanged planes
    for field, axis in ((fx.FIELD_VELOCITY, 1), (fx.FIELD_COLOR, 0), (fx.FIELD_PRESSURE, 0)):
        got = np.concatenate([f.download(field) for f in fl], axis=axis)
        want = ref.download(field)
        assert want.any(), c
        assert np.array_equal(got, want), (c, field)


# ---- random cameras / viewports / sample counts through every Render() mode ------------------------------------------------
_STATE = {}


def density(X):
    if X not in _STATE:
        s = orc.Sim(X, X, X, iters=20)
        for _ in range(8):
            s.step()
        rng = np.random.default_rng(X)
        z, y, x = np.meshgrid(*(np.arange(X),) * 3, indexing="ij")
        blob = np.exp(-(((x - X * .55) ** 2 + (y - X * .5) ** 2 + (z - X * .45) ** 2) / (X * .22) ** 2)).astype(f32)
        col = s.color + (blob[..., None] * rng.random((X, X, X, 4)) * np.array([.3, .5, .8, .6])).astype(f32)
        _STATE[X] = np.clip(col, 0, 1).astype(f32)
    return _STATE[X]


def draw_camera(seed):
    rng = np.random.default_rng(9000 + seed)
    X = int(rng.choice([16, 24, 32]))
    d = rng.standard_normal(3)
    if rng.random() < 0.25:                                # straight down an axis: the degenerate cases of the face culling
        d = np.eye(3)[int(rng.integers(0, 3))] * rng.choice([-1.0, 1.0]) + rng.standard_normal(3) * 1e-3
    d /= np.linalg.norm(d)
    eye = (d * rng.choice([6.0, 14.0, 25.0, 43.0, 90.0])).astype(f32)          # the volume is the cube |x| <= 10 (Fluid.cpp:171); 6 = an eye inside it
    up = np.array([0, 1, 0], f32) if abs(d[1]) < 0.9 else np.array([0, 0, 1], f32)
    focus = (rng.standard_normal(3) * 2.0).astype(f32)
    vp = [(160, 120), (200, 150), (320, 200), (128, 256)][int(rng.integers(0, 4))]
    flags = int(rng.choice([fx.Fluid.OPTIMIZED, fx.Fluid.RAY_MARCH_CUBEMAP, fx.Fluid.SEPARATE_LIGHT_PASS, fx.Fluid.RAY_MARCH_DIRECT]))
    return dict(X=X, eye=eye, up=up, focus=focus, vp=vp, flags=flags, use_sh=bool(rng.random() < 0.4), storage=str(rng.choice(["fp32", "fp16"])),
                samples=(int(rng.choice([32, 48, 96, 192])), int(rng.choice([8, 16, 64]))),
                fov=float(rng.choice([np.pi / 4, np.pi / 3, np.pi / 6])), rng=rng)


@pytest.mark.parametrize("seed", range(SOAK or 40))
def test_random_camera_render_matches_oracle(seed):
    c = draw_camera(seed)
    X, (vw, vh), col = c["X"], c["vp"], density(c["X"])
    if c["storage"] == "fp16":
        col = col.astype(np.float16).astype(f32)               # what a fp16-storage context holds after the upload
    view = fx.look_at_lh(c["eye"], c["focus"], c["up"])
    proj = fx.perspective_fov_lh(f32(c["fov"]), vw / float(vh), 1.0, 1000.0)
    sh = (c["rng"].random((9, 3)) * np.array([[2.0]] + [[0.5]] * 8)).astype(f32) if c["use_sh"] else None
    f = fx.Fluid()
    assert f.Init(vw, vh, (X, X, X), storage=c["storage"])
    f.SetMaxSamples(*c["samples"])
    if sh is not None:
        f.SetSH(sh)
    f.upload(fx.FIELD_COLOR, col)
    f.UpdateFrame(0.0, 0, view, proj, c["eye"])
    fr, lod, rs, mask, _ = orc.update_frame(view, proj, c["eye"], vw, vh, X, c["samples"][0])
    fi = f.frame_info()
    assert (fi.cube_lod, fi.ray_samples, fi.visibility_mask) == (lod, rs, mask), c
    if sh is not None:
        for i, v in enumerate(sh.reshape(27)):
            fr.sh[i] = v
    nl = c["samples"][1]
    separate = bool(c["flags"] & fx.Fluid.SEPARATE_LIGHT_PASS)
    lm = orc.raymarch_light(col, fr, nl, c["use_sh"], 2) if separate else None
    f.ClearRenderTarget()
    f.Render(0, c["flags"])
    f.Synchronize()
    if c["flags"] & fx.Fluid.RAY_MARCH_CUBEMAP:
        _, cu = orc.raymarch_view(col, lm, fr, X >> lod, mask, rs, nl, c["use_sh"], separate)
        cube = f.download(fx.FIELD_CUBEMAP)
        d = np.abs(cube.astype(np.int32) - cu.astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() <= 0.02, (c, int(d.max()), float((d > 0).mean()))
        assert cu[..., 3].max() > 20, c
    else:
        wvp_i = np.array(list(fi.world_view_proj_i), f32).reshape(4, 4)
        out, cov = orc.raycast_direct(col, lm, fr, wvp_i, vw, vh, rs if separate else c["samples"][0], nl, c["use_sh"], separate)
        got = f.download(fx.FIELD_TARGET_FLOAT)
        if separate:
            assert np.mean(got != out) < 5e-3 and np.abs(got - out).max() < 0.05, (c, float(np.mean(got != out)), float(np.abs(got - out).max()))
        else:
            assert np.mean(got != out) < 1e-4 and np.abs(got - out).max() < 1e-5, (c, float(np.mean(got != out)), float(np.abs(got - out).max()))


@pytest.mark.parametrize("seed", range(SOAK or 24))
def test_random_camera_resolve_and_sky_match_oracle(seed):
    """cube map -> screen resolve (PSRayCastCube) of a fully random cube map and the sky pass (PSEnvironment) of a random
    radiance cube under the random cameras: SV_TARGET bit for bit, the blended RGBA8 target exactly"""
    c = draw_camera(seed)
    rng = c["rng"]
    (vw, vh) = c["vp"]
    N = int(rng.choice([8, 16, 32]))
    view = fx.look_at_lh(c["eye"], c["focus"], c["up"])
    proj = fx.perspective_fov_lh(f32(c["fov"]), vw / float(vh), 1.0, 1000.0)
    f = fx.Fluid()
    assert f.Init(vw, vh, (N, N, N))
    f.UpdateFrame(0.0, 0, view, proj, c["eye"])
    fi = f.frame_info()
    fr = orc.update_frame(view, proj, c["eye"], vw, vh, N, 192)[0]
    S = fi.cube_size
    cube = rng.integers(0, 256, (6, S, S, 4), dtype=np.uint8)
    f.upload(fx.FIELD_CUBEMAP, cube)
    wvp_i = np.array(list(fi.world_view_proj_i), f32).reshape(4, 4)
    out, cov = orc.resolve_cube(cube, fr, wvp_i, vw, vh)
    rgba = (float(rng.random()), float(rng.random()), float(rng.random()), 0.0)
    f.ClearRenderTarget(rgba)
    f.RenderCube(0)
    f.Synchronize()
    assert np.array_equal(f.download(fx.FIELD_TARGET_FLOAT).view(np.uint32), out.view(np.uint32)), c
    target = np.empty((vh, vw, 4), np.uint8)
    target[...] = [int(np.floor(f32(min(max(v, 0.0), 1.0)) * f32(255) + f32(0.5))) for v in rgba]
    assert np.array_equal(f.download(fx.FIELD_TARGET), orc.blend_premultiplied(out, cov, target)), c
    # sky
    M = int(rng.choice([4, 16, 33]))
    sky = (rng.random((6, M, M, 3)) ** 3 * 4.0).astype(f32)
    f.SetEnvironment(sky)
    f.RenderEnvironment(0)
    f.Synchronize()
    s2w = np.array(list(fi.screen_to_world), f32).reshape(4, 4)
    want = orc.environment(sky, c["eye"], s2w, vw, vh)
    assert np.array_equal(f.download(fx.FIELD_TARGET_FLOAT).view(np.uint32), want.view(np.uint32)), c


@pytest.mark.parametrize("seed", range(SOAK or 12))
def test_random_sh_projection_matches_oracle(seed):
    rng = np.random.default_rng(12000 + seed)
    n = int(rng.choice([4, 8, 16, 24, 32, 64, 100, 128]))
    cube = (rng.random((6, n, n, 3)) ** 2 * 3.0).astype(f32)
    f = fx.Fluid()
    assert f.Init(64, 64, (16, 16, 16))
    probe = fx.LightProbe(f)
    probe.Init(cube)
    probe.TransformSH()
    got = np.asarray(probe.GetSH(), f32).reshape(9, 3)
    want = np.asarray(orc.sh_transform(cube), f32).reshape(9, 3)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (n, float(np.abs(got - want).max()))


@pytest.mark.parametrize("seed", range(SOAK or 12))
def test_random_call_sequences_leave_the_simulation_alone(seed, tmp_path):
    """API state machine: one context runs its simulation steps interleaved with a random mix of everything else the ABI offers
    (renders in every mode, sky, resolve, downloads, timing on/off, sample counts, SH on/off, a checkpoint save + reload of its
    own state, paused frames); a second context runs the steps alone.  The fields must come out bit-identical."""
    rng = np.random.default_rng(20000 + seed)
    X = int(rng.choice([16, 24, 32]))
    storage = str(rng.choice(["fp32", "fp16"]))
    vp = [(96, 64), (160, 120), (64, 96)][int(rng.integers(0, 3))]
    kw = dict(storage=storage, jacobi_iters=int(rng.integers(2, 12)), jacobi_mode=str(rng.choice(["fixed", "faithful"])))
    a, b = fx.Fluid(), fx.Fluid()
    assert a.Init(vp[0], vp[1], (X, X, X), **kw) and b.Init(vp[0], vp[1], (X, X, X), **kw)
    view, proj, eye = fx.default_camera(*vp)
    dt = f32(a.default_time_step())
    sky = (rng.random((6, 8, 8, 3)) * 2).astype(f32)
    ck = str(tmp_path / "state.fxck")
    for f in (a, b):
        f.UpdateFrame(0.0, 0, view, proj, eye)                 # Render / RenderEnvironment before the first frame are call-order errors
    steps = 0
    for op in rng.integers(0, 12, size=40):
        k = steps % 3
        if op <= 3:                                            # a simulation step on both
            for f in (a, b):
                f.UpdateFrame(dt, k, view, proj, eye)
                f.Simulate(k)
            steps += 1
        elif op == 4:
            a.UpdateFrame(0.0, k, view, proj, eye)             # paused frame: velocity copied, nothing else moves
            a.Simulate(k)
            b.UpdateFrame(0.0, k, view, proj, eye)
            b.Simulate(k)
        elif op == 5:
            a.SetMaxSamples(int(rng.integers(8, 64)), int(rng.integers(4, 32)))
            a.ClearRenderTarget()
            a.Render(k, int(rng.integers(0, 4)), to_target=bool(rng.integers(0, 2)))
        elif op == 6:
            a.SetSH((rng.random((9, 3)) * 0.5).astype(f32) if rng.random() < 0.7 else None)
        elif op == 7:
            a.SetEnvironment(sky)
            a.ClearRenderTarget()
            a.RenderEnvironment(k)
            a.RenderCube(k)
        elif op == 8:
            a.timing_enable(bool(rng.integers(0, 2)))
            a.timing_read(bool(rng.integers(0, 2)))
        elif op == 9:
            a.download(int(rng.choice([fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE, fx.FIELD_VELOCITY1, fx.FIELD_DIVERGENCE])))
        elif op == 10:
            a.SaveCheckpoint(ck)
            a.LoadCheckpoint(ck)                               # its own state back in: a no-op for the fields
        else:
            a.Synchronize()
    a.Synchronize()
    b.Synchronize()
    for field in (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE):
        assert np.array_equal(a.download(field), b.download(field)), (seed, field)


@pytest.mark.parametrize("seed", range(SOAK or 40))
def test_random_descriptors_fail_cleanly_or_work(seed):
    """fx_create with random descriptors -- half of them deliberately broken (zero / unequal extents, unknown enum values,
    slabs outside the grid or thinner than their halo, wrong struct size, unknown flags): every call returns FX_OK or a negative
    status and leaves no context behind on failure; what it accepts can step, render, report and be destroyed"""
    import ctypes as C
    rng = np.random.default_rng(30000 + seed)
    lib = capi.load()
    pick = lambda good, bad, p=0.85: int(rng.choice(good) if rng.random() < p else rng.choice(bad))
    d = capi.Desc()
    d.struct_size = pick([C.sizeof(capi.Desc)], [0, 4, C.sizeof(capi.Desc) - 4, C.sizeof(capi.Desc) + 8], 0.95)
    S = pick([4, 8, 12, 20, 32, 36, 64, 100], [0, 1, 2, 3, 5, 7, 65536, 1 << 20, 0xFFFFFFFC, 0xFFFFFFFF])
    d.grid_x, d.grid_y = S, (S if rng.random() < 0.9 else (S + 4) & 0xFFFFFFFF)
    d.grid_z = pick([1, 2, 3, 8, 17, 32, 40], [0, 1 << 24, 0xFFFFFFFF])
    d.viewport_w, d.viewport_h = pick([16, 64, 200], [0, 1 << 20]), pick([16, 48, 150], [0, 1 << 20])
    d.storage, d.jacobi_mode, d.advect_address = pick([0, 1], [2, 7, 255]), pick([0, 1], [2, 9]), pick([0, 1], [2, 3])
    d.jacobi_iters = pick([1, 2, 5, 20, 64], [0])
    d.device = pick([-1, 0], [1, 7, -2, 99], 0.9)
    if rng.random() < 0.35:
        d.slab_z0, d.slab_nz = int(rng.integers(0, 45)), int(rng.integers(0, 45))
        d.halo_advect, d.halo_jacobi = int(rng.integers(0, 12)), int(rng.integers(0, 12))
    d.flags = int(rng.integers(0, 5)) | (0x10 if rng.random() < 0.2 else 0) | (0x20 if rng.random() < 0.15 else 0) | (int(rng.integers(1, 1 << 20)) << 8 if rng.random() < 0.1 else 0)
    ctx = C.c_void_p()
    rc = lib.fx_create(C.byref(ctx), C.byref(d))
    assert rc in (capi.FX_OK, capi.FX_E_INVALID, capi.FX_E_DEVICE, capi.FX_E_NOMEM, capi.FX_E_STATE), rc
    if rc != capi.FX_OK:
        assert not ctx.value
        return
    try:
        whole = d.slab_nz == 0 or (d.slab_z0 == 0 and d.slab_nz == d.grid_z)
        view, proj, eye = fx.default_camera(max(d.viewport_w, 1), max(d.viewport_h, 1))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        v, p_, e = (np.ascontiguousarray(m, f32) for m in (view, proj, eye))
        assert lib.fx_update_frame(ctx, C.c_float(1.0 / max(d.grid_y, 1)), 0, fp(v), fp(p_), fp(e)) == capi.FX_OK
        rc = lib.fx_simulate(ctx, None, 0)
        giant = d.grid_x * d.grid_y * d.grid_z > 5e7                                  # 16 M planes of 4 x 4: fx_create fits, a lazily allocated scratch may not
        assert rc == (capi.FX_E_STATE if d.flags & 0x20 else capi.FX_OK) or (giant and rc == capi.FX_E_NOMEM), "rc %d desc %s" % (rc, " ".join(str(getattr(d, n)) for n, _ in capi.Desc._fields_))   # render-only contexts do not simulate
        if rc == capi.FX_E_NOMEM:
            return
        if whole and d.grid_z > 1:
            rflags = int(rng.integers(0, 4))
            rc = lib.fx_render(ctx, None, 0, rflags)
            no_viewport = d.viewport_w == 0 or d.viewport_h == 0       # a simulate-only context: rendering is an argument error
            huge_viewport = d.viewport_w >= (1 << 20) or d.viewport_h >= (1 << 20)
            if huge_viewport and not no_viewport:
                assert rc in (capi.FX_OK, capi.FX_E_NOMEM, capi.FX_E_DEVICE, capi.FX_E_INVALID), rc     # a 16-TB target cannot be allocated
            else:
                assert rc == (capi.FX_E_INVALID if no_viewport else capi.FX_OK), (rc, rflags, [getattr(d, n) for n, _ in capi.Desc._fields_])
        rc = lib.fx_synchronize(ctx)
        assert rc in (capi.FX_OK, capi.FX_E_HALO), rc       # a lone slab context has no neighbour data: its halo check may fire
        fi = capi.FrameInfo()
        assert lib.fx_get_frame_info(ctx, C.byref(fi)) == capi.FX_OK
        assert lib.fx_field_bytes(ctx, 99) == 0 and lib.fx_download(ctx, 99, C.byref(fi), 4) < 0
    finally:
        assert lib.fx_destroy(ctx) == capi.FX_OK


@pytest.mark.parametrize("seed", range(SOAK or 40))
def test_mutated_dds_files_never_crash_the_decoder(seed):
    """the DDS / BC6H container parser on damaged input: random byte flips in the header, truncation, absurd sizes and mip
    counts -- fx_dds_cube_info / fx_dds_decode_cube either succeed with consistent sizes or return a negative status"""
    import ctypes as C
    import os
    rng = np.random.default_rng(40000 + seed)
    data = bytearray(open(os.path.join(os.path.dirname(__file__), "..", "examples", "data", "probe_32.dds"), "rb").read())
    kind = int(rng.integers(0, 6))
    if kind == 0:                                              # flip bytes in the 148-byte header
        for _ in range(int(rng.integers(1, 6))):
            data[int(rng.integers(0, 148))] = int(rng.integers(0, 256))
    elif kind == 1:                                            # truncate anywhere
        data = data[:int(rng.integers(0, len(data)))]
    elif kind == 2:                                            # huge / zero extents and mip counts
        for off in (12, 16, 28):
            if rng.random() < 0.6:
                data[off:off + 4] = int(rng.choice([0, 1, 3, 1 << 16, 1 << 30, 0xFFFFFFFF])).to_bytes(4, "little")
    elif kind == 3:                                            # payload garbage (every block decodes to something)
        for _ in range(64):
            data[int(rng.integers(148, len(data)))] = int(rng.integers(0, 256))
    lib = capi.load()
    f = fx.Fluid()
    assert f.Init(64, 64, (16, 16, 16))
    buf = (C.c_char * max(len(data), 1)).from_buffer_copy(bytes(data) if len(data) else b"\0")
    size, mips = C.c_uint32(), C.c_uint32()
    rc = lib.fx_dds_cube_info(buf, len(data), C.byref(size), C.byref(mips))
    assert rc <= 0
    if rc != capi.FX_OK:
        out = np.zeros(6 * 4 * 4 * 3, f32)
        assert lib.fx_dds_decode_cube(f._ctx, buf, len(data), 0, out.ctypes.data_as(C.POINTER(C.c_float)), out.size) < 0
        return
    assert 1 <= size.value <= 16384 and 1 <= mips.value <= 15
    mip = int(rng.integers(0, mips.value + 2))
    n = max(size.value >> mip, 1)
    if 6 * n * n * 3 > (1 << 26):
        return
    out = np.zeros(6 * n * n * 3, f32)
    rc = lib.fx_dds_decode_cube(f._ctx, buf, len(data), mip, out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
    assert rc == capi.FX_OK or rc < 0
    if mip >= mips.value:
        assert rc < 0
    if rc == capi.FX_OK and kind == 4:
        assert np.isfinite(out).all()


@pytest.mark.parametrize("seed", range(SOAK or 24))
def test_damaged_checkpoint_files_are_refused(seed, tmp_path):
    rng = np.random.default_rng(50000 + seed)
    dims = (8, 8, 6)
    f = fx.Fluid()
    assert f.Init(32, 32, dims, jacobi_iters=4)
    for k in range(2):
        f.UpdateFrame(f32(f.default_time_step()), k)
        f.Simulate(k)
    good = tmp_path / "good.fxck"
    f.SaveCheckpoint(str(good))
    want = {fid: f.download(fid) for fid in (fx.FIELD_VELOCITY, fx.FIELD_COLOR, fx.FIELD_PRESSURE)}
    data = bytearray(good.read_bytes())
    kind = int(rng.integers(0, 6))
    ok_expected = False
    if kind == 0:
        data = data[:int(rng.integers(0, len(data)))]                       # truncated
    elif kind == 1:
        off = int(rng.choice([0, 3, 8, 12, 16]))                            # magic or an extent
        data[off] ^= int(rng.integers(1, 256))
    elif kind == 2:
        data += bytes(int(rng.integers(1, 64)))                             # trailing bytes
    elif kind == 3:
        data[int(rng.integers(64, len(data) - 8 * dims[2]))] ^= 0x01        # payload: still a valid file of this grid
        ok_expected = True
    elif kind == 4:
        data[len(data) - 8 * (1 + int(rng.integers(0, dims[2])))] = 0       # a plane not marked complete (interrupted save): u64 mark -> 0
    else:
        data[len(data) - 8 * (1 + int(rng.integers(0, dims[2])))] = 9       # a plane left over from another save (its mark names other steps)
    bad = tmp_path / "bad.fxck"
    bad.write_bytes(bytes(data))
    g2 = fx.Fluid()
    assert g2.Init(32, 32, dims, jacobi_iters=4)
    if ok_expected:
        g2.LoadCheckpoint(str(bad))
    else:
        with pytest.raises(fx.FluidxError):
            g2.LoadCheckpoint(str(bad))
        # a refused file leaves the context usable, and the good one still loads
        g2.LoadCheckpoint(str(good))
        for fid, w in want.items():
            assert np.array_equal(g2.download(fid), w)
    with pytest.raises(fx.FluidxError):
        g2.LoadCheckpoint(str(tmp_path / "missing.fxck"))


@pytest.mark.parametrize("seed", range(SOAK or 40))
def test_random_slab_groups_are_validated(seed):
    """fx_comm_init_local with random member lists: a contiguous chain of like contexts is accepted and steps; anything else
    (gaps, overlaps, wrong order, a whole-grid member, members of another grid / storage / sweep count / halo, the same context
    twice, a member already in a group) is refused with a status -- never a crash, a hang or a corrupted neighbour"""
    import ctypes as C
    rng = np.random.default_rng(60000 + seed)
    lib = capi.load()
    S, Z = 32, 48
    base = dict(storage="fp32", jacobi_iters=6, halo_advect=6, halo_jacobi=4)
    cuts = [0, 16, 32, 48]
    members, descs, valid = [], [], True
    for r in range(3):
        kw, dims, slab = dict(base), (S, S, Z), (cuts[r], cuts[r + 1] - cuts[r])
        fault = int(rng.integers(0, 14)) if rng.random() < 0.5 else -1
        if fault == 0: dims = (S, S, Z + 16 * (r == 2)); valid &= r != 2
        elif fault == 1: dims = (64, 64, Z); valid = False
        elif fault == 2: kw["storage"] = "fp16"; valid = False
        elif fault == 3: kw["jacobi_iters"] = 7; valid = False
        elif fault == 4: kw["halo_jacobi"] = 5; valid = False
        elif fault == 5: kw["halo_advect"] = 8; valid = False
        elif fault == 6: slab = (slab[0] + 1, slab[1] - 1) if r else (slab[0], slab[1] - 1); valid = False      # gap
        elif fault == 7: slab = None; valid = False                                                         # whole grid
        elif fault == 8: kw["jacobi_mode"] = "faithful"; valid = False
        elif fault == 9: kw["advect_address"] = "mirror"; valid = False
        f = fx.Fluid()
        assert f.Init(64, 64, dims, slab=slab, **kw), f.last_status
        members.append(f)
        descs.append((dims, tuple(sorted(kw.items()))))
    if len(set(descs)) == 1 and descs[0][0] == (S, S, Z) and all(m.slab == (cuts[r], 16) for r, m in enumerate(members)):
        valid = True                                          # every member drew the same deviation: a consistent chain after all
    order = list(range(3))
    twist = rng.random()
    if twist < 0.15:
        order = [int(i) for i in rng.permutation(3)]
        valid &= order == [0, 1, 2]
    elif twist < 0.25:
        order = [0, 1, 1]; valid = False
    elif twist < 0.33:
        order = [0, 1]; valid = False                        # the chain stops short of the grid
    arr = (C.c_void_p * len(order))(*[members[i]._ctx for i in order])
    rc = lib.fx_comm_init_local(arr, len(order))
    assert rc == (capi.FX_OK if valid else capi.FX_E_INVALID), (rc, valid, order)
    if rc == capi.FX_OK:
        assert lib.fx_comm_init_local(arr, len(order)) == capi.FX_E_STATE          # already grouped
        dt = f32(members[0].default_time_step())
        for k in range(2):
            members[0].UpdateFrame(dt, k)
            members[0].Simulate(k)
        members[0].Synchronize()
        assert np.isfinite(members[1].download(fx.FIELD_PRESSURE)).all()
    else:
        # refused: every member is still a free context that can be destroyed (or grouped properly later)
        for m in members:
            assert m.frame_info() is not None
    for m in members:
        m.Release()


def test_every_entry_point_refuses_null_and_nonsense():
    """each ABI call with a NULL context, NULL buffers, unknown enum values or sizes that do not fit: a negative status (or 0
    bytes), never a crash"""
    import ctypes as C
    lib = capi.load()
    null = C.c_void_p()
    fbuf = (C.c_float * 64)()
    fi, tm = capi.FrameInfo(), capi.Timing()
    u = C.c_uint32()
    calls = [
        lambda c: lib.fx_destroy(c), lambda c: lib.fx_set_max_samples(c, 1, 1), lambda c: lib.fx_set_sh(c, fbuf),
        lambda c: lib.fx_update_frame(c, C.c_float(0.1), 0, fbuf, fbuf, fbuf), lambda c: lib.fx_simulate(c, None, 0),
        lambda c: lib.fx_render(c, None, 0, 3), lambda c: lib.fx_get_frame_info(c, C.byref(fi)), lambda c: lib.fx_synchronize(c),
        lambda c: lib.fx_upload(c, 0, fbuf, 256), lambda c: lib.fx_download(c, 0, fbuf, 256),
        lambda c: lib.fx_checkpoint_save(c, b"/tmp/x.fxck"), lambda c: lib.fx_checkpoint_load(c, b"/tmp/x.fxck"),
        lambda c: lib.fx_advect(c, None), lambda c: lib.fx_divergence(c, None), lambda c: lib.fx_jacobi(c, None, 1),
        lambda c: lib.fx_project(c, None), lambda c: lib.fx_sh_transform(c, fbuf, 1, fbuf), lambda c: lib.fx_set_environment(c, fbuf, 1),
        lambda c: lib.fx_render_environment(c, None, 0), lambda c: lib.fx_clear_render_target(c, None, fbuf),
        lambda c: lib.fx_render_cube(c, None, 0), lambda c: lib.fx_timing_enable(c, 1), lambda c: lib.fx_timing_read(c, C.byref(tm), 0),
        lambda c: lib.fx_set_option(c, 1, 1), lambda c: lib.fx_comm_gather_color(c, None, None, 0, None, None),
        lambda c: lib.fx_dds_decode_cube(c, fbuf, 256, 0, fbuf, 64),
    ]
    for i, call in enumerate(calls):
        assert call(null) < 0, i
    assert lib.fx_field_bytes(null, 0) == 0
    assert lib.fx_dds_cube_info(None, 0, C.byref(u), C.byref(u)) < 0
    assert lib.fx_comm_init_local(None, 2) < 0 and lib.fx_comm_get_unique_id(None, 0) < 0
    assert lib.fx_create(None, None) < 0 and lib.fx_create(C.byref(null), None) < 0
    # a live context with nonsense arguments
    f = fx.Fluid()
    assert f.Init(32, 32, (16, 16, 16))
    c = f._ctx
    assert lib.fx_update_frame(c, C.c_float(0.1), 3, fbuf, fbuf, fbuf) < 0 and lib.fx_simulate(c, None, 7) < 0 and lib.fx_render(c, None, 9, 3) < 0
    assert lib.fx_upload(c, 0, None, 4) < 0 and lib.fx_upload(c, 0, fbuf, 4) < 0 and lib.fx_upload(c, 77, fbuf, 256) < 0
    assert lib.fx_download(c, 2, fbuf, 1) < 0 and lib.fx_download(c, -1, fbuf, 256) < 0 and lib.fx_download(c, 8, fbuf, 256) < 0   # no target yet
    assert lib.fx_set_option(c, 99, 1) < 0 and lib.fx_set_option(c, 1, 4) < 0 and lib.fx_set_option(c, 2, 0) < 0
    assert lib.fx_sh_transform(c, None, 4, fbuf) < 0 and lib.fx_sh_transform(c, fbuf, 0, fbuf) < 0 and lib.fx_sh_transform(c, fbuf, 1 << 20, fbuf) < 0
    assert lib.fx_set_environment(c, fbuf, 0) < 0 and lib.fx_set_environment(c, fbuf, 1 << 20) < 0
    assert lib.fx_jacobi(c, None, 0) < 0 and lib.fx_get_frame_info(c, None) < 0 and lib.fx_timing_read(c, None, 0) < 0
    assert lib.fx_checkpoint_save(c, None) < 0 and lib.fx_checkpoint_save(c, b"") < 0 and lib.fx_checkpoint_load(c, b"/nonexistent/dir/x") < 0
    assert lib.fx_checkpoint_save(c, b"/nonexistent/dir/x") < 0
    assert lib.fx_comm_gather_color(c, None, c, 0, None, None) < 0                       # not in a group
    assert lib.fx_clear_render_target(c, None, None) <= 0
    # and it still works
    f.UpdateFrame(f32(f.default_time_step()), 0)
    f.Simulate(0)
    f.Synchronize()
    assert f.download(fx.FIELD_COLOR).any()


def test_contexts_on_concurrent_host_threads_do_not_interfere():
    """separate contexts driven from separate host threads (ctypes drops the GIL inside every call): each thread's fields equal
    the same run done alone -- no shared mutable state behind the ABI besides the per-context one"""
    import threading
    configs = [((32, 32, 32), "fp32", 10, "fixed"), ((48, 48, 20), "fp16", 7, "faithful"), ((64, 64, 1), "fp32", 12, "fixed"),
               ((40, 40, 24), "fp32", 5, "fixed"), ((32, 32, 32), "fp16", 9, "fixed"), ((256, 256, 64), "fp32", 6, "fixed")]

    def run(cfg, out, idx, noisy):
        dims, storage, iters, mode = cfg
        f = fx.Fluid()
        assert f.Init(96, 64, dims, storage=storage, jacobi_iters=iters, jacobi_mode=mode)
        view, proj, eye = fx.default_camera(96, 64)
        for k in range(6):
            f.UpdateFrame(f32(f.default_time_step()), k % 3, view, proj, eye)
            f.Simulate(k % 3)
            if noisy and dims[2] > 1 and k % 2:
                f.Render(k % 3, fx.Fluid.OPTIMIZED, to_target=True)
                f.download(fx.FIELD_PRESSURE)
        f.Synchronize()
        out[idx] = (f.download(fx.FIELD_VELOCITY), f.download(fx.FIELD_COLOR), f.download(fx.FIELD_PRESSURE))
        f.Release()

    alone = [None] * len(configs)
    for i, cfg in enumerate(configs):
        run(cfg, alone, i, False)
    for _ in range(3):
        together = [None] * len(configs)
        threads = [threading.Thread(target=run, args=(cfg, together, i, True)) for i, cfg in enumerate(configs)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for i in range(len(configs)):
            assert together[i] is not None, i
            for a, b in zip(alone[i], together[i]):
                assert np.array_equal(a, b), configs[i]


@pytest.mark.parametrize("seed", range(SOAK or 16))
def test_random_dds_mip_chains_decode_like_the_oracle(seed):
    """BC6H cube maps of random extent (also not a multiple of 4) with random mip counts and random block data: every mip of
    every face decodes bit for bit like the oracle (mip offsets, partial edge blocks, all modes)"""
    import os
    import struct
    rng = np.random.default_rng(70000 + seed)
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "bc6h_fixture.npz"))
    n = int(rng.integers(1, 71))
    max_mips = int(np.floor(np.log2(n))) + 1
    mips = int(rng.integers(1, max_mips + 1))
    hdr = bytearray(gold["dds_mip3"].tobytes()[:148])
    struct.pack_into("<I", hdr, 12, n)
    struct.pack_into("<I", hdr, 16, n)
    struct.pack_into("<I", hdr, 20, ((n + 3) // 4) ** 2 * 16)
    struct.pack_into("<I", hdr, 28, mips)
    per_face = sum((((max(n >> m, 1)) + 3) // 4) ** 2 * 16 for m in range(mips))
    body = rng.integers(0, 256, 6 * per_face, dtype=np.uint8).tobytes()
    dds = bytes(hdr) + body
    f = fx.Fluid()
    assert f.Init(64, 64, (16, 16, 16))
    probe = fx.LightProbe(f)
    for mip in range(mips):
        want, _ = orc.dds_bc6h_cube(dds, mip)
        got = probe.decode_dds(dds, mip)
        assert got is not None and got.shape == want.shape == (6, max(n >> mip, 1), max(n >> mip, 1), 3), (n, mips, mip)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, mips, mip)
    assert probe.decode_dds(dds, mips) is None


@pytest.mark.parametrize("seed", range(SOAK or 24))
def test_random_frame_sequences_render_alike_on_both_paths(seed, knob):
    """simulate-and-render sequences as a caller would run them -- random grid (powers of two and not), storage, light probe, camera, which
    advection kernel family serves the grid, which frames are rendered and how, an upload in between: the accelerated marches (side volume
    written by the advection of a rendered frame, the filling build pass, the three-pass light volume) give every frame the picture the
    plain kernels give it, bit for bit, and leave the simulation alone"""
    c = draw_camera(seed)
    rng = np.random.default_rng(77000 + seed)
    X = int(rng.choice([32, 40, 64, 64, 48]))
    Z = int(rng.choice([32, 64, 24, 40]))
    knob("ADVECT_LDS", str(rng.choice(["0", "2"])))
    if rng.random() < 0.3:
        knob("LIGHT_FILL", "0")
    vw, vh = c["vp"]
    view = fx.look_at_lh(c["eye"], c["focus"], c["up"])
    proj = fx.perspective_fov_lh(f32(c["fov"]), vw / float(vh), 1.0, 1000.0)
    sh = (rng.random((9, 3)) * np.array([[2.0]] + [[0.5]] * 8)).astype(f32) if c["use_sh"] else None
    n = int(rng.integers(10, 18))
    plan = [int(rng.choice([-1, fx.Fluid.OPTIMIZED, fx.Fluid.OPTIMIZED, fx.Fluid.RAY_MARCH_CUBEMAP, fx.Fluid.SEPARATE_LIGHT_PASS, fx.Fluid.RAY_MARCH_DIRECT])) for _ in range(n)]
    plan[-1] = fx.Fluid.OPTIMIZED
    upload_at = int(rng.integers(4, n)) if rng.random() < 0.4 else -1

    def run(accel):
        f = fx.Fluid()
        assert f.Init(vw, vh, (X, X, Z), storage=c["storage"])
        f.SetMaxSamples(*c["samples"])
        f.set_option(capi.OPT_RENDER_ACCEL, accel)
        if sh is not None:
            f.SetSH(sh)
        out = []
        for k in range(n):
            f.UpdateFrame(f32(f.default_time_step() * 2.0), k % 3, view, proj, c["eye"])
            f.Simulate(k % 3)
            if k == upload_at:
                f.upload(fx.FIELD_COLOR, np.ascontiguousarray(f.download(fx.FIELD_COLOR)[::-1]))
            if plan[k] >= 0:
                f.ClearRenderTarget()
                f.Render(k % 3, plan[k])
                f.Synchronize()
                out.append(f.download(fx.FIELD_CUBEMAP) if plan[k] & fx.Fluid.RAY_MARCH_CUBEMAP else f.download(fx.FIELD_TARGET_FLOAT))
                if plan[k] & fx.Fluid.SEPARATE_LIGHT_PASS:
                    out.append(f.download(fx.FIELD_LIGHTMAP))
        out += [f.download(fx.FIELD_VELOCITY), f.download(fx.FIELD_COLOR), f.download(fx.FIELD_PRESSURE)]
        return out

    a, b = run(1), run(0)
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (seed, k, X, Z, c["storage"], plan)
