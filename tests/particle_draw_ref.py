"""numpy model of the particle draw (include/fluidx_hip.h fx_set_particle_draw / fx_draw_particles / fx_particle_splats,
fluidx12_amd/csrc/fx_particle_draw.hip: k_draw_splat, k_draw_resolve).

The rule, fp32, every operation rounded as written; (W, H) = the viewport, M = the forward WorldViewProj rows, c = particle_ref.c01.  A record
(p, age) is drawn iff age >= 0 (-0.0 is live, a NaN is dead):
  1 project    q_a = fma(c(p_a), 2, -1);  h_r = fma(1, M[4r+3], fma(q_z, M[4r+2], fma(q_y, M[4r+1], q_x * M[4r+0])));  culled unless h_3 > 0;
               cx, cy, cz = h_0 / h_3, h_1 / h_3, h_2 / h_3;  culled unless 0 <= cz < 1;  u = fma(cx, .5, .5), v = -fma(cy, .5, .5) + 1;
               X = u * W, Y = v * H;  culled unless 0 <= X < W and 0 <= Y < H (a NaN culls);  host pixel (px, py) = ((int)X, (int)Y)
  2 depth      with a scene depth: culled unless cz <= depth[py][px]
  3 occlusion  T = c(-alpha + 1), alpha = what the merged direct view march returns for the host pixel with a depth buffer holding cz there.
               NOT restated here: it comes from test_depth_ref.ref_direct, the depth-aware CPU reference (it includes nothing of the product and
               is anchored to the oracle), one call per layer -- the rank of a particle among those of its pixel -- with the depth buffer 1.0
               everywhere except cz at the layer's pixels.  At most MAX_LAYERS layers
  4 amounts    qb = (uint)(T * 32768 + 0.5);  s = lifetime > 0 ? c(age / lifetime) : 0;  qs = (uint)(s * 256 + 0.5);
               young = qb (256 - qs), old = qb qs
  5 footprint  per axis t = X - 0.5, fl = floor(t), w1 = (int)rint((t - fl) * 128), w0 = 128 - w1 on the pixels (int)fl and (int)fl + 1; a pixel off
               the viewport is dropped;  acc[iy][ix] += (young, old) * wx * wy in uint64: qb << 22 in total for a footprint on screen
  6 resolve    Yv = (float)acc0 * 2^-37, Ov = (float)acc1 * 2^-37;  k0_c = color_c * color_w, k1_c = end_color_c * end_color_w;
               src_c = fma(Ov, k1_c, Yv * k0_c);  where acc0 | acc1 != 0: target = blend_premultiplied(target, src, 0), target_float = (src, 0);
               elsewhere the target keeps its bytes and target_float = 0
`project` / `splats` / `resolve` are vectorised, `splats_loops` / `resolve_loops` their plain-loop twins on Python integers
(tests/test_particle_draw_ref.py holds one against the other).

Layouts: records float32[n][4]; the accumulator uint64[H][W][2]; target uint8[H][W][4] (r, g, b, a), target_float float32[H][W][4]."""
import numpy as np

import particle_ref as pr
from fma_ref import fma
from particle_trail_ref import to_f32_rne

f32 = np.float32
ONE = 1 << 37                                                    # what an unoccluded record whose footprint is on screen adds in total
MAX_LAYERS = 8
COUNTS = list(pr.COUNTS)                                         # 1, 257, 4099: a wave edge and a workgroup edge
DRAWN, DEAD, BEHIND, Z_OUT, X_OUT, Y_OUT, HIDDEN = range(7)      # what became of a record: drawn, or the first test it failed


# ---- the camera -----------------------------------------------------------------------------------------------------------------------------
def mat_mul(a, b):
    """the host's 4 x 4 product (fx_hostmath.h Mat4::operator*): a product, then three fma, per element"""
    a, b = np.asarray(a, f32).reshape(4, 4), np.asarray(b, f32).reshape(4, 4)
    acc = (a[:, 0:1] * b[0:1, :]).astype(f32)
    for k in range(1, 4):
        acc = fma(a[:, k:k + 1], b[k:k + 1, :], acc)
    return acc


def forward_wvp(view, proj):
    """M: CBPerObject.WorldViewProj = world * (view * proj), world = scale 10, as its four constant-buffer rows (fx_update_frame), float32[16]"""
    world = np.diag(np.array([10, 10, 10, 1], f32))
    return np.ascontiguousarray(mat_mul(world, mat_mul(view, proj)).T).reshape(16)


def inside_camera(W, H):
    """a camera whose eye lies inside the volume (the world-space cube [-10, 10]^3): records behind the eye, in front of the near plane and
    off the screen on both axes all exist"""
    import fluidx12_amd as fx
    eye = np.array([3.0, 2.0, -4.0], f32)
    view = fx.look_at_lh(eye, [-1.0, 0.5, 3.0], [0, 1, 0])
    proj = fx.perspective_fov_lh(f32(np.pi) / f32(4.0), W / float(H), 1.0, 1000.0)
    return view.reshape(16), proj.reshape(16), eye


# ---- steps 1 and 2 ----------------------------------------------------------------------------------------------------------------------------
def project(rec, M, W, H, depth=None):
    """-> dict: cls (DRAWN ... per record), cz, X, Y (float32), px, py (int64; 0 where the record has no host pixel)"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    M = np.asarray(M, f32).reshape(16)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        live = rec[:, 3] >= 0
        q = [fma(pr.c01(rec[:, a]), f32(2), f32(-1)) for a in range(3)]
        h = [fma(f32(1), M[4 * r + 3], fma(q[2], M[4 * r + 2], fma(q[1], M[4 * r + 1], (q[0] * M[4 * r + 0]).astype(f32)))) for r in range(4)]
        front = h[3] > 0
        cx, cy, cz = [(h[a] / h[3]).astype(f32) for a in range(3)]
        z_in = (f32(0) <= cz) & (cz < f32(1))
        u = fma(cx, f32(0.5), f32(0.5))
        v = (-fma(cy, f32(0.5), f32(0.5)) + f32(1)).astype(f32)
        X, Y = (u * f32(W)).astype(f32), (v * f32(H)).astype(f32)
        x_in = (f32(0) <= X) & (X < f32(W))
        y_in = (f32(0) <= Y) & (Y < f32(H))
    cls = np.select([~live, ~front, ~z_in, ~x_in, ~y_in], [DEAD, BEHIND, Z_OUT, X_OUT, Y_OUT], DRAWN)
    on = cls == DRAWN
    px = np.where(on, X, 0).astype(np.int64)
    py = np.where(on, Y, 0).astype(np.int64)
    if depth is not None:
        depth = np.ascontiguousarray(depth, f32).reshape(H, W)
        with np.errstate(invalid="ignore"):
            cls = np.where(on & ~(cz <= depth[py, px]), HIDDEN, cls)
    return {"cls": cls, "cz": cz, "X": X, "Y": Y, "px": px, "py": py}


# ---- step 3: from the depth-aware reference -----------------------------------------------------------------------------------------------------
def layers_of(P, W):
    """the rank of every drawn record among the drawn records of its host pixel, in index order (-1: not drawn)"""
    idx = np.nonzero(P["cls"] == DRAWN)[0]
    pix = P["py"][idx] * W + P["px"][idx]
    order = np.argsort(pix, kind="stable")
    sp = pix[order]
    first = np.r_[True, sp[1:] != sp[:-1]] if len(sp) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(sp)), 0)) if len(sp) else np.zeros(0, np.int64)
    rank = np.full(len(P["cls"]), -1, np.int64)
    rank[idx[order]] = np.arange(len(sp)) - start
    return rank


def transmittance(P, col, fr, wvp_i, W, H, ns, nl):
    """T per record (1 where it is not drawn): one ref_direct call per layer, merged, without the light probe, ns samples"""
    from test_depth_ref import ref_direct
    rank = layers_of(P, W)
    layers = int(rank.max()) + 1 if len(rank) else 0
    assert layers <= MAX_LAYERS, "%d particles in one pixel: the model serves at most %d" % (layers, MAX_LAYERS)
    T = np.ones(len(rank), f32)
    for l in range(layers):
        sel = np.nonzero(rank == l)[0]
        depth = np.ones((H, W), f32)
        depth[P["py"][sel], P["px"][sel]] = P["cz"][sel]
        out, _ = ref_direct(col, None, fr, wvp_i, W, H, ns, nl, False, False, depth)
        T[sel] = pr.c01((-out[P["py"][sel], P["px"][sel], 3] + f32(1)).astype(f32))
    return T


# ---- steps 4 and 5 ----------------------------------------------------------------------------------------------------------------------------
def amounts(T, age, lifetime):
    """-> (young, old) per record, int64"""
    T, age, lifetime = np.asarray(T, f32), np.asarray(age, f32), f32(lifetime)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        qb = ((T * f32(32768)).astype(f32) + f32(0.5)).astype(f32).astype(np.int64)
        s = pr.c01((age / lifetime).astype(f32)) if lifetime > 0 else np.zeros(len(T), f32)
        qs = ((s * f32(256)).astype(f32) + f32(0.5)).astype(f32).astype(np.int64)
    return qb * (256 - qs), qb * qs


def foot_axis(x):
    """-> (first pixel, weight 0, weight 1) of every coordinate, int64"""
    t = (np.asarray(x, f32) - f32(0.5)).astype(f32)
    fl = np.floor(t)
    w1 = np.rint(((t - fl).astype(f32) * f32(128)).astype(f32)).astype(np.int64)
    return fl.astype(np.int64), 128 - w1, w1


def splats(rec, P, T, lifetime, W, H):
    """the accumulator behind the splat: uint64 [H][W][2]"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    on = P["cls"] == DRAWN
    young, old = amounts(np.asarray(T, f32)[on], rec[on, 3], lifetime)
    ix, wx0, wx1 = foot_axis(P["X"][on])
    iy, wy0, wy1 = foot_axis(P["Y"][on])
    acc = np.zeros((H * W, 2), np.uint64)
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            x, y = ix + dx, iy + dy
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            w = (wx * wy)[ok]
            np.add.at(acc[:, 0], (y * W + x)[ok], (young[ok] * w).astype(np.uint64))
            np.add.at(acc[:, 1], (y * W + x)[ok], (old[ok] * w).astype(np.uint64))
    return acc.reshape(H, W, 2)


# ---- step 6 -----------------------------------------------------------------------------------------------------------------------------------
def to_unorm8(v):
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        q = ((v * f32(255)).astype(f32) + f32(0.5)).astype(f32)
        return np.where(~(v > 0), 0, np.where(v >= 1, 255, np.where(np.isfinite(q), q, 0).astype(np.int64))).astype(np.uint8)


def source(acc, draw):
    """src = the light every pixel receives: float32 [H][W][3]"""
    acc = np.asarray(acc, np.uint64)
    Yv = (acc[..., 0].astype(f32) * f32(2.0 ** -37)).astype(f32)
    Ov = (acc[..., 1].astype(f32) * f32(2.0 ** -37)).astype(f32)
    c0, c1 = np.asarray(draw["color"], f32), np.asarray(draw["end_color"], f32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([fma(Ov, f32(c1[c] * c1[3]), (Yv * f32(c0[c] * c0[3])).astype(f32)) for c in range(3)], axis=-1)


def resolve(acc, draw, target):
    """-> (target_float float32[H][W][4], target uint8[H][W][4]) behind the resolve over the RGBA8 `target`"""
    acc = np.asarray(acc, np.uint64)
    target = np.ascontiguousarray(target, np.uint8)
    hit = (acc[..., 0] | acc[..., 1]) != 0
    src = source(acc, draw)
    tf = np.zeros(acc.shape[:2] + (4,), f32)
    tf[..., :3] = np.where(hit[..., None], src, f32(0))
    out = target.copy()
    ia = f32(1) - f32(0)
    for c in range(4):
        s = src[..., c] if c < 3 else np.zeros(acc.shape[:2], f32)
        out[..., c] = np.where(hit, to_unorm8(fma((target[..., c].astype(f32) / f32(255)).astype(f32), ia, s)), target[..., c])
    return tf, out


# ---- the same in plain loops, on Python integers and numpy scalars ---------------------------------------------------------------------------------
def splats_loops(rec, M, W, H, T, lifetime, depth=None):
    """steps 1, 2, 4 and 5 record by record; T: the transmittance per record (step 3)"""
    M = [f32(v) for v in np.asarray(M, f32).reshape(16)]
    acc = [[0, 0] for _ in range(W * H)]
    lifetime = f32(lifetime)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k, (x, y, z, age) in enumerate(np.ascontiguousarray(rec, f32).reshape(-1, 4)):
            if not age >= 0:
                continue
            q = [fma(pr._c(v), f32(2), f32(-1)) for v in (x, y, z)]
            h = [fma(f32(1), M[4 * r + 3], fma(q[2], M[4 * r + 2], fma(q[1], M[4 * r + 1], f32(q[0] * M[4 * r + 0])))) for r in range(4)]
            if not h[3] > 0:
                continue
            cx, cy, cz = f32(h[0] / h[3]), f32(h[1] / h[3]), f32(h[2] / h[3])
            if not (0 <= cz and cz < 1):
                continue
            u, v = fma(cx, f32(0.5), f32(0.5)), f32(-fma(cy, f32(0.5), f32(0.5)) + f32(1))
            X, Y = f32(u * f32(W)), f32(v * f32(H))
            if not (0 <= X and X < W and 0 <= Y and Y < H):
                continue
            px, py = int(X), int(Y)
            if depth is not None and not cz <= depth[py][px]:
                continue
            qb = int(f32(f32(f32(T[k]) * f32(32768)) + f32(0.5)))
            s = pr._c(f32(age / lifetime)) if lifetime > 0 else f32(0)
            qs = int(f32(f32(s * f32(256)) + f32(0.5)))
            young, old = qb * (256 - qs), qb * qs
            taps = []
            for c in (X, Y):
                t = f32(c - f32(0.5))
                fl = np.floor(t)
                w1 = int(np.rint(f32(f32(t - fl) * f32(128))))
                taps.append(((int(fl), 128 - w1), (int(fl) + 1, w1)))
            for iy, wy in taps[1]:
                for ix, wx in taps[0]:
                    if 0 <= ix < W and 0 <= iy < H:
                        acc[iy * W + ix][0] += young * wx * wy
                        acc[iy * W + ix][1] += old * wx * wy
    return np.array(acc, np.uint64).reshape(H, W, 2)


def resolve_loops(acc, draw, target):
    acc = np.asarray(acc, np.uint64)
    H, W = acc.shape[:2]
    tf = np.zeros((H, W, 4), f32)
    out = np.ascontiguousarray(target, np.uint8).copy()
    c0, c1 = [f32(v) for v in draw["color"]], [f32(v) for v in draw["end_color"]]
    for y in range(H):
        for x in range(W):
            a0, a1 = int(acc[y, x, 0]), int(acc[y, x, 1])
            if not (a0 | a1):
                continue
            Yv, Ov = f32(to_f32_rne(a0) * f32(2.0 ** -37)), f32(to_f32_rne(a1) * f32(2.0 ** -37))
            for c in range(3):
                s = fma(Ov, f32(c1[c] * c1[3]), f32(Yv * f32(c0[c] * c0[3])))
                tf[y, x, c] = s
                v = fma(f32(f32(out[y, x, c]) / f32(255)), f32(1), s)
                out[y, x, c] = 0 if not v > 0 else 255 if v >= 1 else int(f32(f32(v * f32(255)) + f32(0.5)))
            v = fma(f32(f32(out[y, x, 3]) / f32(255)), f32(1), f32(0))
            out[y, x, 3] = 0 if not v > 0 else 255 if v >= 1 else int(f32(f32(v * f32(255)) + f32(0.5)))
    return tf, out


# ---- the sets the tests draw ---------------------------------------------------------------------------------------------------------------------
def records(n, lifetime, seed=3, dead_every=5):
    """n records at numpy.random.default_rng(seed).random((n, 3)), ages spread over [0, 1.5 lifetime], one in `dead_every` dead -- by a negative
    age and by a NaN one in turn (0: none)"""
    rng = np.random.default_rng(seed)
    rec = np.empty((n, 4), f32)
    rec[:, :3] = rng.random((n, 3)).astype(f32)
    rec[:, 3] = (np.random.default_rng(seed + 100).random(n) * 1.5 * lifetime).astype(f32)
    if dead_every:
        dead = np.arange(n) % dead_every == dead_every - 1
        rec[dead, 3] = np.where(np.arange(dead.sum()) % 2 == 0, f32(-1), f32(np.nan))
    return rec
