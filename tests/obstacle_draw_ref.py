"""numpy model of the obstacle draw (include/fluidx_hip.h fx_set_obstacle_draw / fx_draw_obstacles / fx_obstacle_hits,
fluidx12_amd/csrc/fx_obstacle_draw.hip: k_obstacle_cast).

The rule, fp32, every operation rounded as written; N = (X, Y, Z), S(i) = the cell i = (x, y, z) is solid, (W, H) = the viewport, M = the
forward WorldViewProj rows:
  1 ray      (o, d) = what the direct march casts for the pixel (fx_march.h pixel_ray with compute_ray_origin); a discard is a miss;
             e = the entry axis of compute_ray_origin, the axis whose quotient became U, -1 when the eye lies inside the box
  2 start    s_a = fma(o_a, .5, .5);  i_a = min(max((int)floor(s_a * N_a), 0), N_a - 1);  st_a = +1 / -1 / 0 for d_a > 0 / < 0 / otherwise;
             r_a = 1 / d_a;  S(i): a hit at t = 0, p = o, face = 2e + (d_e > 0) with an entry axis, 6 without
  3 walk     t_a = st_a ? (fma((float)(i_a + (st_a > 0)) / (float)N_a, 2, -1) - o_a) * r_a : FLT_MAX;
             a* = (t_0 <= t_1 && t_0 <= t_2) ? 0 : (t_1 <= t_2) ? 1 : 2;  st_a* == 0: miss;  i_a* += st_a*;  off the grid: miss;
             S(i): hit with t_hit = t_a*, face = 2 a* + (st_a* > 0), p_a = fma(d_a, t_hit, o_a);  X + Y + Z advances at most
  4 visible  h_r = fma(1, M[4r+3], fma(p_2, M[4r+2], fma(p_1, M[4r+1], p_0 * M[4r+0])));  cz = h_2 / h_3;
             drawn iff h_3 > 0 && 0 <= cz && cz < 1 && (no scene depth || cz <= scene[py][px])
  5 shade    L = the local light direction, or the direction from p to the local light point (0 where the marches cast no ray);
             st = +1 for an odd face, -1 for an even one, a = face / 2;  ndl = face < 6 ? fmax(0, (float)(-st) * L_a) : 0;
             src_c = ((albedo_c * albedo_w) * fma(ndl, color_w * color_c, ambient_w * ambient_c)) * 0.159154937
  6 store    drawn: target = (unorm8(src), 255), target_float = (src, 1), depth = cz;  else the target keeps its bytes, target_float = 0,
             depth = the scene depth or 1;  hits word = a hit ? 1 << 63 | drawn << 62 | face << 32 | (z Y + y) X + x : 0
`cast` / `shade` / `draw` are vectorised over the pixels; `draw_loops` is their plain-loop twin on Python floats holding float32 values
(tests/test_obstacle_draw_ref.py holds one against the other).

Layouts: the mask bool[Z][Y][X]; hits uint64[H][W]; depth float32[H][W]; target uint8[H][W][4]; target_float float32[H][W][4]."""
import math
import struct

import numpy as np

import particle_draw_ref as pd
from fma_ref import fma

f32 = np.float32
FLT_MAX = f32(3.40282347e+38)
INV_2PI = f32(0.159154937)
HIT, DRAWN = 1 << 63, 1 << 62


# ---- the scene of the tests ---------------------------------------------------------------------------------------------------------------------
def scene_mask(X, Z, ball=True, slab=True, beam=True):
    """on an X x X x Z grid: a ball (cell centres within 0.2 of (.5, .45, .5) in texture space), a slab on the floor that touches the y and
    z walls (all z, y < 3, x in [2X/3, 2X/3 + 6)) and a beam through both x walls (z in [Z/3, Z/3 + 3), y in [X/3, X/3 + 4), all x)"""
    S = np.zeros((Z, X, X), bool)
    if ball:
        z, y, x = np.meshgrid((np.arange(Z) + 0.5) / Z, (np.arange(X) + 0.5) / X, (np.arange(X) + 0.5) / X, indexing="ij")
        S |= (x - 0.5) ** 2 + (y - 0.45) ** 2 + (z - 0.5) ** 2 <= 0.2 ** 2
    if slab:
        S[:, :3, 2 * X // 3:2 * X // 3 + 6] = True
    if beam:
        S[Z // 3:Z // 3 + 3, X // 3:X // 3 + 4, :] = True
    return S


def cameras(name, W, H):
    """(view[16], proj[16], eye[3]) of the tests' cameras: "default" (eye (4, 16, -40)), "opposite" (eye (-4, -16, 40)), "axis" (eye (0, 0, -30):
    the centre row and column of an odd viewport have d_y = 0 and d_x = 0), "inside" (particle_draw_ref.inside_camera)"""
    import fluidx12_amd as fx
    if name == "inside":
        view, proj, eye = pd.inside_camera(W, H)
    else:
        eye = np.array({"default": (4.0, 16.0, -40.0), "opposite": (-4.0, -16.0, 40.0), "axis": (0.0, 0.0, -30.0)}[name], f32)
        view = fx.look_at_lh(eye, [0, 0, 0], [0, 1, 0])
        proj = fx.perspective_fov_lh(f32(np.pi) / f32(4.0), W / float(H), 1.0, 1000.0)
    return np.ascontiguousarray(view, f32).reshape(16), np.ascontiguousarray(proj, f32).reshape(16), np.asarray(eye, f32)


def frame(view, proj, eye, W, H, X, wvp_i=None, light=None):
    """the constants the cast reads: world_i (3 x 4 rows), eye, wvp_i (default: the oracle's inverse; the GPU tests pass the context's own
    fx_frame_info.world_view_proj_i), M, and the light -- the reference's constants, or `light` = {"kind", "position", "color", "ambient"}"""
    from oracle import orc
    fr = orc.update_frame(view, proj, eye, W, H, X)[0]
    out = {"world_i": np.array(list(fr.world_i), f32), "eye": np.array(list(fr.eye_pt), f32),
           "wvp_i": np.asarray(orc.world_view_proj_inverse(view, proj) if wvp_i is None else wvp_i, f32).reshape(16),
           "M": pd.forward_wvp(view, proj), "point": False,
           "light_pt": np.array(list(fr.light_pt), f32), "light_color": np.array(list(fr.light_color), f32), "ambient": np.array(list(fr.ambient), f32)}
    if light is not None:
        out["point"] = light.get("kind", "directional") == "point"
        out["light_pt"] = np.asarray(light["position"], f32)
        for k, key in (("color", "light_color"), ("ambient", "ambient")):
            if light.get(k) is not None:
                out[key] = np.asarray(light[k], f32)
    return out


# ---- step 1 -------------------------------------------------------------------------------------------------------------------------------------
def dot3(ax, ay, az, bx, by, bz):
    return fma(az, bz, fma(ay, by, (ax * bx).astype(f32)))


def local_point(fr, p):
    """mul(float4(p, 1), worldI): the chain of the eye point (pixel_ray, light_point_local)"""
    r = fr["world_i"].reshape(3, 4)
    return [fma(r[a, 3], f32(1), fma(p[2], r[a, 2], fma(p[1], r[a, 1], f32(p[0] * r[a, 0])))) for a in range(3)]


def rays(fr, W, H):
    """pixel_ray for every pixel, row-major: o, d float32[n][3], ok bool[n] (False: discard), e int64[n] (-1: none)"""
    py, px = np.divmod(np.arange(W * H), W)
    with np.errstate(all="ignore"):
        u = ((px.astype(f32) + f32(0.5)) / f32(W)).astype(f32)
        v = ((py.astype(f32) + f32(0.5)) / f32(H)).astype(f32)
        qx, qy, one = fma(u, f32(2), f32(-1)), fma(v, f32(-2), f32(1)), f32(1)
        M = fr["wvp_i"]
        h = [dot3(qx, qy, one, M[4 * r], M[4 * r + 1], M[4 * r + 3]) for r in range(4)]
        o = [(h[a] / h[3]).astype(f32) for a in range(3)]
        eye = local_point(fr, fr["eye"])
        d = [(o[a] + -eye[a]).astype(f32) for a in range(3)]
        rl = (f32(1) / np.sqrt(dot3(d[0], d[1], d[2], d[0], d[1], d[2]))).astype(f32)
        d = [(d[a] * rl).astype(f32) for a in range(3)]
        # compute_ray_origin
        inside = (np.abs(o[0]) <= 1) & (np.abs(o[1]) <= 1) & (np.abs(o[2]) <= 1)
        U = np.full(W * H, FLT_MAX, f32)
        hit = np.zeros(W * H, bool)
        e = np.full(W * H, -1, np.int64)
        for i in range(3):
            sgn = ((0 < d[i]).astype(f32) - (d[i] < 0).astype(f32)).astype(f32)
            q = ((-o[i] + -sgn).astype(f32) / d[i]).astype(f32)
            j, k = (i + 1) % 3, (i + 2) % 3
            ok = (q >= 0) & (1 >= np.abs(fma(d[j], q, o[j]))) & (1 >= np.abs(fma(d[k], q, o[k])))
            upd = ok & (q < U)
            U, hit, e = np.where(upd, q, U), hit | upd, np.where(upd, i, e)
        moved = [np.fmin(np.fmax(fma(d[a], U, o[a]), f32(-1)), f32(1)) for a in range(3)]
        o = [np.where(inside, o[a], moved[a]).astype(f32) for a in range(3)]
    return {"o": np.stack(o, 1), "d": np.stack(d, 1), "ok": inside | hit, "e": np.where(inside, -1, e)}


# ---- steps 2 to 4 -------------------------------------------------------------------------------------------------------------------------------
def plane_t(i, st, n, o, r):
    with np.errstate(all="ignore"):
        P = fma(((i + (st > 0)).astype(f32) / f32(n)).astype(f32), f32(2), f32(-1))
        return np.where(st != 0, ((P - o).astype(f32) * r).astype(f32), FLT_MAX).astype(f32)


def cast(S, fr, W, H, scene=None, R=None):
    """-> dict per pixel (row-major): hit, start, drawn (bool), face, cell, advances (int64), t, cz (float32), p (float32[n][3])"""
    S = np.ascontiguousarray(S, bool)
    Z, Y, X = S.shape
    N = np.array([X, Y, Z], np.int64)
    R = rays(fr, W, H) if R is None else R
    o, d, n = R["o"], R["d"], W * H
    flat = S.reshape(-1)
    with np.errstate(all="ignore"):
        s = fma(o, f32(0.5), f32(0.5))
        i = np.clip(np.nan_to_num(np.floor((s * N.astype(f32)).astype(f32)), nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), 0, N - 1)
        st = (d > 0).astype(np.int64) - (d < 0).astype(np.int64)
        r = (f32(1) / d).astype(f32)
    cell = (i[:, 2] * Y + i[:, 1]) * X + i[:, 0]
    start = R["ok"] & flat[cell]
    hit = start.copy()
    e = R["e"]
    de = np.take_along_axis(d, np.maximum(e, 0)[:, None], 1)[:, 0]
    face = np.where(start & (e >= 0), 2 * e + (de > 0), 6).astype(np.int64)
    th = np.zeros(n, f32)
    adv = np.zeros(n, np.int64)
    t = np.stack([plane_t(i[:, a], st[:, a], N[a], o[:, a], r[:, a]) for a in range(3)], 1)
    active = R["ok"] & ~start
    for _ in range(int(X + Y + Z)):
        idx = np.nonzero(active)[0]
        if not len(idx):
            break
        with np.errstate(invalid="ignore"):
            a0 = (t[idx, 0] <= t[idx, 1]) & (t[idx, 0] <= t[idx, 2])
            a1 = ~a0 & (t[idx, 1] <= t[idx, 2])
        ax = np.where(a0, 0, np.where(a1, 1, 2))
        sta = st[idx, ax]
        ia = i[idx, ax] + sta
        go = (sta != 0) & (ia >= 0) & (ia < N[ax])
        active[idx[~go]] = False
        idx, ax, sta, ia = idx[go], ax[go], sta[go], ia[go]
        tn = t[idx, ax]
        i[idx, ax] = ia
        t[idx, ax] = plane_t(ia, sta, N[ax], o[idx, ax], r[idx, ax])
        adv[idx] += 1
        c = (i[idx, 2] * Y + i[idx, 1]) * X + i[idx, 0]
        h = flat[c]
        hi = idx[h]
        hit[hi], th[hi], face[hi], cell[hi] = True, tn[h], 2 * ax[h] + (sta[h] > 0), c[h]
        active[hi] = False
    with np.errstate(all="ignore"):
        p = np.where(start[:, None], o, fma(d, th[:, None], o)).astype(f32)
        M = fr["M"]
        hh = [fma(f32(1), M[4 * k + 3], fma(p[:, 2], M[4 * k + 2], fma(p[:, 1], M[4 * k + 1], (p[:, 0] * M[4 * k]).astype(f32)))) for k in (2, 3)]
        cz = (hh[0] / hh[1]).astype(f32)
        drawn = hit & (hh[1] > 0) & (f32(0) <= cz) & (cz < f32(1))
        if scene is not None:
            drawn &= cz <= np.ascontiguousarray(scene, f32).reshape(-1)
    return {"hit": hit, "start": start, "drawn": drawn, "face": face, "cell": np.where(hit, cell, 0), "advances": adv, "t": th, "cz": cz, "p": p, "rays": R}


# ---- step 5 -------------------------------------------------------------------------------------------------------------------------------------
def light_vectors(fr, p):
    """L per hit point: float32[n][3]"""
    n = len(p)
    with np.errstate(all="ignore"):
        if fr["point"]:
            q = local_point(fr, fr["light_pt"])
            v = [(q[a] - p[:, a]).astype(f32) for a in range(3)]
            l2 = dot3(v[0], v[1], v[2], v[0], v[1], v[2])
            ok = (l2 > 0) & (l2 <= FLT_MAX)
            r = (f32(1) / np.sqrt(l2)).astype(f32)
            return np.stack([np.where(ok, (v[a] * r).astype(f32), f32(0)) for a in range(3)], 1).astype(f32)
        w, lp = fr["world_i"].reshape(3, 4), fr["light_pt"]
        l = [dot3(lp[0], lp[1], lp[2], w[a, 0], w[a, 1], w[a, 2]) for a in range(3)]
        r = f32(f32(1) / np.sqrt(dot3(l[0], l[1], l[2], l[0], l[1], l[2])))
        return np.tile(np.array([f32(l[a] * r) for a in range(3)], f32), (n, 1))


def shade(C, fr, albedo):
    """src per pixel, float32[n][3] (meaningful where C["drawn"])"""
    albedo = np.asarray(albedo, f32)
    L = light_vectors(fr, C["p"])
    face = C["face"]
    with np.errstate(all="ignore"):
        La = np.take_along_axis(L, np.minimum(face >> 1, 2)[:, None], 1)[:, 0]
        ndl = np.where(face < 6, np.fmax(f32(0), (np.where(face & 1, f32(-1), f32(1)) * La).astype(f32)), f32(0)).astype(f32)
        lc, am = fr["light_color"], fr["ambient"]
        return np.stack([((f32(albedo[c] * albedo[3]) * fma(ndl, f32(lc[3] * lc[c]), f32(am[3] * am[c]))).astype(f32) * INV_2PI).astype(f32)
                         for c in range(3)], 1)


# ---- step 6 -------------------------------------------------------------------------------------------------------------------------------------
def words(C):
    w = np.uint64(HIT) | (C["drawn"].astype(np.uint64) << np.uint64(62)) | (C["face"].astype(np.uint64) << np.uint64(32)) | C["cell"].astype(np.uint64)
    return np.where(C["hit"], w, np.uint64(0))


def draw(S, fr, W, H, albedo, target=None, scene=None, R=None):
    """-> dict: hits uint64[H][W], depth float32[H][W], target_float float32[H][W][4], target uint8[H][W][4] (over `target`, default all zero),
    cast (the per-pixel record)"""
    C = cast(S, fr, W, H, scene, R)
    src = shade(C, fr, albedo)
    dr = C["drawn"]
    behind = np.ones(W * H, f32) if scene is None else np.ascontiguousarray(scene, f32).reshape(-1)
    tf = np.zeros((W * H, 4), f32)
    tf[dr, :3], tf[dr, 3] = src[dr], 1
    out = (np.zeros((H, W, 4), np.uint8) if target is None else np.ascontiguousarray(target, np.uint8)).reshape(-1, 4).copy()
    out[dr, :3], out[dr, 3] = pd.to_unorm8(src[dr]), 255
    return {"hits": words(C).reshape(H, W), "depth": np.where(dr, C["cz"], behind).astype(f32).reshape(H, W), "target_float": tf.reshape(H, W, 4),
            "target": out.reshape(H, W, 4), "cast": C}


# ---- the same in plain loops, on Python floats that hold float32 values ----------------------------------------------------------------------------
# A product of two float32 is exact in a float64; a sum, a quotient and a square root of float32 values rounded to float64 and then to float32
# are the correctly rounded float32 results (53 >= 2 * 24 + 2).  The fused multiply-add is fma_ref's: the float64 sum rounded to odd first.
def _r(x):
    return struct.unpack("f", struct.pack("f", x))[0] if abs(x) < 3.4028235677973366e+38 else (x if x != x or abs(x) == math.inf else math.copysign(math.inf, x))


def _fma(a, b, c):
    p = a * b
    s = p + c
    if s - s != 0:
        return _r(s)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0 and not struct.unpack("<q", struct.pack("<d", s))[0] & 1:
        s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return _r(s)


def _div(a, b):
    if b == 0:
        return math.nan if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return _r(a / b)


def _dot3(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, _r(ax * bx)))


def _rsq(x):
    return _div(1.0, _r(math.sqrt(x))) if x >= 0 else math.nan


def _unorm8(v):
    return 0 if not v > 0 else 255 if v >= 1 else int(_r(_r(v * 255.0) + 0.5))


def draw_loops(S, fr, W, H, albedo, target=None, scene=None):
    """`draw` pixel by pixel -> (hits, depth, target_float, target)"""
    S = np.ascontiguousarray(S, bool)
    Z, Y, X = S.shape
    N = (X, Y, Z)
    solid = S.reshape(-1).tolist()
    Mi, M = [float(v) for v in fr["wvp_i"]], [float(v) for v in fr["M"]]
    wi = [float(v) for v in fr["world_i"]]

    def local(p):
        return [_fma(wi[4 * a + 3], 1.0, _fma(p[2], wi[4 * a + 2], _fma(p[1], wi[4 * a + 1], _r(p[0] * wi[4 * a])))) for a in range(3)]

    eye = local([float(v) for v in fr["eye"]])
    lp = [float(v) for v in fr["light_pt"]]
    lq = local(lp)
    ld = [_dot3(lp[0], lp[1], lp[2], wi[4 * a], wi[4 * a + 1], wi[4 * a + 2]) for a in range(3)]
    lr = _rsq(_dot3(ld[0], ld[1], ld[2], ld[0], ld[1], ld[2]))
    ld = [_r(v * lr) for v in ld]
    al, lc, am = [float(v) for v in np.asarray(albedo, f32)], [float(v) for v in fr["light_color"]], [float(v) for v in fr["ambient"]]
    k = [_r(al[c] * al[3]) for c in range(3)]
    lcc, amc = [_r(lc[3] * lc[c]) for c in range(3)], [_r(am[3] * am[c]) for c in range(3)]
    hits = np.zeros((H, W), np.uint64)
    depth = np.ones((H, W), f32) if scene is None else np.ascontiguousarray(scene, f32).reshape(H, W).copy()
    tf = np.zeros((H, W, 4), f32)
    out = np.zeros((H, W, 4), np.uint8) if target is None else np.ascontiguousarray(target, np.uint8).reshape(H, W, 4).copy()
    fmax = float(FLT_MAX)

    def plane(i, st, n, o, r):
        if not st:
            return fmax
        return _r(_r(_fma(_div(float(i + (st > 0)), float(n)), 2.0, -1.0) - o) * r)

    for py in range(H):
        v = _div(_r(py + 0.5), float(H))
        qy = _fma(v, -2.0, 1.0)
        for px in range(W):
            # 1: the ray
            qx = _fma(_div(_r(px + 0.5), float(W)), 2.0, -1.0)
            h = [_dot3(qx, qy, 1.0, Mi[4 * r], Mi[4 * r + 1], Mi[4 * r + 3]) for r in range(4)]
            o = [_div(h[a], h[3]) for a in range(3)]
            d = [_r(o[a] + -eye[a]) for a in range(3)]
            rl = _rsq(_dot3(d[0], d[1], d[2], d[0], d[1], d[2]))
            d = [_r(v_ * rl) for v_ in d]
            e = -1
            if not (abs(o[0]) <= 1 and abs(o[1]) <= 1 and abs(o[2]) <= 1):
                U, ok = fmax, False
                for a in range(3):
                    sgn = float((0 < d[a]) - (d[a] < 0))
                    q = _div(_r(-o[a] + -sgn), d[a])
                    j, kk = (a + 1) % 3, (a + 2) % 3
                    if not q >= 0 or not 1 >= abs(_fma(d[j], q, o[j])) or not 1 >= abs(_fma(d[kk], q, o[kk])):
                        continue
                    if q < U:
                        U, ok, e = q, True, a
                moved = [_fma(d[a], U, o[a]) for a in range(3)]
                o = [min(max(m if m == m else -1.0, -1.0), 1.0) for m in moved]
                if not ok:
                    continue
            # 2: the start
            i = [min(max(int(math.floor(_r(_fma(o[a], 0.5, 0.5) * N[a]))), 0), N[a] - 1) for a in range(3)]
            st = [(d[a] > 0) - (d[a] < 0) for a in range(3)]
            r = [_div(1.0, d[a]) for a in range(3)]
            hit, start, face, th = False, False, 6, 0.0
            if solid[(i[2] * Y + i[1]) * X + i[0]]:
                hit = start = True
                face = 2 * e + (d[e] > 0) if e >= 0 else 6
            else:
                # 3: the walk
                t = [plane(i[a], st[a], N[a], o[a], r[a]) for a in range(3)]
                for _ in range(X + Y + Z):
                    a = 0 if t[0] <= t[1] and t[0] <= t[2] else 1 if t[1] <= t[2] else 2
                    if not st[a]:
                        break
                    i[a] += st[a]
                    if not 0 <= i[a] < N[a]:
                        break
                    tn = t[a]
                    t[a] = plane(i[a], st[a], N[a], o[a], r[a])
                    if solid[(i[2] * Y + i[1]) * X + i[0]]:
                        hit, th, face = True, tn, 2 * a + (st[a] > 0)
                        break
            if not hit:
                continue
            # 4: visible
            p = o if start else [_fma(d[a], th, o[a]) for a in range(3)]
            h2, h3 = [_fma(1.0, M[4 * q + 3], _fma(p[2], M[4 * q + 2], _fma(p[1], M[4 * q + 1], _r(p[0] * M[4 * q])))) for q in (2, 3)]
            cz = _div(h2, h3)
            drawn = h3 > 0 and 0 <= cz and cz < 1 and (scene is None or cz <= float(depth[py, px]))
            hits[py, px] = HIT | (DRAWN if drawn else 0) | (face << 32) | ((i[2] * Y + i[1]) * X + i[0])
            if not drawn:
                continue
            # 5: shade
            if fr["point"]:
                vv = [_r(lq[a] - p[a]) for a in range(3)]
                l2 = _dot3(vv[0], vv[1], vv[2], vv[0], vv[1], vv[2])
                ok = l2 > 0 and l2 <= fmax
                rr = _rsq(l2)
                L = [_r(vv[a] * rr) if ok else 0.0 for a in range(3)]
            else:
                L = ld
            ndl = 0.0
            if face < 6:
                x = (-1.0 if face & 1 else 1.0) * L[face >> 1]
                ndl = x if x > 0 else 0.0
            src = [_r(_r(k[c] * _fma(ndl, lcc[c], amc[c])) * float(INV_2PI)) for c in range(3)]
            # 6: store
            depth[py, px] = cz
            tf[py, px] = src + [1.0]
            out[py, px] = [_unorm8(s) for s in src] + [255]
    return hits, depth, tf, out
