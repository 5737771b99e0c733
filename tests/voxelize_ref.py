"""numpy model of the mesh voxeliser (include/fluidx_hip.h fx_set_obstacle_meshes, fluidx12_amd/csrc/fx_voxelize.hip).

The rule, restated step by step as the header numbers it: a float32 transform with every operation rounded on its own, one float32 multiply
and a round-to-nearest-even per coordinate, int64 from there.  The model tests every column of the grid against every triangle (no bounding
boxes, no patches, no atomics) and fills with np.bitwise_xor.accumulate.  Also the meshes the tests share: a box, a UV sphere, a torus.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

f32 = np.float32
CLAMP = f32(262144.0)


def transform(pos, m):
    """step 1: p_a = ((m[4a] * x + m[4a+1] * y) + m[4a+2] * z) + m[4a+3] in float32, each operation rounded; m None = the bits untouched"""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    if m is None:
        return pos
    m = np.asarray(m, f32).reshape(12)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    out = np.empty_like(pos)
    with np.errstate(all="ignore"):
        for a in range(3):
            out[:, a] = ((m[4 * a] * x + m[4 * a + 1] * y) + m[4 * a + 2] * z) + m[4 * a + 3]
    return out


def quantise(p, dims):
    """step 2 -> (q int64 (n, 3), finite bool (n,)): 1 / 256 of a cell, clamped to +-2^18, ties to even"""
    q = np.zeros(p.shape, np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            t = (p[:, a] * f32(256 * dims[a])).astype(f32)
            t = np.minimum(np.maximum(t, -CLAMP), CLAMP)
            q[:, a] = np.where(np.isnan(t), 0, np.rint(t)).astype(np.int64)
    return q, np.isfinite(p).all(axis=1)


def _edge(p, r, Py, Pz):
    """step 4 for the directed edge p -> r; p, r (n, 3) int64, Py / Pz broadcast against (n, 1, 1)"""
    dy = (r[:, 1] - p[:, 1])[:, None, None]
    dz = (r[:, 2] - p[:, 2])[:, None, None]
    E = dy * (Pz - p[:, 2][:, None, None]) - dz * (Py - p[:, 1][:, None, None])
    return (E > 0) | ((E == 0) & ((dy > 0) | ((dy == 0) & (dz > 0))))


def toggles(positions, indices, m, dims, chunk=256):
    """steps 1-5 for one mesh -> (toggle bits uint8 (Z, Y, X + 1), skipped triangles)"""
    X, Y, Z = dims
    pos = np.asarray(positions, f32).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    tog = np.zeros((Z, Y, X + 1), np.uint8)
    if idx.shape[0] == 0:
        return tog, 0
    q, finite = quantise(transform(pos, m), dims)
    nv = pos.shape[0]
    inrange = (idx < nv).all(axis=1)
    safe = np.where(idx < nv, idx, 0)
    ok = inrange & finite[safe].all(axis=1) if nv else inrange
    skipped = int((~ok).sum())
    idx = idx[ok]
    a, b, c = q[idx[:, 0]], q[idx[:, 1]], q[idx[:, 2]]
    A = (b[:, 1] - a[:, 1]) * (c[:, 2] - a[:, 2]) - (b[:, 2] - a[:, 2]) * (c[:, 1] - a[:, 1])
    keep = A != 0                                                    # step 3: edge-on triangles cover nothing
    a, b, c, A = a[keep], b[keep], c[keep], A[keep]
    swap = A < 0
    b, c = np.where(swap[:, None], c, b), np.where(swap[:, None], b, c)
    A = np.abs(A)
    Py = (256 * np.arange(Y, dtype=np.int64) + 128)[None, None, :]
    Pz = (256 * np.arange(Z, dtype=np.int64) + 128)[None, :, None]
    for s in range(0, A.shape[0], chunk):
        ta, tb, tc, tA = a[s:s + chunk], b[s:s + chunk], c[s:s + chunk], A[s:s + chunk][:, None, None]
        cov = _edge(ta, tb, Py, Pz) & _edge(tb, tc, Py, Pz) & _edge(tc, ta, Py, Pz)          # (n, Z, Y)
        e1, e2 = tb - ta, tc - ta
        ny = (e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2])[:, None, None]
        nz = (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])[:, None, None]
        T = (ta[:, 0][:, None, None] - 128) * tA - (ny * (Py - ta[:, 1][:, None, None]) + nz * (Pz - ta[:, 2][:, None, None]))
        i0 = np.clip(-((-T) // (256 * tA)), 0, X)                     # the ceiling of the exact quotient
        t, k, j = np.nonzero(cov)
        np.bitwise_xor.at(tog, (k, j, i0[t, k, j]), 1)
    return tog, skipped


def voxelise(meshes, dims):
    """meshes: [(positions, indices, transform or None)] -> (mask uint8 (Z, Y, X) of 0 / 1, report dict): steps 6 and 7"""
    X, Y, Z = dims
    mask = np.zeros((Z, Y, X), np.uint8)
    open_columns = skipped = 0
    for positions, indices, m in meshes:
        tog, sk = toggles(positions, indices, m, dims)
        par = np.bitwise_xor.accumulate(tog, axis=2)
        mask |= par[:, :, :X]
        open_columns += int(par[:, :, X].sum())
        skipped += sk
    return mask, {"solid_cells": int(mask.sum()), "open_columns": open_columns, "skipped_triangles": skipped}


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def box_mesh(lo, hi):
    """12 triangles, outward winding; lo / hi in texture space"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], f32)
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
    tri = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(tri, np.uint32)


def cell_centre(dims, cell):
    return tuple((cell[a] + 0.5) / dims[a] for a in range(3))


def uv_sphere(center, radius, stacks=12, slices=24):
    """a closed UV sphere: two poles, stacks - 1 rings of `slices` vertices; radius a scalar or one per axis"""
    r = np.broadcast_to(np.asarray(radius, np.float64), (3,))
    v = [(0.0, 1.0, 0.0)]                                             # the poles on the y axis
    for i in range(1, stacks):
        th = np.pi * i / stacks
        for j in range(slices):
            ph = 2.0 * np.pi * j / slices
            v.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
    v.append((0.0, -1.0, 0.0))
    v = (np.asarray(center, np.float64)[None, :] + np.asarray(v) * r[None, :]).astype(f32)
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    south = 1 + (stacks - 1) * slices
    tri = []
    for j in range(slices):
        tri.append((0, ring(1, j), ring(1, j + 1)))
        tri.append((south, ring(stacks - 1, j + 1), ring(stacks - 1, j)))
    for i in range(1, stacks - 1):
        for j in range(slices):
            tri.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            tri.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return v, np.array(tri, np.uint32)


def torus(center, R, r, major=20, minor=10):
    """a closed torus about the z axis through `center`"""
    v = []
    for i in range(major):
        u = 2.0 * np.pi * i / major
        for j in range(minor):
            w = 2.0 * np.pi * j / minor
            v.append(((R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)))
    v = (np.asarray(center, np.float64)[None, :] + np.asarray(v)).astype(f32)
    at = lambda i, j: (i % major) * minor + j % minor
    tri = []
    for i in range(major):
        for j in range(minor):
            tri.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            tri.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return v, np.array(tri, np.uint32)


def translation(d):
    return np.array([1, 0, 0, d[0], 0, 1, 0, d[1], 0, 0, 1, d[2]], f32)


def rotation_translation(axis, angle, pivot, shift):
    """a rotation about `axis` through `pivot`, then a shift; float64 -> float32[12]: the entries are whatever they round to"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    p = np.asarray(pivot, np.float64)
    t = p - R @ p + np.asarray(shift, np.float64)
    return np.concatenate([R, t[:, None]], axis=1).astype(f32).reshape(12)
