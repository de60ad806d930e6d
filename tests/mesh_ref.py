"""The arithmetic contract of the mesh producer (include/mpdx.h, mpdx_sdf_grid_from_mesh) restated in float64 numpy, and the procedural meshes of its
tests.  Node positions come from the fp32 product and sum the kernel takes and are cast up; everything after that is float64: Ericson's closest
point of a closed triangle (vertex, edge or face region), the distance measured from that closest point, Van Oosterom and Strackee's solid angle.
Arrays of node values are [nz, ny, nx] (x fastest), as every grid plane."""
from functools import lru_cache

import numpy as np

F32 = np.float32
FACE, EDGE, VERTEX = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------- the field
def nodes(n, origin, cell):
    """[nz, ny, nx, 3] float64: node (ix, iy, iz) at origin_j + (float)i_j * cell, the product and the sum each rounded once in fp32"""
    ax = [(F32(origin[j]) + np.arange(n[j], dtype=F32) * F32(cell)).astype(F32) for j in range(3)]
    assert all(a.dtype == F32 for a in ax)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1).astype(np.float64)


def _dot(u, v):
    return (u * v).sum(-1)


def closest_point(p, a, b, c):
    """Ericson, Real-Time Collision Detection 5.1.5, vectorised: p [N, 1, 3], a / b / c [F, 3] -> (cp [N, F, 3], feature [N, F] of FACE / EDGE / VERTEX).
    The regions are tried in the book's order: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, the face."""
    ab, ac, bc = b - a, c - a, c - b
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    region = np.select(conds, [0, 1, 2, 3, 4, 5], 6)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
        cands = [a + 0 * p, b + 0 * p, a + t_ab[..., None] * ab, c + 0 * p, a + t_ac[..., None] * ac, b + t_bc[..., None] * bc,
                 a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]]
    out = cands[6]
    for k in range(6):
        out = np.where((region == k)[..., None], cands[k], out)
    feature = np.select([region == 6, (region == 2) | (region == 4) | (region == 5)], [FACE, EDGE], VERTEX)
    return out, feature


def solid_angles(p, a, b, c):
    """Omega [N, F] = 2 atan2(det[A B C], |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|), A = a - p ...: positive for a face seen from inside a mesh whose
    faces are counter-clockwise seen from outside"""
    A, B, C = a - p, b - p, c - p
    la, lb, lc = np.linalg.norm(A, axis=-1), np.linalg.norm(B, axis=-1), np.linalg.norm(C, axis=-1)
    det = _dot(A, np.cross(B, C))
    return 2.0 * np.arctan2(det, la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb)


def field_at(P, V, F, winding=True, chunk=48):
    """P [N, 3] float64, V [nv, 3], F [nf, 3] -> (d [N], w [N] or None, feature [N] of each node's nearest point)"""
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64)
    N = P.shape[0]
    best, feat, w = np.full(N, np.inf), np.zeros(N, np.int64), np.zeros(N)
    p = P[:, None, :]
    for lo in range(0, F.shape[0], chunk):
        f = F[lo: lo + chunk]
        a, b, c = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
        cp, ft = closest_point(p, a, b, c)
        r = p - cp
        d2 = _dot(r, r)
        k = d2.argmin(1)
        m = d2[np.arange(N), k]
        better = m < best
        best = np.where(better, m, best)
        feat = np.where(better, ft[np.arange(N), k], feat)
        if winding:
            w += solid_angles(p, a, b, c).sum(1)
    return np.sqrt(best), (w / (4.0 * np.pi) if winding else None), feat


def field(V, F, n, origin, cell, winding=True, with_feature=False):
    """-> (P [nz, ny, nx, 3], d [nz, ny, nx], w [nz, ny, nx] or None[, feature])"""
    P = nodes(n, origin, cell)
    shp = P.shape[:-1]
    d, w, feat = field_at(P.reshape(-1, 3), V, F, winding)
    out = (P, d.reshape(shp), None if w is None else w.reshape(shp))
    return out + (feat.reshape(shp),) if with_feature else out


def signed_volume(V, F):
    V = np.asarray(V, np.float64)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return float(_dot(a, np.cross(b, c)).sum() / 6.0)


def box_sdf(P, lo, hi):
    """the closed-form signed distance of an axis-aligned box"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    q = np.abs(P - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


# ---------------------------------------------------------------------------------------------------------------- the meshes
def icosphere(subdivisions, r, centre):
    """(V float64 [nv, 3] on the sphere, F int32 [20 * 4^subdivisions, 3]), faces counter-clockwise seen from outside"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(subdivisions):
        mid, G = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                v = V[i] + V[j]
                V.append(v / np.linalg.norm(v))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    V = np.asarray(centre, np.float64) + r * np.array(V)
    F = np.array(F, np.int32)
    assert signed_volume(V - np.asarray(centre, np.float64), F) > 0
    return V, F


def box(lo, hi):
    """12 faces, outward orientation"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    V = np.array([[(lo, hi)[(i >> j) & 1][j] for j in range(3)] for i in range(8)], np.float64)   # vertex i: bit j picks hi along axis j
    F = np.array([(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)], np.int32)
    assert abs(signed_volume(V, F) - np.prod(hi - lo)) < 1e-12
    return V, F


def concat(*meshes):
    Vs, Fs, off = [], [], 0
    for V, F in meshes:
        Vs.append(V)
        Fs.append(F + off)
        off += V.shape[0]
    return np.concatenate(Vs), np.concatenate(Fs).astype(np.int32)


def open_cap(subdivisions=2, r=0.3, centre=(0.1, -0.05, 0.4), z_cut=0.55):
    """the icosphere without the faces whose centroid has z >= z_cut: an open sheet"""
    V, F = icosphere(subdivisions, r, centre)
    keep = V[F].mean(1)[:, 2] < z_cut
    return V, F[keep]


# ---------------------------------------------------------------------------------------------------------------- the cases of tests/test_gpu_mesh_sdf.py
GRID = dict(n=(23, 21, 19), origin=(-0.5037, -0.4537, -0.0537), cell=0.05)
COARSE = dict(n=(13, 11, 9), origin=(-0.5037, -0.4537, -0.0537), cell=0.09)
BOX = ((-0.2, -0.3, 0.1), (0.25, 0.1, 0.5))


def mesh(name):
    if name == "box":
        return box(*BOX)
    if name == "sphere":
        return icosphere(2, 0.3, (0.1, -0.05, 0.4))
    if name == "two":
        return concat(icosphere(1, 0.25, (0.0, 0.0, 0.35)), box((0.3, -0.2, 0.0), (0.6, 0.2, 0.3)))
    if name == "open_cap":
        return open_cap()
    if name == "many":
        return concat(icosphere(3, 0.3, (0.1, -0.05, 0.4)), box((-0.45, -0.4, 0.0), (-0.25, -0.1, 0.25)))
    raise KeyError(name)


CASES = {"box": GRID, "sphere": GRID, "two": GRID, "open_cap": GRID, "many": COARSE}
CLOSED = ("box", "sphere", "two", "many")


@lru_cache(maxsize=None)
def case(name):
    """dict(V32 fp32 [nv, 3] - what the device is given -, F int32, grid, P, d, w, feature, L) of a named case; the reference is evaluated on V32 cast up,
    once per session, and is read-only.  L = the largest absolute coordinate among nodes and vertices."""
    V, F = mesh(name)
    V32 = V.astype(F32)
    g = CASES[name]
    P, d, w, feat = field(V32.astype(np.float64), F, g["n"], g["origin"], g["cell"], with_feature=True)
    out = dict(V32=V32, F=F, grid=g, P=P, d=d, w=w, feature=feat, L=float(max(np.abs(P).max(), np.abs(V32).max())))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
