"""The definition of the occupancy transform (include/mpdx.h, mpdx_sdf_grid_from_occupancy / mpdx_occupancy_from_points) as brute-force numpy:
integer d2 over all node pairs, the fp32 formula for s, the gradient plane, the voxelisation.  Arrays are [nz, ny, nx] (nz = 1 in 2-D), x fastest.
Every fp32 step is one numpy float32 operation, so each is rounded once - the arithmetic the kernels are held to bit for bit."""
from functools import lru_cache

import numpy as np

F = np.float32


def sentinel(shape):
    nz, ny, nx = shape
    return (nx + ny + nz) ** 2


def d2_ref(occ):
    """occ [nz, ny, nx] (non-zero = occupied) -> int32 [nz, ny, nx]: per node the smallest squared distance (in cells) to a node of the OTHER side;
    (nx + ny + nz)^2 where there is none.  All pairs, in chunks."""
    occ = np.asarray(occ) != 0
    shape = occ.shape
    idx = np.stack(np.meshgrid(*[np.arange(v, dtype=np.int32) for v in shape], indexing="ij"), -1).reshape(-1, 3)
    o = occ.reshape(-1)
    out = np.full(o.size, sentinel(shape), np.int64)
    for side in (False, True):                      # nodes of this side look for the nearest node of the other
        mine, other = np.nonzero(o == side)[0], np.nonzero(o != side)[0]
        if not other.size:
            continue
        seeds = idx[other].astype(np.float64)         # |a - b|^2 = |a|^2 + |b|^2 - 2 a.b in float64: integers below 2^53, exact
        s2 = (seeds * seeds).sum(1)
        step = max(1, (1 << 23) // other.size)
        for lo in range(0, mine.size, step):
            a = idx[mine[lo: lo + step]].astype(np.float64)
            d = (a * a).sum(1)[:, None] + s2[None] - 2.0 * (a @ seeds.T)
            out[mine[lo: lo + step]] = np.rint(d.min(1)).astype(np.int64)
    return out.reshape(shape).astype(np.int32)


def sdf_ref(d2, occ, cell, inflate=0.0):
    """fp32, every step rounded: s = cell * (sqrt(d2) - 0.5) - inflate at a free node, -(cell * (sqrt(d2) - 0.5)) - inflate at an occupied one"""
    occ = np.asarray(occ) != 0
    t = F(cell) * (np.sqrt(d2.astype(F)) - F(0.5))
    assert t.dtype == F
    return (np.where(occ, -t, t) - F(inflate)).astype(F)


def grad_ref(s, cell):
    """[nz, ny, nx, 4]: central differences (s[i+1] - s[i-1]) * k2 inside, one-sided (.) * k1 at the faces, k1 = 1 / cell, k2 = 0.5 / cell in fp32;
    the unused axis (nz = 1) and the fourth word are 0"""
    assert s.dtype == F
    k1, k2 = F(1.0) / F(cell), F(0.5) / F(cell)
    g = np.zeros(s.shape + (4,), F)
    for j, ax in enumerate((2, 1, 0)):              # x, y, z
        n = s.shape[ax]
        if n == 1:
            continue
        v = np.moveaxis(s, ax, 0)
        d = np.empty_like(v)
        d[1:-1] = (v[2:] - v[:-2]) * k2
        d[0] = (v[1] - v[0]) * k1
        d[-1] = (v[-1] - v[-2]) * k1
        g[..., j] = np.moveaxis(d, 0, ax)
    return g


def voxelise_ref(points, shape, origin, cell, occ=None):
    """points [P, 3] fp32 -> occupancy bytes [nz, ny, nx] (accumulated into `occ` if given): u = (p - origin) * (1 / cell) in fp32, i = rint(u) half to
    even; a point with a non-finite used coordinate or an index outside the grid is dropped; z is ignored when nz = 1"""
    nz, ny, nx = shape
    n = np.array([nx, ny, nz])
    dim = 2 if nz == 1 else 3
    occ = np.zeros(shape, np.uint8) if occ is None else occ.copy()
    p = np.asarray(points, F)[:, :dim]
    inv = F(1.0) / F(cell)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((p - np.asarray(origin, F)[:dim]) * inv)
        keep = ((r >= 0) & (r <= (n[:dim] - 1).astype(F))).all(1)
    i = np.zeros((int(keep.sum()), 3), np.int64)
    i[:, :dim] = r[keep].astype(np.int64)
    occ[i[:, 2], i[:, 1], i[:, 0]] = 1
    return occ


# ---- the shapes and patterns of the GPU test (tests/test_gpu_occupancy.py); each reference is computed once per session
SHAPES = [(17, 13, 9), (65, 33, 1), (70, 7, 5), (300, 3, 2), (2, 2, 2), (4096, 2, 2), (3, 1000, 2), (2, 3, 260)]    # (nx, ny, nz)
PATTERNS = ["random3", "random50", "corner", "one_free", "all_free", "all_occupied"]


def pattern(shape_xyz, name):
    nx, ny, nz = shape_xyz
    shape = (nz, ny, nx)
    rng = np.random.default_rng(0)
    if name == "random3":
        return (rng.random(shape) < 0.03).astype(np.uint8)
    if name == "random50":
        return (rng.random(shape) < 0.5).astype(np.uint8)
    occ = np.zeros(shape, np.uint8) if name in ("corner", "all_free") else np.ones(shape, np.uint8)
    if name == "corner":
        occ[-1, -1, -1] = 1
    if name == "one_free":
        occ[nz // 2, ny // 3, (2 * nx) // 3] = 0
    return occ


@lru_cache(maxsize=None)
def case(shape_xyz, name):
    """(occ uint8 [nz, ny, nx], d2 int32) of a shape x pattern"""
    occ = pattern(shape_xyz, name)
    d2 = d2_ref(occ)
    occ.setflags(write=False)
    d2.setflags(write=False)
    return occ, d2
