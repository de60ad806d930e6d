"""The definition of the depth-camera fusion (include/mpdx.h, mpdx_tsdf_integrate) as numpy fp32, one rounded operation per step, in the kernel's
order - the arithmetic the kernel is held to bit for bit; the transform that follows is tests/edt_ref.py.  Also a float64 ray caster for spheres and
axis-aligned boxes that renders fp32 depth images (z along the optical axis, OpenCV frame: x right, y down, z forward, pixel (iu, iv) centred at
(iu, iv)), a look_at helper, and the scene of the tests.  Arrays are [nz, ny, nx], x fastest."""
import numpy as np

F = np.float32


# ------------------------------------------------------------------------------------------------------------------------ cameras
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world_from_cam 4x4 float64 of a camera at `eye` looking at `target` (z forward), y pointing away from `up` (down in the image)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, y, z, eye
    return M


def camera(depth, K, world_from_cam, depth_range=(0.1, 5.0)):
    """the record the kernel reads (fp32 everywhere), from float64 inputs as GridSDF.from_depth forms it: the inverse in float64, both rounded"""
    M = np.asarray(world_from_cam, np.float64)
    H = np.eye(4)
    H[:3] = M[:3]
    inv = np.linalg.inv(H)
    return dict(depth=np.ascontiguousarray(depth, F), fx=F(K[0]), fy=F(K[1]), cx=F(K[2]), cy=F(K[3]), A=inv[:3].astype(F), B=H[:3].astype(F),
                min_depth=F(depth_range[0]), max_depth=F(depth_range[1]))


# ------------------------------------------------------------------------------------------------------------------------ the fusion
def node_positions(shape, origin, cell):
    """(p0, p1, p2) fp32 [n_nodes]: origin_j + (float)i_j * cell, one rounded product and one rounded sum"""
    nz, ny, nx = shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return tuple(F(origin[j]) + i.reshape(-1).astype(F) * F(cell) for j, i in enumerate((ix, iy, iz)))


def _row(M, j, a, b, c):
    return ((M[j, 0] * a + M[j, 1] * b) + M[j, 2] * c) + M[j, 3]


def observe_ref(cam, p, spheres=None, trunc=0.1, with_mask=True):
    """one camera's observation of the nodes p: (ok [n] bool, o [n] fp32, s [n] fp32, stage [n] int8) - stage says where a node left: 0 behind the
    camera, 1 outside the image, 2 no measurement, 3 masked, 4 occluded, 5 an observation"""
    p0, p1, p2 = p
    A = cam["A"]
    h, w = cam["depth"].shape
    n = p0.size
    stage = np.zeros(n, np.int8)
    with np.errstate(all="ignore"):
        x2 = _row(A, 2, p0, p1, p2)
        front = x2 > 0
        x0, x1 = _row(A, 0, p0, p1, p2), _row(A, 1, p0, p1, p2)
        u = cam["fx"] * (x0 / x2) + cam["cx"]
        v = cam["fy"] * (x1 / x2) + cam["cy"]
        ru, rv = np.rint(u), np.rint(v)
        inside = front & (ru >= 0) & (ru <= F(w - 1)) & (rv >= 0) & (rv <= F(h - 1))
        iu, iv = np.where(inside, ru, 0).astype(np.int64), np.where(inside, rv, 0).astype(np.int64)
        d = cam["depth"][iv, iu]
        meas = inside & (d >= cam["min_depth"]) & (d <= cam["max_depth"])
        masked = np.zeros(n, bool)
        if spheres is not None and len(spheres) and with_mask:
            sp = np.asarray(spheres, F)
            q0 = ((ru - cam["cx"]) / cam["fx"]) * d
            q1 = ((rv - cam["cy"]) / cam["fy"]) * d
            B = cam["B"]
            P = [_row(B, j, q0, q1, d) for j in range(3)]
            for c in sp:
                dx, dy, dz = P[0] - c[0], P[1] - c[1], P[2] - c[2]
                masked |= ((dx * dx + dy * dy) + dz * dz) < c[3] * c[3]
            masked &= meas
        s = d - x2
        occl = meas & ~masked & (s < -F(trunc))
        ok = meas & ~masked & ~occl
        o = np.fmin(s, F(trunc)) / F(trunc)
    stage[front] = 1
    stage[inside] = 2
    stage[meas] = 5
    stage[masked] = 3
    stage[occl] = 4
    return ok, o.astype(F), s.astype(F), stage


def integrate_ref(tsdf, weight, cams, shape, origin, cell, trunc, max_weight, spheres=None):
    """mpdx_tsdf_integrate: (tsdf, weight, occ) after the cameras, in order; inputs are not changed"""
    T = np.array(tsdf, F).reshape(-1).copy()
    W = np.array(weight, F).reshape(-1).copy()
    p = node_positions(shape, origin, cell)
    for cam in cams:
        ok, o, _, _ = observe_ref(cam, p, spheres, trunc)
        w1 = W + F(1)
        Tn = (T * W + o) / w1
        T = np.where(ok, Tn, T).astype(F)
        W = np.where(ok, np.fmin(w1, F(max_weight)), W).astype(F)
    occ = (W > 0) & (T < 0)
    return T.reshape(shape), W.reshape(shape), occ.reshape(shape).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------ ray caster
def render(spheres, boxes, K, world_from_cam, w, h):
    """fp32 depth [h, w] of the scene (spheres [n, 4] centre, radius; boxes [m, 6] centre, half extents), float64 throughout: the z of the first hit
    along each pixel centre's ray; 0 where the ray hits nothing"""
    fx, fy, cx, cy = (float(v) for v in K)
    M = np.asarray(world_from_cam, np.float64)
    iv, iu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = np.stack([(iu - cx) / fx, (iv - cy) / fy, np.ones_like(iu)], -1)       # z = 1: the ray parameter is the depth
    dw = dc @ M[:3, :3].T
    o = M[:3, 3]
    best = np.full((h, w), np.inf)
    for c in np.asarray(spheres, np.float64).reshape(-1, 4):
        oc = o - c[:3]
        a = (dw * dw).sum(-1)
        b = (dw * oc).sum(-1)
        cc = oc @ oc - c[3] ** 2
        disc = b * b - a * cc
        with np.errstate(invalid="ignore"):
            t = (-b - np.sqrt(disc)) / a
        best = np.where((disc >= 0) & (t > 0) & (t < best), t, best)
    for bx in np.asarray(boxes, np.float64).reshape(-1, 6):
        lo, hi = bx[:3] - bx[3:], bx[:3] + bx[3:]
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo - o) / dw, (hi - o) / dw
        tmin = np.nanmax(np.minimum(t1, t2), -1)
        tmax = np.nanmin(np.maximum(t1, t2), -1)
        hit = (tmax >= tmin) & (tmin > 0)
        best = np.where(hit & (tmin < best), tmin, best)
    return np.where(np.isfinite(best), best, 0.0).astype(F)


def scene_sdf(points, spheres, boxes):
    """float64 signed distance of points [..., 3] to the union of the primitives"""
    p = np.asarray(points, np.float64)
    sd = np.full(p.shape[:-1], np.inf)
    for c in np.asarray(spheres, np.float64).reshape(-1, 4):
        sd = np.minimum(sd, np.linalg.norm(p - c[:3], axis=-1) - c[3])
    for bx in np.asarray(boxes, np.float64).reshape(-1, 6):
        d = np.abs(p - bx[:3]) - bx[3:]
        sd = np.minimum(sd, np.minimum(d.max(-1), 0.0) + np.linalg.norm(np.maximum(d, 0.0), axis=-1))
    return sd


# ------------------------------------------------------------------------------------------------------------------------ the tests' scene
SHAPE = (23, 29, 37)                       # (nz, ny, nx): odd, 24679 nodes (not a multiple of 256)
CELL = 0.05
ORIGIN = (-0.93, -0.71, -0.57)
SPHERES = np.array([[0.35, 0.15, -0.05, 0.22], [-0.40, -0.20, 0.05, 0.18]])
BOX = np.array([[-0.05, 0.35, -0.15, 0.14, 0.10, 0.16]])
FLOOR = np.array([[0.0, 0.0, -0.62, 4.0, 4.0, 0.05]])     # top face at z = -0.57: under the grid's lowest node plane ... nearly
K1, WH1 = (40.0, 38.0, 23.5, 19.5), (48, 40)
K2, WH2 = (30.0, 29.0, 16.2, 13.1), (33, 27)
EYE1, EYE2 = (1.9, 0.6, 1.1), (-1.4, -1.7, 0.9)


def nodes_xyz(shape=SHAPE, origin=ORIGIN, cell=CELL):
    """float64 [nz, ny, nx, 3] of the fp32 node positions"""
    p = node_positions(shape, origin, cell)
    return np.stack([v.astype(np.float64).reshape(shape) for v in p], -1)
