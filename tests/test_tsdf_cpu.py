"""CPU checks of the depth-camera fusion (csrc/tsdf.hpp, mpdx_tsdf_integrate): properties of the numpy reference (tests/tsdf_ref.py) itself on a
ray-cast scene, the mpdx_depth_camera layout against the C header, every host-side refusal of the entry point through the C ABI (host buffers
stand in for device pointers: nothing is launched, the method of tests/test_grid_sdf_cpu.py), the refusals of the Python surface, and the robot
spheres of the mask."""
import ctypes as C
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import tsdf_ref as R

ROOT = Path(__file__).resolve().parent.parent
SQ2 = math.sqrt(2.0) / 2.0


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def _scene(box=True):
    boxes = np.concatenate([R.BOX, R.FLOOR]) if box else R.FLOOR
    return R.SPHERES, boxes


def _cams(box=True, which=(0, 1)):
    """the two 48 x 40 cameras of the property tests, on the scene with or without the box"""
    sp, bx = _scene(box)
    out = []
    for k in which:
        eye = (R.EYE1, R.EYE2)[k]
        M = R.look_at(eye, (0.0, 0.0, -0.1))
        out.append(R.camera(R.render(sp, bx, R.K1, M, *R.WH1), R.K1, M))
    return out


def _band(cams, trunc):
    """per node the bound of the surface band (derivation in test_occupied_nodes_lie_in_the_surface_band): max over the cameras that see the node in
    front of them of trunc * k + x2 * (sqrt(2) / 2) / min(fx, fy), k the largest ray-length factor of the camera's image"""
    p = R.node_positions(R.SHAPE, R.ORIGIN, R.CELL)
    xyz = np.stack([v.astype(np.float64) for v in p], -1)
    bound = np.zeros(xyz.shape[0])
    for c in cams:
        h, w = c["depth"].shape
        fx, fy, cx, cy = (float(c[k]) for k in ("fx", "fy", "cx", "cy"))
        ku = max(abs(0 - cx), abs(w - 1 - cx)) / fx
        kv = max(abs(0 - cy), abs(h - 1 - cy)) / fy
        k = math.sqrt(1.0 + ku * ku + kv * kv)
        A = c["A"].astype(np.float64)
        z = xyz @ A[2, :3] + A[2, 3]
        bound = np.maximum(bound, np.where(z > 0, trunc * k + z * SQ2 / min(fx, fy), 0.0))
    return (bound + 1e-5).reshape(R.SHAPE)


def test_occupied_nodes_lie_in_the_surface_band_and_far_nodes_are_free():
    """Surface band.  A node is occupied only if T < 0, and T is a weighted mean of observations o, so some camera observed it with
    o < 0, i.e. -trunc <= s = d - x2 < 0: the pixel (iu, iv) it projects to measured d.  Let S be the surface point that pixel's centre ray hit (at
    depth d) and Q the point of that ray at the node's depth x2.  Along the ray, depth grows by 1 per k_pix = sqrt(1 + ((iu - cx) / fx)^2 +
    ((iv - cy) / fy)^2) of length, so |Q - S| = |d - x2| k_pix <= trunc * k, k the largest k_pix of the image.  The node projects within half a
    pixel of (iu, iv) along each axis, so at depth x2 it lies within x2 * sqrt((0.5 / fx)^2 + (0.5 / fy)^2) <= x2 * (sqrt(2) / 2) / min(fx, fy) =
    r_pix of Q.  Hence |node - S| <= trunc * k + r_pix, and the distance to the surface is at most that.  1e-5 covers the fp32 rounding of the node
    positions, the poses and the rendered depth (all below 1e-6 m at these sizes).
    Free space: the same bound read backwards - a node further than it from every surface (on either side) is never occupied."""
    sp, bx = _scene()
    cams = _cams()
    for trunc in (2 * R.CELL, 0.5 * R.CELL):
        z = np.zeros(R.SHAPE, np.float32)
        T, W, occ = R.integrate_ref(z, z, cams, R.SHAPE, R.ORIGIN, R.CELL, trunc, 20.0)
        sd = R.scene_sdf(R.nodes_xyz(), sp, bx)
        bound = _band(cams, trunc)
        o = occ != 0
        print(f"trunc {trunc}: occupied {int(o.sum())}, observed {int((W > 0).sum())}, max |sdf| / bound over occupied "
              f"{float((np.abs(sd) / bound)[o].max()):.3f}")
        assert o.any()
        assert (np.abs(sd)[o] <= bound[o]).all()
        far = (np.abs(sd) > bound) & (W > 0)
        assert far.sum() > 1000 and not o[far].any()


def test_a_removed_box_is_carved():
    """Frame 1 sees the box, frame 2 (same cameras) does not.  With max_weight 20 every node that stays occupied after frame 2 lies in the band of the
    scene WITHOUT the box (a node of the box's shell had o1 >= -1 and now o2 = 1 unless it is within trunc of what lies behind: T = (o1 + o2) / 2 >= 0).
    With max_weight 1 (and 3) and a saturated weight, one camera, each frame without the box moves T to (M T + 1) / (M + 1) at a node it observes with
    o = 1: T_n = 1 - (1 - T_0) (M / (M + 1))^n, so the node turns free after the smallest n with T_n >= 0."""
    sp, bx_free = _scene(box=False)
    with_box, without = _cams(True), _cams(False)
    trunc = 2 * R.CELL
    z = np.zeros(R.SHAPE, np.float32)
    T1, W1, occ1 = R.integrate_ref(z, z, with_box, R.SHAPE, R.ORIGIN, R.CELL, trunc, 20.0)
    T2, W2, occ2 = R.integrate_ref(T1, W1, without, R.SHAPE, R.ORIGIN, R.CELL, trunc, 20.0)
    sd_free = R.scene_sdf(R.nodes_xyz(), sp, bx_free)
    bound = _band(with_box, trunc)
    stale1 = (occ1 != 0) & (np.abs(sd_free) > bound)
    stale2 = (occ2 != 0) & (np.abs(sd_free) > bound)
    print(f"occupied nodes away from the remaining surfaces: {int(stale1.sum())} after frame 1, {int(stale2.sum())} after frame 2")
    assert stale1.sum() > 20 and stale2.sum() == 0
    p = R.node_positions(R.SHAPE, R.ORIGIN, R.CELL)
    for M in (1.0, 3.0):
        cam1, cam2 = with_box[:1], without[:1]
        T, W = z, z
        for _ in range(int(M) + 2):
            T, W, occ = R.integrate_ref(T, W, cam1, R.SHAPE, R.ORIGIN, R.CELL, trunc, M)
        ok, o, _, _ = R.observe_ref(cam2[0], p, trunc=trunc)
        sel = ((occ != 0) & (W == M)).reshape(-1) & ok & (o == 1)
        T0 = T.reshape(-1)[sel].astype(np.float64)
        n = np.arange(0, 40)[:, None]
        Tn = 1.0 - (1.0 - T0[None]) * (M / (M + 1.0)) ** n
        pred = np.argmax(Tn >= 0, 0)
        clear = np.abs(Tn[pred, np.arange(T0.size)]) > 1e-6                        # (a float64 value this close to 0 is left to the rounding)
        got = np.full(T0.size, -1)
        for k in range(1, 40):
            T, W, occ = R.integrate_ref(T, W, cam2, R.SHAPE, R.ORIGIN, R.CELL, trunc, M)
            now = (occ.reshape(-1)[sel] == 0) & (got < 0)
            got[now] = k
            if (got >= 0).all():
                break
        print(f"max_weight {M}: {int(sel.sum())} saturated box nodes, frames to clear {np.bincount(got[got >= 0]).tolist()}")
        assert sel.sum() > 10 and (got >= 0).all()
        assert np.array_equal(got[clear], pred[clear]) and clear.mean() > 0.9
        if M == 3.0:
            assert got.max() >= 2


def test_skips_leave_the_planes_untouched_and_unseen_nodes_stay_empty():
    cam = _cams()[0]
    p = R.node_positions(R.SHAPE, R.ORIGIN, R.CELL)
    rng = np.random.default_rng(4)
    T0 = rng.uniform(-1, 1, R.SHAPE).astype(np.float32)
    W0 = rng.integers(1, 6, R.SHAPE).astype(np.float32)
    mask = np.array([[*R.SPHERES[0, :3], R.SPHERES[0, 3] + 0.02]], np.float32)     # one scene sphere stands in for a robot link
    trunc = 0.5 * R.CELL
    T, W, _ = R.integrate_ref(T0, W0, [cam], R.SHAPE, R.ORIGIN, R.CELL, trunc, 20.0, spheres=mask)
    _, _, _, stage = R.observe_ref(cam, p, mask, trunc)
    stage = stage.reshape(R.SHAPE)
    counts = {s: int((stage == s).sum()) for s in range(6)}
    print("stages (behind, outside, no measurement, masked, occluded, observed):", counts)
    assert counts[3] > 0 and counts[4] > 0 and counts[5] > 0
    skipped = stage != 5
    assert np.array_equal(T[skipped], T0[skipped]) and np.array_equal(W[skipped], W0[skipped])
    assert (W[~skipped] == W0[~skipped] + 1).all()
    # from an empty map: a node no camera observed keeps W = 0 and is free
    z = np.zeros(R.SHAPE, np.float32)
    cams = _cams()
    T, W, occ = R.integrate_ref(z, z, cams, R.SHAPE, R.ORIGIN, R.CELL, trunc, 20.0)
    seen = np.zeros(R.SHAPE, bool)
    for c in cams:
        seen |= (R.observe_ref(c, p, trunc=trunc)[3] == 5).reshape(R.SHAPE)
    assert (~seen).sum() > 0 and (W[~seen] == 0).all() and not occ[~seen].any() and (W[seen] > 0).all()


def test_reference_formulas_on_a_hand_case():
    """One node, a camera at the origin looking along +z, one pixel: s = d - z, o = min(s, trunc) / trunc, T = (T W + o) / (W + 1), W capped."""
    cam = R.camera(np.full((1, 1), 2.0, np.float32), (10.0, 10.0, 0.0, 0.0), np.eye(4))   # u = 10 * 0.2 / 1.9 > 0.5 at ix = 1
    T, W, occ = R.integrate_ref(np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2), np.float32), [cam], (2, 2, 2), (0.0, 0.0, 1.9), 0.2, 0.2, 2.0)
    f = np.float32
    z0, z1 = f(1.9), f(1.9) + f(1.0) * f(0.2)
    assert T[0, 0, 0] == (f(2.0) - z0) / f(0.2) and W[0, 0, 0] == 1 and occ[0, 0, 0] == 0                            # s = 0.1
    assert T[1, 0, 0] == (f(2.0) - z1) / f(0.2) and T[1, 0, 0] < 0 and occ[1, 0, 0] == 1                             # s = -0.1
    assert (W[:, :, 1] == 0).all() and (W[:, 1, :] == 0).all()                                                         # outside the one pixel
    T, W, occ = R.integrate_ref(T, W, [cam, cam], (2, 2, 2), (0.0, 0.0, 1.9), 0.2, 0.2, 2.0)
    assert W[0, 0, 0] == 2 and W.max() == 2                                                                             # capped at max_weight


# ---------------------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_depth_camera_layout_matches_the_c_header(tmp_path):
    from mpd_public_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on this host")
    names = [f[0] for f in _lib.DepthCamera._fields_]
    src = tmp_path / "cam.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpdx.h"\nint main(void) { printf("%zu' + " %zu" * len(names) + '\\n", '
                   'sizeof(mpdx_depth_camera), ' + ", ".join(f"offsetof(mpdx_depth_camera, {n})" for n in names) + "); return 0; }\n")
    exe = tmp_path / "cam"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.DepthCamera)] + [getattr(_lib.DepthCamera, n).offset for n in names]
    assert C.sizeof(_lib.DepthCamera) == 136 and "mpdx_tsdf_integrate" in _lib.SIGNATURES


def _valid_args():
    """a VALID call of mpdx_tsdf_integrate on host buffers (never made: every refusal below breaks one argument first)"""
    from mpd_public_amd import _lib
    nodes = 4 * 3 * 2
    b = dict(depth=(C.c_float * 64)(), tsdf=(C.c_float * (nodes + 1))(), weight=(C.c_float * (nodes + 1))(), occ=(C.c_uint8 * nodes)(),
             spheres=(C.c_float * 8)(0.1, 0.2, 0.3, 0.05, 0.0, 0.0, 0.0, 0.0))
    cams = (_lib.DepthCamera * 2)()
    for c in cams:
        c.depth, c.width, c.height = C.addressof(b["depth"]), 8, 8
        c.fx, c.fy, c.cx, c.cy = 4.0, 4.0, 3.5, 3.5
        c.cam_from_world[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1]
        c.world_from_cam[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1]
        c.min_depth, c.max_depth = 0.1, 5.0
    b["cams"] = cams
    kw = dict(cams=C.cast(cams, C.c_void_p), n_cams=2, spheres=C.cast(b["spheres"], C.c_void_p), n_spheres=2, tsdf=C.addressof(b["tsdf"]),
              weight=C.addressof(b["weight"]), occ=C.addressof(b["occ"]), n=(4, 3, 2), origin=(0.0, 0.0, 0.0), cell=0.1, trunc=0.2, max_weight=20.0)
    return kw, b


def _call(lib, kw):
    n = None if kw["n"] is None else C.byref((C.c_int * 3)(*kw["n"]))
    o = None if kw["origin"] is None else C.byref((C.c_float * 3)(*kw["origin"]))
    rc = lib.mpdx_tsdf_integrate(kw["cams"], kw["n_cams"], kw["spheres"], kw["n_spheres"], kw["tsdf"], kw["weight"], kw["occ"], n, o, kw["cell"],
                                 kw["trunc"], kw["max_weight"], None)
    return rc, lib.mpdx_last_error().decode()


def _cam(k, **v):
    def f(kw, b):
        for name, val in v.items():
            if name in ("cam_from_world", "world_from_cam"):
                getattr(b["cams"][k], name)[val[0]] = val[1]
            else:
                setattr(b["cams"][k], name, val)
    return f


def _set(**v):
    def f(kw, b):
        kw.update(v)
    return f


def _misalign(name, bytes_=2):
    def f(kw, b):
        if name == "depth":
            b["cams"][1].depth = C.addressof(b["depth"]) + bytes_
        else:
            kw[name] = kw[name] + bytes_
    return f


def _sphere(i, val):
    def f(kw, b):
        b["spheres"][i] = val
    return f


NAN, INF = float("nan"), float("inf")
REFUSALS = [
    ("2-D grid", _set(n=(4, 3, 1)), "n[2]"), ("n null", _set(n=None), "n"), ("one node along x", _set(n=(1, 3, 2)), "n[0]"),
    ("too many along y", _set(n=(4, 4097, 2)), "n[1]"), ("more than 2^29 nodes", _set(n=(4096, 4096, 33)), "nodes"),
    ("cams null", _set(cams=None), "cams"), ("no cameras", _set(n_cams=0), "n_cams"), ("nine cameras", _set(n_cams=9), "n_cams"),
    ("depth null", _cam(1, depth=None), "depth"), ("depth misaligned", _misalign("depth"), "depth"),
    ("width zero", _cam(0, width=0), "width"), ("width 8193", _cam(1, width=8193), "width"),
    ("height zero", _cam(0, height=0), "height"), ("height 8193", _cam(0, height=8193), "height"),
    ("fx zero", _cam(0, fx=0.0), "fx"), ("fx negative", _cam(1, fx=-4.0), "fx"), ("fx inf", _cam(0, fx=INF), "fx"), ("fy nan", _cam(0, fy=NAN), "fy"),
    ("cx nan", _cam(1, cx=NAN), "cx"), ("cy inf", _cam(0, cy=-INF), "cy"),
    ("cam_from_world nan", _cam(1, cam_from_world=(5, NAN)), "cam_from_world"), ("world_from_cam inf", _cam(0, world_from_cam=(11, INF)), "world_from_cam"),
    ("min_depth negative", _cam(0, min_depth=-0.1), "min_depth"), ("max_depth equal", _cam(1, max_depth=0.1), "max_depth"),
    ("max_depth below", _cam(0, max_depth=0.05), "max_depth"), ("max_depth inf", _cam(0, max_depth=INF), "max_depth"), ("min_depth nan", _cam(1, min_depth=NAN), "min_depth"),
    ("n_spheres negative", _set(n_spheres=-1), "n_spheres"), ("65 spheres", _set(n_spheres=65), "n_spheres"),
    ("spheres null", _set(spheres=None), "spheres"), ("sphere nan", _sphere(5, NAN), "spheres[1]"), ("sphere inf", _sphere(0, INF), "spheres[0]"),
    ("radius negative", _sphere(3, -0.01), "radius"),
    ("cell zero", _set(cell=0.0), "cell"), ("cell nan", _set(cell=NAN), "cell"), ("origin nan", _set(origin=(0.0, NAN, 0.0)), "origin"),
    ("origin null", _set(origin=None), "origin"),
    ("trunc zero", _set(trunc=0.0), "trunc"), ("trunc negative", _set(trunc=-0.1), "trunc"), ("trunc inf", _set(trunc=INF), "trunc"),
    ("trunc nan", _set(trunc=NAN), "trunc"), ("max_weight below 1", _set(max_weight=0.5), "max_weight"),
    ("max_weight 2^25", _set(max_weight=float(1 << 25)), "max_weight"), ("max_weight nan", _set(max_weight=NAN), "max_weight"),
    ("tsdf null", _set(tsdf=None), "tsdf"), ("weight null", _set(weight=None), "weight"), ("occ null", _set(occ=None), "occ"),
    ("tsdf misaligned", _misalign("tsdf"), "tsdf"), ("weight misaligned", _misalign("weight", 1), "weight"),
]


@pytest.mark.parametrize("what,change,needle", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_entry_point_refuses_on_the_host_without_launching(lib, what, change, needle):
    kw, b = _valid_args()
    for k in ("tsdf", "weight", "occ"):
        C.memset(b[k], 0x5A, C.sizeof(b[k]))
    change(kw, b)
    before = {k: bytes(b[k]) for k in ("tsdf", "weight", "occ")}
    rc, msg = _call(lib, kw)
    assert rc == -1 and needle in msg, (what, rc, msg)
    assert {k: bytes(b[k]) for k in before} == before, what       # nothing ran


def test_zero_spheres_take_a_null_array_as_far_as_the_host_checks_go(lib):
    """n_spheres = 0 with spheres null is valid: the NEXT refusal in line answers"""
    kw, b = _valid_args()
    kw.update(spheres=None, n_spheres=0, trunc=0.0)
    rc, msg = _call(lib, kw)
    assert rc == -1 and "trunc" in msg


# ---------------------------------------------------------------------------------------------------------------- Python surface
def _good():
    d = np.full((40, 48), 1.5, np.float32)
    return d, (40.0, 40.0, 23.5, 19.5), R.look_at((1.5, 0.5, 1.0), (0.0, 0.0, 0.0))


def test_python_refusals_before_any_device():
    from mpd_public_amd.planning import GridSDF, RobotPanda
    d, K, M = _good()
    ws = dict(ws_min=[-0.5, -0.5, -0.5], ws_max=[0.5, 0.5, 0.5], cell_size=0.1, device="cpu")
    # a valid call goes through every check and stops at the device (no CPU fallback)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GridSDF.from_depth(d, K, M, **ws)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GridSDF.from_depth([d, d[:20, :30]], [K, K], [M, M[:3]], **ws)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GridSDF.from_depth((d * 1000).astype(np.uint16), K, M, depth_scale=0.001, robot=RobotPanda(), q=np.zeros((5, 7)), **ws)
    bad = [
        (dict(depth=d[None, None]), "depth"), (dict(depth=d[:, :0]), "depth"), (dict(depth=np.zeros((10, 9000), np.float32)), "depth"),
        (dict(depth=d.astype(np.int32)), "uint16"), (dict(depth=d > 0), "uint16"), (dict(depth=[]), "no frames"),
        (dict(intrinsics=(40.0, 40.0, 23.5)), "intrinsics"), (dict(intrinsics=(0.0, 40.0, 23.5, 19.5)), "fx"),
        (dict(intrinsics=(40.0, np.nan, 23.5, 19.5)), "fx"), (dict(intrinsics=(40.0, 40.0, np.inf, 19.5)), "intrinsics"),
        (dict(world_from_cam=M[:2]), "world_from_cam"), (dict(world_from_cam=np.eye(3)), "world_from_cam"),
        (dict(depth=[d, d], intrinsics=[K, K], world_from_cam=M), "world_from_cam"), (dict(depth=[d, d], intrinsics=K, world_from_cam=[M, M]), "intrinsics"),
    ]
    skew = M.copy()
    skew[:3, :3] *= 1.001
    bad.append((dict(world_from_cam=skew), "orthonormal"))
    shear = M.copy()
    shear[0, 1] += 2e-4
    bad.append((dict(world_from_cam=shear), "orthonormal"))
    for v in (np.nan, np.inf):
        nf = M.copy()
        nf[1, 3] = v
        bad.append((dict(world_from_cam=nf), "finite"))
    row = M.copy()
    row[3, 0] = 0.1
    bad.append((dict(world_from_cam=row), "last row"))
    for change, needle in bad:
        args = dict(depth=d, intrinsics=K, world_from_cam=M)
        args.update(change)
        with pytest.raises(ValueError, match=needle):
            GridSDF.from_depth(args["depth"], args["intrinsics"], args["world_from_cam"], **ws)
    for kw, needle in [(dict(ws_min=[-0.5, -0.5], ws_max=[0.5, 0.5]), "3-D only"), (dict(trunc=0.0), "trunc"), (dict(trunc=np.nan), "trunc"),
                       (dict(max_weight=0.5), "max_weight"), (dict(max_weight=2.0 ** 25), "max_weight"), (dict(depth_range=(0.5, 0.5)), "depth_range"),
                       (dict(depth_range=(-0.1, 2.0)), "depth_range"), (dict(depth_scale=0.0), "depth_scale"), (dict(robot_padding=-0.01), "robot_padding"),
                       (dict(robot=RobotPanda(), q=np.zeros((6, 7))), "64"), (dict(robot=RobotPanda()), "q"), (dict(q=np.zeros(7)), "robot"),
                       (dict(robot=RobotPanda(), q=np.zeros(6)), "q"), (dict(robot=RobotPanda(), q=np.full(7, np.nan)), "finite")]:
        args = dict(ws)
        args.update(kw)
        with pytest.raises(ValueError, match=needle):
            GridSDF.from_depth(d, K, M, **args)
    # a grid that was not made from depth frames has nothing to integrate into
    plain = GridSDF(torch.zeros(4, 5, 6), [0.0, 0.0, 0.0], 0.1)
    with pytest.raises(ValueError, match="from_depth"):
        plain.integrate_depth(d, K, M)
    assert plain.tsdf() is None


def test_exports():
    import mpd_public_amd as m
    from mpd_public_amd import planning
    assert "robot_link_spheres" in m.__all__ and m.robot_link_spheres is planning.robot_link_spheres
    assert callable(m.GridSDF.from_depth) and callable(m.GridSDF.integrate_depth)


# ---------------------------------------------------------------------------------------------------------------- robot spheres
def test_panda_spheres_equal_the_oracle():
    from oracle import costs as oc
    from mpd_public_amd.planning import RobotPanda, robot_link_spheres
    rng = np.random.default_rng(11)
    q = rng.uniform(-2.5, 2.5, (64, 7))
    sp = robot_link_spheres(RobotPanda(), q)
    o = oc.RobotPanda()
    want = o.link_points(torch.from_numpy(q)).numpy()                     # [64, 11, 3] in float64
    assert sp.dtype == np.float64 and sp.shape == (64 * 11, 4)
    err = np.abs(sp[:, :3].reshape(64, 11, 3) - want).max()
    print(f"max |centre - oracle| = {err:.3e}")
    assert err <= 1e-12
    assert torch.equal(torch.from_numpy(sp[:11, 3]).float(), o.radii)      # the oracle keeps its radii in fp32
    assert np.array_equal(robot_link_spheres(RobotPanda(), q[3]), sp[33:44])


def test_chain_and_point_mass_spheres():
    from mpd_public_amd.planning import RobotChain, RobotPointMass, robot_link_spheres
    joints = [(np.eye(3), np.array([0.0, 0.0, 0.2]), "revolute"),
              (np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]), np.array([0.1, 0.0, 0.3]), "revolute"),
              (np.eye(3), np.array([0.0, 0.4, 0.0]), "prismatic")]
    spheres = [(0, (0.0, 0.0, 0.05), 0.08), (1, (0.05, 0.0, 0.1), 0.06), (2, (0.0, 0.2, 0.0), 0.05), (3, (0.01, 0.02, 0.03), 0.04)]
    ch = RobotChain(joints, spheres)
    q = np.random.default_rng(2).uniform(-1, 1, (5, 3))
    sp = robot_link_spheres(ch, q).reshape(5, 4, 4)
    for k, (fr, off, rad) in enumerate(spheres):
        assert np.array_equal(sp[:, k, :3], ch.fk(q, frame=fr, offset=off)[0]) and (sp[:, k, 3] == rad).all()
    pm = RobotPointMass(3, link_margin=0.03)
    assert robot_link_spheres(pm, [0.1, -0.2, 0.3]).tolist() == [[0.1, -0.2, 0.3, 0.03]]
    assert robot_link_spheres(pm, torch.zeros(2, 3)).shape == (2, 4)
    with pytest.raises(ValueError, match="2-D point mass"):
        robot_link_spheres(RobotPointMass(2), [0.0, 0.0])
    with pytest.raises(ValueError, match="q is"):
        robot_link_spheres(pm, np.zeros((2, 2, 3)))


def test_command_line_depth_archive_refusals(tmp_path):
    from mpd_public_amd.inference import _depth_grid_args
    d, K, M = _good()
    path = tmp_path / "scan.npz"
    np.savez(path, depth=d[None], intrinsics=np.array([K]))
    base = dict(model_id="EnvSpheres3D-RobotPanda", sdf_grid_mode="linear")
    assert _depth_grid_args(dict(base, sdf_grid_depth=None, sdf_grid_cell_size=None)) == dict(base, sdf_grid_cell_size=None)
    with pytest.raises(SystemExit, match="needs --sdf_grid_cell_size"):
        _depth_grid_args(dict(base, sdf_grid_depth=str(path), sdf_grid_cell_size=None))
    with pytest.raises(SystemExit, match="exclude"):
        _depth_grid_args(dict(base, sdf_grid_depth=str(path), sdf_grid_cell_size=None, sdf_grid=object()))
    with pytest.raises(SystemExit, match="world_from_cam"):
        _depth_grid_args(dict(base, sdf_grid_depth=str(path), sdf_grid_cell_size=0.05))
