"""GPU tests of the depth-camera fusion (csrc/tsdf.hpp: mpdx_tsdf_integrate) and of what is built on it (GridSDF.from_depth / integrate_depth,
refresh_grids, a plan on a fused grid).

The tsdf, weight and occupancy planes are compared BIT FOR BIT with tests/tsdf_ref.py (numpy fp32, one rounded operation per step in the kernel's
order); the transform that follows is the one tests/test_gpu_occupancy.py holds to tests/edt_ref.py, so it is compared with from_occupancy of the
reference occupancy.  No tolerance anywhere: the arithmetic is stated, not approximated."""
import ctypes as C
from math import ceil

import numpy as np
import pytest
import torch

import tsdf_ref as R
from helpers import synth_sd, t, product_guide, obstacle_hugging_trajs, DIM_MULTS
from test_gpu_grid_sdf import TA

pytestmark = pytest.mark.gpu

PANDA_Q = np.array([0.3, -0.4, 0.1, -2.0, 0.0, 1.9, 0.7])


def _frame(spheres, boxes, K, wh, eye, target=(0.0, 0.0, -0.1), depth_range=(0.1, 5.0)):
    M = R.look_at(eye, target)
    return R.camera(R.render(spheres, boxes, K, M, *wh), K, M, depth_range), M


def _frames(box):
    """the two cameras of the tests on the scene with `box` ([1, 6]) and the floor"""
    boxes = np.concatenate([box, R.FLOOR])
    c1, _ = _frame(R.SPHERES, boxes, R.K1, R.WH1, R.EYE1)
    c2, _ = _frame(R.SPHERES, boxes, R.K2, R.WH2, R.EYE2)
    return [c1, c2]


def _device_call(cams, planes, shape, origin, cell, trunc, max_weight, spheres=None):
    """mpdx_tsdf_integrate on the planes (tsdf, weight, occ device tensors) -> rc; the depth images are uploaded here"""
    from mpd_public_amd import _lib
    imgs = [torch.from_numpy(c["depth"]).cuda() for c in cams]
    arr = (_lib.DepthCamera * len(cams))()
    for k, c in enumerate(cams):
        r = arr[k]
        r.depth, r.height, r.width = imgs[k].data_ptr(), c["depth"].shape[0], c["depth"].shape[1]
        r.fx, r.fy, r.cx, r.cy = float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])
        r.cam_from_world[:], r.world_from_cam[:] = c["A"].reshape(-1).tolist(), c["B"].reshape(-1).tolist()
        r.min_depth, r.max_depth = float(c["min_depth"]), float(c["max_depth"])
    sp = None if spheres is None else (C.c_float * (4 * len(spheres)))(*np.asarray(spheres, np.float32).reshape(-1).tolist())
    nz, ny, nx = shape
    tsdf, weight, occ = planes
    rc = _lib.load().mpdx_tsdf_integrate(arr, len(cams), sp, 0 if spheres is None else len(spheres), tsdf.data_ptr(), weight.data_ptr(), occ.data_ptr(),
                                         C.byref((C.c_int * 3)(nx, ny, nz)), C.byref((C.c_float * 3)(*origin)), cell, trunc, max_weight,
                                         _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def _planes(shape):
    n = int(np.prod(shape))
    return torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.full((n,), 7, dtype=torch.uint8, device="cuda")


def _assert_equal(planes, want, what):
    for name, got, w in zip(("tsdf", "weight", "occ"), planes, want):
        w = torch.from_numpy(np.ascontiguousarray(w).reshape(-1)).cuda()
        assert got.dtype == w.dtype and torch.equal(got, w), f"{what}: {name} differs at {int((got != w).sum())} of {w.numel()} nodes"


# ------------------------------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("trunc_cells,max_weight", [(2.0, 2.0), (2.0, 20.0), (0.5, 2.0), (0.5, 20.0)])
def test_integration_bit_for_bit_over_three_calls(trunc_cells, max_weight):
    shape, origin, cell = R.SHAPE, R.ORIGIN, R.CELL
    trunc = trunc_cells * cell
    moved = R.BOX + np.array([[0.25, -0.3, 0.05, 0, 0, 0]])
    calls = [_frames(R.BOX), _frames(moved), _frames(moved)[1:]]
    planes = _planes(shape)
    T, W = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    seen = []
    for k, cams in enumerate(calls):
        assert _device_call(cams, planes, shape, origin, cell, trunc, max_weight) == 0
        T, W, occ = R.integrate_ref(T, W, cams, shape, origin, cell, trunc, max_weight)
        _assert_equal(planes, (T, W, occ), f"call {k}")
        seen.append((int((W > 0).sum()), int(occ.sum())))
    print("observed / occupied nodes after each call:", seen)
    assert all(0 < o < s < W.size for s, o in seen)                       # the case is not empty: some nodes seen, some occupied, some not seen
    if max_weight == 2.0:
        assert W.max() == 2.0                                              # the cap was reached


# ------------------------------------------------------------------------------------------------------------------------ 2. edges
def test_rejected_pixels_partial_frustum_and_out_of_image_projections():
    shape, origin, cell, trunc, max_weight = R.SHAPE, R.ORIGIN, R.CELL, 2 * R.CELL, 20.0
    boxes = np.concatenate([R.BOX, R.FLOOR])
    cam, _ = _frame(R.SPHERES, boxes, R.K1, R.WH1, R.EYE1, depth_range=(0.3, 3.0))
    d = cam["depth"].copy()
    rows = np.arange(d.shape[0])[:, None] + np.arange(d.shape[1])[None]
    for k, v in enumerate([0.0, np.nan, np.inf, -1.0, 0.2, 3.5]):          # zero, NaN, +inf, negative, below min_depth, above max_depth
        d[rows % 9 == k] = v
    d[0, 0], d[-1, -1] = 0.3, 3.0                                          # the bounds themselves are measurements
    cam["depth"] = d
    # a camera inside the grid box looking along +x with a narrow field: nodes behind it, nodes outside the image
    M = R.look_at((-0.2, 0.05, 0.0), (1.0, 0.1, -0.05))
    K = (60.0, 60.0, 12.3, 9.7)
    inner = R.camera(R.render(R.SPHERES, boxes, K, M, 25, 19), K, M)
    p = R.node_positions(shape, origin, cell)
    _, _, _, st = R.observe_ref(inner, p, trunc=trunc)
    _, _, _, st1 = R.observe_ref(cam, p, trunc=trunc)
    counts = {s: int((st == s).sum()) for s in range(6)}
    print("inner camera stages (behind, outside, no measurement, masked, occluded, observed):", counts, "; rejected-pixel camera:",
          {s: int((st1 == s).sum()) for s in range(6)})
    assert counts[0] > 0 and counts[1] > 0 and counts[5] > 0 and counts[4] > 0
    assert int((st1 == 2).sum()) > 0 and int((st1 == 5).sum()) > 0
    planes = _planes(shape)
    T, W = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    for cams in ([cam], [inner], [cam, inner]):
        assert _device_call(cams, planes, shape, origin, cell, trunc, max_weight) == 0
        T, W, occ = R.integrate_ref(T, W, cams, shape, origin, cell, trunc, max_weight)
        _assert_equal(planes, (T, W, occ), f"{len(cams)} camera(s)")


def test_half_pixel_ties_round_half_to_even():
    """A camera aligned with the grid axes (looking along +z), dyadic cell, origin and eye, fx = fy = 16, cx = cy = 15.5: on the node planes one and
    two metres in front of it, x0 / x2 is an exact multiple of 1 / 16 or 1 / 32, so u = fx * (x0 / x2) + cx lands exactly on k + 0.5"""
    shape, origin, cell = (33, 33, 33), (-1.0, -1.0, -1.0), 0.0625
    M = np.eye(4)
    M[:3, 3] = (0.0, 0.0, -2.0)
    K = (16.0, 16.0, 15.5, 15.5)
    scene = np.array([[0.1, -0.2, 0.3, 0.45], [-0.5, 0.4, -0.2, 0.3]])
    cam = R.camera(R.render(scene, R.FLOOR[:0], K, M, 32, 32), K, M)
    p = R.node_positions(shape, origin, cell)
    with np.errstate(all="ignore"):
        x0 = ((cam["A"][0, 0] * p[0] + cam["A"][0, 1] * p[1]) + cam["A"][0, 2] * p[2]) + cam["A"][0, 3]
        x2 = ((cam["A"][2, 0] * p[0] + cam["A"][2, 1] * p[1]) + cam["A"][2, 2] * p[2]) + cam["A"][2, 3]
        u = cam["fx"] * (x0 / x2) + cam["cx"]
    ok, _, _, _ = R.observe_ref(cam, p, trunc=2 * cell)
    ties = (x2 > 0) & (u - np.floor(u) == np.float32(0.5)) & (u > 0) & (u < 31)
    print(f"nodes projecting exactly half-way between two pixel centres: {int(ties.sum())}; of them observed: {int((ties & ok).sum())}")
    assert (ties & ok).sum() > 0
    planes = _planes(shape)
    for trunc in (2 * cell, 0.5 * cell):
        T, W, occ = R.integrate_ref(planes[0].cpu().numpy().reshape(shape), planes[1].cpu().numpy().reshape(shape), [cam], shape, origin, cell, trunc, 5.0)
        assert _device_call([cam], planes, shape, origin, cell, trunc, 5.0) == 0
        _assert_equal(planes, (T, W, occ), f"trunc {trunc}")
        assert occ.any()


# ------------------------------------------------------------------------------------------------------------------------ 3. robot mask
def test_robot_mask_bit_for_bit_and_it_matters():
    import mpd_public_amd as m
    robot, pad = m.make_robot("RobotPanda"), 0.02
    links = m.robot_link_spheres(robot, PANDA_Q)
    ws_min, ws_max, cell = np.array([-0.6, -0.6, -0.1]), np.array([0.6, 0.6, 1.1]), 0.05
    scene = np.array([[-0.45, -0.45, 0.2, 0.15]])
    floor = np.array([[0.0, 0.0, -0.3, 4.0, 4.0, 0.05]])
    K, M = (40.0, 40.0, 23.6, 19.4), R.look_at((1.8, 0.5, 0.9), (0.0, 0.0, 0.45))
    depth = R.render(np.concatenate([scene, links]), floor, K, M, 48, 40)
    kw = dict(padding=0.0, trunc=2 * cell, max_weight=20.0, depth_range=(0.1, 5.0))
    g = m.GridSDF.from_depth(depth, K, M, ws_min, ws_max, cell, robot=robot, q=PANDA_Q, robot_padding=pad, **kw)
    bare = m.GridSDF.from_depth(depth, K, M, ws_min, ws_max, cell, **kw)
    shape = tuple(reversed(g.shape))
    cam = R.camera(depth, K, M)
    sp = links.copy()
    sp[:, 3] += pad
    sp = sp.astype(np.float32)
    z = np.zeros(shape, np.float32)
    want = R.integrate_ref(z, z, [cam], shape, g.origin, cell, 2 * cell, 20.0, spheres=sp)
    _assert_equal((*[v.reshape(-1) for v in g.tsdf()], g.occupancy().reshape(-1)), want, "masked")
    want_bare = R.integrate_ref(z, z, [cam], shape, g.origin, cell, 2 * cell, 20.0)
    _assert_equal((*[v.reshape(-1) for v in bare.tsdf()], bare.occupancy().reshape(-1)), want_bare, "unmasked")
    xyz = R.nodes_xyz(shape, g.origin, cell)
    inside = np.zeros(shape, bool)
    for c in sp.astype(np.float64):
        inside |= np.linalg.norm(xyz - c[:3], axis=-1) < c[3]
    occ, occ_bare = g.occupancy().cpu().numpy() != 0, bare.occupancy().cpu().numpy() != 0
    print(f"nodes inside padded link spheres: {int(inside.sum())}; occupied with the mask {int((occ & inside).sum())}, without {int((occ_bare & inside).sum())}")
    assert not (occ & inside).any()
    assert (occ_bare & inside).any()
    assert occ.any()                                                       # the scene itself is still there


# ------------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_on_device_buffers_launch_nothing():
    from mpd_public_amd import _lib
    shape, origin, cell = R.SHAPE, R.ORIGIN, R.CELL
    cams = _frames(R.BOX)
    n = int(np.prod(shape))
    planes = (torch.full((n,), -3.5, device="cuda"), torch.full((n,), 9.0, device="cuda"), torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda"))
    keep = [p.clone() for p in planes]
    bad_nan = [dict(c) for c in cams]
    bad_nan[1]["A"] = bad_nan[1]["A"].copy()
    bad_nan[1]["A"][0, 3] = np.nan
    bad_depth = [dict(c) for c in cams]
    bad_depth[0]["max_depth"] = bad_depth[0]["min_depth"]
    for what, args, needle in [("trunc zero", (cams, planes, shape, origin, cell, 0.0, 20.0), "trunc"),
                               ("max_weight 0.5", (cams, planes, shape, origin, cell, 0.1, 0.5), "max_weight"),
                               ("non-finite pose", (bad_nan, planes, shape, origin, cell, 0.1, 20.0), "cam_from_world"),
                               ("depth bounds", (bad_depth, planes, shape, origin, cell, 0.1, 20.0), "depth"),
                               ("2-D grid", (cams, planes, (1,) + shape[1:], origin, cell, 0.1, 20.0), "n[2]"),
                               ("sphere radius", (cams, planes, shape, origin, cell, 0.1, 20.0, [[0.0, 0.0, 0.0, -1.0]]), "radius"),
                               ("nine cameras", (cams * 4 + cams[:1], planes, shape, origin, cell, 0.1, 20.0), "n_cams")]:
        assert _device_call(*args) == -1, what
        assert needle in _lib.load().mpdx_last_error().decode(), what
    for p, k in zip(planes, keep):
        assert torch.equal(p, k)


# ------------------------------------------------------------------------------------------------------------------------ 5. identities
def _panda_frames(n_cams=4, wh=(64, 48), shift=(0.0, 0.0, 0.0)):
    """the fixed spheres of EnvSpheres3D (shifted by `shift`) and a floor, from n_cams cameras around the Panda's workspace"""
    import mpd_public_amd as m
    env = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args=TA).env
    o = env.obj_fixed
    spheres = np.concatenate([np.asarray(o.sphere_centers, np.float64) + np.asarray(shift), np.asarray(o.sphere_radii, np.float64)[:, None]], 1)
    floor = np.array([[0.0, 0.0, -0.45, 5.0, 5.0, 0.05]])
    K = (48.0, 48.0, (wh[0] - 1) / 2 + 0.13, (wh[1] - 1) / 2 - 0.21)
    out = []
    for k in range(n_cams):
        a = 2 * np.pi * (k + 0.3) / n_cams
        M = R.look_at((2.6 * np.cos(a), 2.6 * np.sin(a), 1.9), (0.0, -0.2, 0.5))
        out.append((R.render(spheres, floor, K, M, *wh), K, M))
    return out


def _from_frames(frames, ws_min, ws_max, cell, **kw):
    import mpd_public_amd as m
    return m.GridSDF.from_depth([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], ws_min, ws_max, cell, **kw)


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_from_depth_equals_from_occupancy_of_the_reference(mode):
    import mpd_public_amd as m
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args=TA)
    frames = _panda_frames()
    cell, inflate = 0.05, 0.01
    g = _from_frames(frames, ds.task.ws_min, ds.task.ws_max, cell, mode=mode, inflate=inflate)
    shape = tuple(reversed(g.shape))
    z = np.zeros(shape, np.float32)
    T, W, occ = R.integrate_ref(z, z, [R.camera(*f) for f in frames], shape, g.origin, cell, 3 * cell, 20.0)
    _assert_equal((*[v.reshape(-1) for v in g.tsdf()], g.occupancy().reshape(-1)), (T, W, occ), "from_depth")
    ref = m.GridSDF.from_occupancy(occ, g.origin, cell, mode=mode, inflate=inflate)
    for a, b in zip(g.node_values(), ref.node_values()):
        assert (a is None and b is None) or torch.equal(a, b)
    assert occ.any() and (W == 0).any()
    # more frames go into the same planes
    ptrs = [p.data_ptr() for p in g.planes("cuda") if p is not None] + [p.data_ptr() for p in g.tsdf()] + [g.occupancy().data_ptr()]
    more = _panda_frames(2, (40, 30), shift=(0.0, 0.1, 0.0))
    assert g.integrate_depth([f[0] for f in more], [f[1] for f in more], [f[2] for f in more]) is g
    assert [p.data_ptr() for p in g.planes("cuda") if p is not None] + [p.data_ptr() for p in g.tsdf()] + [g.occupancy().data_ptr()] == ptrs
    T2, W2, occ2 = R.integrate_ref(T, W, [R.camera(*f) for f in more], shape, g.origin, cell, 3 * cell, 20.0)
    _assert_equal((*[v.reshape(-1) for v in g.tsdf()], g.occupancy().reshape(-1)), (T2, W2, occ2), "integrate_depth")
    assert not np.array_equal(occ2, occ)
    ref2 = m.GridSDF.from_occupancy(occ2, g.origin, cell, mode=mode, inflate=inflate)
    for a, b in zip(g.node_values(), ref2.node_values()):
        assert (a is None and b is None) or torch.equal(a, b)
    # reset starts from an empty map
    g.integrate_depth([f[0] for f in more], [f[1] for f in more], [f[2] for f in more], reset=True)
    _assert_equal((*[v.reshape(-1) for v in g.tsdf()], g.occupancy().reshape(-1)),
                  R.integrate_ref(z, z, [R.camera(*f) for f in more], shape, g.origin, cell, 3 * cell, 20.0), "reset")


def test_integrate_depth_then_refresh_equals_a_fresh_guide():
    import mpd_public_amd as m
    env_id, robot_id, cell = "EnvSpheres3D", "RobotPanda", 0.05
    ds_prim = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
    frames = _panda_frames()
    grid = _from_frames(frames, ds_prim.task.ws_min, ds_prim.task.ws_max, cell, inflate=0.01)
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA, sdf_grid=grid)
    x = obstacle_hugging_trajs(ds_prim, 7, seed=f"g/{env_id}", scale=0.9).cuda()
    pg = product_guide(ds).cuda()
    first = pg(x)
    xu = ds.unnormalize_trajectories(x)
    m_first = ds.task.trajectory_metrics(xu)
    moved = _panda_frames(shift=(0.12, -0.1, 0.05))
    assert grid.integrate_depth([f[0] for f in moved], [f[1] for f in moved], [f[2] for f in moved], reset=True) is grid
    pg.refresh_grids()
    ds.task.refresh_grids()
    second = pg(x)
    fresh_grid = _from_frames(moved, ds_prim.task.ws_min, ds_prim.task.ws_max, cell, inflate=0.01)
    ds2 = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA, sdf_grid=fresh_grid)
    want = product_guide(ds2).cuda()(x)
    assert torch.equal(second, want) and not torch.equal(second, first) and float(second.abs().max()) > 0
    assert torch.equal(ds.task.trajectory_metrics(xu), ds2.task.trajectory_metrics(xu))
    assert not torch.equal(ds.task.trajectory_metrics(xu), m_first)


# ------------------------------------------------------------------------------------------------------------------------ 6. end to end
def test_plan_on_a_fused_depth_grid_fused_equals_stepwise():
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    env_id, robot_id, opt, T, B, n0 = "EnvSpheres3D", "RobotPanda", 0, 25, 4, 5
    ds0 = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
    grid = _from_frames(_panda_frames(), ds0.task.ws_min, ds0.task.ws_max, 0.05)
    task = m.PlanningTask(ds0.env, ds0.robot, obstacle_cutoff_margin=ds0.task.obstacle_cutoff_margin, tensor_args=TA, sdf_grid=grid)
    assert task.df_collision_objects.kind == _lib.FIELD_GRID
    ds0.task = task
    D = ds0.state_dim
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
    noise = t(f"guided_noise/{env_id}", (T + n0 + 1, B, 64, D))
    start = ds0.normalizer.normalize(torch.cat([t(f"gs/{env_id}", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    goal = ds0.normalizer.normalize(torch.cat([t(f"gg/{env_id}", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    hc = {0: start, 63: goal}
    pg = product_guide(ds0, 1e-2, 1e-7).cuda()
    kw = dict(n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, n_guide_steps=5, t_start_guide=ceil(0.25 * T),
              n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise.cuda())
    a = dm.run_inference(None, hc, fused=True, guide=pg, **kw)
    b = dm.run_inference(None, hc, fused=False, guide=pg, **kw)
    assert torch.equal(a, b)
    unguided = dm.run_inference(None, hc, fused=True, guide=None, **kw)
    assert float((a[-1] - unguided[-1]).abs().max()) > 1e-3, "guidance must matter in this test"


def test_command_line_archive_gives_the_same_grid(tmp_path):
    import mpd_public_amd as m
    from mpd_public_amd.inference import _depth_grid_args
    frames = _panda_frames(2, (40, 30))
    path = tmp_path / "scan.npz"
    np.savez(path, depth=np.stack([f[0] for f in frames]), intrinsics=np.array([f[1] for f in frames]), world_from_cam=np.stack([f[2] for f in frames]))
    a = _depth_grid_args(dict(model_id="EnvSpheres3D-RobotPanda", sdf_grid_depth=str(path), sdf_grid_cell_size=0.05, sdf_grid_mode="nearest"))
    assert a["sdf_grid_cell_size"] is None and "sdf_grid_depth" not in a
    ws_min, ws_max = m.make_env("EnvSpheres3D").limits
    want = _from_frames(frames, ws_min, ws_max, 0.05, mode="nearest")
    for x, y in zip(a["sdf_grid"].node_values(), want.node_values()):
        assert torch.equal(x, y)
    assert a["sdf_grid"].occupancy().any()
