"""GPU tests of the occupancy transform (csrc/edt.hpp: mpdx_sdf_grid_from_occupancy, mpdx_occupancy_from_points) and of what is built on it
(GridSDF.from_occupancy / from_points / update_occupancy, refresh_grids, PlanningTask(sdf_grid=<GridSDF>), experiment(sdf_grid=...)).

The transform and the voxelisation are compared BIT FOR BIT with tests/edt_ref.py (brute force over all node pairs; fp32 steps rounded one by one):
the arithmetic is exact by construction, so there is no tolerance.  The field under the guide and the metrics is held to the fp64 grid oracle
(tests/grid_ref.py) fed the node values downloaded from the device, with exactly the bound and the ambiguity classification of
tests/test_gpu_grid_sdf.py (imported from there)."""
import ctypes as C
from math import ceil

import numpy as np
import pytest
import torch

import edt_ref
from helpers import synth_sd, t, product_guide, obstacle_hugging_trajs, DIM_MULTS
from test_gpu_grid_sdf import CAP, CELL, TA, _classify, _oracle_with_grid, _to_supports

pytestmark = pytest.mark.gpu

CELL_T, INFLATES = 0.02, (0.0, 0.03)


def _n3(shape_xyz):
    return (C.c_int * 3)(*shape_xyz)


def _run_transform(occ, cell, inflate, with_grad=True):
    """mpdx_sdf_grid_from_occupancy on occ [nz, ny, nx] -> (d2, sdf, grad) as numpy; every output starts as a sentinel"""
    from mpd_public_amd import _lib
    lib = _lib.load()
    nz, ny, nx = occ.shape
    nodes = occ.size
    o = torch.from_numpy(np.array(occ, dtype=np.uint8)).cuda()
    sdf = torch.full((nodes,), float("nan"), device="cuda")
    grad = torch.full((nodes, 4), float("nan"), device="cuda") if with_grad else None
    d2 = torch.full((nodes,), -7, dtype=torch.int32, device="cuda")
    n = _n3((nx, ny, nz))
    ws_bytes = lib.mpdx_sdf_grid_edt_ws_bytes(C.byref(n))
    assert ws_bytes == 8 * nodes
    ws = torch.full((ws_bytes // 4 + 16,), -1, dtype=torch.int32, device="cuda")     # (+16: a guard the transform must leave alone)
    _lib.check(lib.mpdx_sdf_grid_from_occupancy(o.data_ptr(), sdf.data_ptr(), None if grad is None else grad.data_ptr(), d2.data_ptr(), C.byref(n), cell,
                                                inflate, ws.data_ptr(), ws_bytes, _lib.current_stream()), "mpdx_sdf_grid_from_occupancy")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes // 4:] == -1).all())
    shp = occ.shape
    return d2.cpu().numpy().reshape(shp), sdf.cpu().numpy().reshape(shp), (None if grad is None else grad.cpu().numpy().reshape(shp + (4,)))


# ------------------------------------------------------------------------------------------------------------------------ 1. transform
@pytest.mark.parametrize("name", edt_ref.PATTERNS)
@pytest.mark.parametrize("shape", edt_ref.SHAPES, ids=["x".join(str(v) for v in s) for s in edt_ref.SHAPES])
def test_transform_bit_for_bit(shape, name):
    occ, d2_want = edt_ref.case(shape, name)
    if name == "all_free" or name == "all_occupied":
        assert (d2_want == sum(shape) ** 2).all()                                  # the sentinel
    for inflate in INFLATES:
        d2, sdf, grad = _run_transform(occ, CELL_T, inflate)
        assert np.array_equal(d2, d2_want), f"d2 differs at {int((d2 != d2_want).sum())} of {d2.size} nodes"
        s_want = edt_ref.sdf_ref(d2_want, occ, CELL_T, inflate)
        assert sdf.dtype == np.float32 and np.array_equal(sdf, s_want)
        assert np.array_equal(grad, edt_ref.grad_ref(s_want, CELL_T))
        if shape[2] == 1:
            assert not grad[..., 2:].any()
    # without the optional outputs the sdf plane is the same
    from mpd_public_amd import _lib
    lib = _lib.load()
    o = torch.from_numpy(np.array(occ, dtype=np.uint8)).cuda()
    sdf2 = torch.empty(occ.size, device="cuda")
    n = _n3(shape)
    ws = torch.empty(2 * occ.size, dtype=torch.int32, device="cuda")
    _lib.check(lib.mpdx_sdf_grid_from_occupancy(o.data_ptr(), sdf2.data_ptr(), None, None, C.byref(n), CELL_T, INFLATES[-1], ws.data_ptr(), 8 * occ.size,
                                                _lib.current_stream()))
    assert np.array_equal(sdf2.cpu().numpy().reshape(occ.shape), sdf)


def test_non_zero_bytes_are_occupied():
    occ, d2_want = edt_ref.case((17, 13, 9), "random3")
    d2, sdf, _ = _run_transform(occ * np.uint8(200), CELL_T, 0.0, with_grad=False)
    assert np.array_equal(d2, d2_want) and np.array_equal(sdf, edt_ref.sdf_ref(d2_want, occ, CELL_T))


# ------------------------------------------------------------------------------------------------------------------------ 2. voxelisation
def _cloud(shape_xyz, origin, cell, seed, n=500):
    """n points uniform in a box a little larger than the grid (some are dropped), then NaN / inf rows and points exactly half-way between nodes"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape_xyz
    lo = np.asarray(origin, np.float64) - 1.5 * cell
    hi = np.asarray(origin, np.float64) + (np.array([nx, ny, nz]) + 0.5) * cell
    p = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    o = np.asarray(origin, np.float32)
    c = np.float32(cell)
    mid = np.float32(o + np.array([1, 1, 1], np.float32) * c)                     # a node, finite everywhere: the rows below spoil one coordinate each
    bad = np.stack([mid] * 6)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, 1], bad[5, 2] = np.nan, np.nan, np.nan, np.inf, -np.inf, np.inf
    half = np.stack([o + np.array([0.5, 1.0, 1.0], np.float32) * c, o + np.array([1.5, 1.0, 1.0], np.float32) * c, o + np.array([1.0, 0.5, 1.0], np.float32) * c,
                     o + np.array([nx - 1.5, ny - 0.5, 1.0], np.float32) * c, o + np.array([-0.5, 1.0, 1.0], np.float32) * c]).astype(np.float32)
    return np.concatenate([p, bad, half]).astype(np.float32)


def _voxelise(points, occ_t, shape_xyz, origin, cell):
    from mpd_public_amd import _lib
    p = torch.from_numpy(points).cuda().contiguous()
    _lib.check(_lib.load().mpdx_occupancy_from_points(p.data_ptr(), p.shape[0], occ_t.data_ptr(), C.byref(_n3(shape_xyz)), C.byref((C.c_float * 3)(*origin)),
                                                      cell, _lib.current_stream()), "mpdx_occupancy_from_points")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,origin,cell", [((17, 13, 9), (-1.0, 0.5, 0.25), 0.25), ((17, 13, 9), (-0.37, 0.11, 0.05), 0.02),
                                               ((65, 33, 1), (-1.0, 0.5, 0.0), 0.125), ((65, 33, 1), (-0.37, 0.11, 0.0), 0.02)])
def test_voxelisation_bit_for_bit_and_two_clouds_give_the_union(shape, origin, cell):
    nx, ny, nz = shape
    rev = (nz, ny, nx)
    a, b = _cloud(shape, origin, cell, 1), _cloud(shape, origin, cell, 2)
    if cell in (0.25, 0.125):   # dyadic: the half-way rows ARE half-way in fp32 (elsewhere the reference's own rounding decides, the same way)
        u = (a[-5:, 0] - np.float32(origin[0])) * (np.float32(1) / np.float32(cell))
        assert u.tolist()[:2] == [0.5, 1.5] and u.tolist()[4] == -0.5
    want_a = edt_ref.voxelise_ref(a, rev, origin, cell)
    assert 0 < want_a.sum() < len(a) - 6                                          # some points land, some are dropped
    guard = 64
    buf = torch.zeros(nx * ny * nz + guard, dtype=torch.uint8, device="cuda")
    _voxelise(a, buf, shape, origin, cell)
    assert np.array_equal(buf[:-guard].cpu().numpy().reshape(rev), want_a) and not bool(buf[-guard:].any())
    want_ab = edt_ref.voxelise_ref(b, rev, origin, cell, occ=want_a)
    assert np.array_equal(want_ab, want_a | edt_ref.voxelise_ref(b, rev, origin, cell)) and want_ab.sum() > want_a.sum()
    _voxelise(b, buf, shape, origin, cell)
    assert np.array_equal(buf[:-guard].cpu().numpy().reshape(rev), want_ab) and not bool(buf[-guard:].any())
    # no points: nothing changes
    from mpd_public_amd import _lib
    assert _lib.load().mpdx_occupancy_from_points(None, 0, buf.data_ptr(), C.byref(_n3(shape)), C.byref((C.c_float * 3)(*origin)), cell, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(buf[:-guard].cpu().numpy().reshape(rev), want_ab)


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_from_points_voxelises_then_transforms(mode):
    from mpd_public_amd.planning import GridSDF, grid_spec_for
    ws_min, ws_max, cell, inflate = np.array([-1.0, -1.0]), np.array([1.0, 1.0]), 0.05, 0.04
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-1.5, 1.5, (300, 2)), np.zeros((300, 1))], 1).astype(np.float32)
    g = GridSDF.from_points(pts, ws_min, ws_max, cell, mode=mode, inflate=inflate)
    shape, origin = grid_spec_for(ws_min, ws_max, cell)
    assert g.shape == shape and g.dim == 2 and g.inflate == inflate
    rev = (1,) + tuple(reversed(shape))
    occ = edt_ref.voxelise_ref(pts, rev, list(origin) + [0.0], cell)
    assert np.array_equal(g.occupancy().cpu().numpy(), occ[0])
    sdf, grad = g.node_values()
    s_want = edt_ref.sdf_ref(edt_ref.d2_ref(occ), occ, cell, inflate)
    assert np.array_equal(sdf.cpu().numpy(), s_want[0])
    assert (grad is None) if mode == "linear" else np.array_equal(grad.cpu().numpy(), edt_ref.grad_ref(s_want, cell)[0])
    # update_occupancy(points=...) starts from an empty map and writes the planes the grid already holds
    ptr = g.planes("cuda")[0].data_ptr()
    more = rng.uniform(-1.0, 1.0, (50, 3)).astype(np.float32)
    g.update_occupancy(points=more)
    occ2 = edt_ref.voxelise_ref(more, rev, list(origin) + [0.0], cell)
    with pytest.raises(ValueError, match="points"):
        g.update_occupancy(points=more[:, :2])
    assert g.planes("cuda")[0].data_ptr() == ptr and np.array_equal(g.occupancy().cpu().numpy(), occ2[0])
    assert np.array_equal(g.node_values()[0].cpu().numpy(), edt_ref.sdf_ref(edt_ref.d2_ref(occ2), occ2, cell, inflate)[0])
    with pytest.raises(ValueError, match="shape"):
        g.update_occupancy(occ=np.zeros((4, 4), bool))


# ------------------------------------------------------------------------------------------------------------------------ 3. the field under the guide
FIELD_CASES = [("EnvSimple2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")]
# The inflate of the fields compared with the oracle.  A transformed grid holds few distinct values, cell * (sqrt(d2) - 0.5) - inflate; at inflate 0 and
# 2 cm cells the integer distances give 0.01, 0.03, ..., 0.11, ... - EXACTLY the Panda's hinge margins (link radii 0.06 ... 0.10, plus the 0.05
# cutoff), so in nearest mode whole regions of nodes sit at zero slack, which the classification rightly calls ambiguous (17 % of the waypoints, over
# the cap that is a condition of the comparison).  3 mm is off that lattice: over d2 < 3000 no node value comes within 1.3e-4 of a margin of either
# robot (EPS_SLACK is 1e-5), computed from the formula alone.
FIELD_INFLATE = 0.003
_OCC = {}


def _primitive_occupancy(env_id, robot_id):
    """(ds_prim, occ [nz, ny, nx] | [ny, nx] bool, origin, cell): occupied = the primitive sdf of the FIXED objects at the node <= 0, in numpy from the
    environment's tables, on the grid box of planning.grid_spec_for"""
    import mpd_public_amd as m
    from mpd_public_amd.planning import grid_spec_for
    if env_id not in _OCC:
        ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
        dim = ds.env.dim
        cell = CELL[dim]
        shape, origin = grid_spec_for(ds.task.ws_min, ds.task.ws_max, cell)
        ax = [origin[j].astype(np.float64) + np.arange(shape[j]) * cell for j in range(dim)]
        pos = np.stack(np.meshgrid(*reversed(ax), indexing="ij")[::-1], -1)           # [(nz,) ny, nx, dim], last axis (x, y, z)
        o = ds.env.obj_fixed
        sd = np.full(pos.shape[:-1], np.inf)
        for c, r in zip(o.sphere_centers, o.sphere_radii):
            sd = np.minimum(sd, np.linalg.norm(pos - c[:dim], axis=-1) - r)
        for c, h in zip(o.box_centers, o.box_half):
            d = np.abs(pos - c[:dim]) - h[:dim]
            sd = np.minimum(sd, np.minimum(d.max(-1), 0.0) + np.linalg.norm(np.maximum(d, 0.0), axis=-1))
        _OCC[env_id] = (ds, sd <= 0, origin, cell)
    return _OCC[env_id]


def _datasets(env_id, robot_id, mode, inflate=FIELD_INFLATE):
    import mpd_public_amd as m
    ds_prim, occ, origin, cell = _primitive_occupancy(env_id, robot_id)
    assert occ.any() and not occ.all()
    grid = m.GridSDF.from_occupancy(occ, origin, cell, mode=mode, inflate=inflate)
    return ds_prim, m.TrajectoryDataset(env_id, robot_id, tensor_args=TA, sdf_grid=grid), grid


@pytest.mark.parametrize("env_id,robot_id", FIELD_CASES)
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_occupancy_grid_guide_increment_vs_oracle(env_id, robot_id, mode):
    """the body of test_gpu_grid_sdf.test_grid_guide_increment_vs_oracle (scale 0.9) on a grid made by the distance transform"""
    from oracle.guide import interpolate_points_v1
    from mpd_public_amd import _lib
    weights = (1e-2, 1e-7)
    ds_prim, ds, grid = _datasets(env_id, robot_id, mode)
    assert ds.task.df_collision_objects.grid is grid and (grid.grad is None) == (mode == "linear")
    B = 7
    x = obstacle_hugging_trajs(ds_prim, B, seed=f"g/{env_id}", scale=0.9)
    og, comp, gf, k = _oracle_with_grid(ds_prim, ds, weights)
    xi = interpolate_points_v1(og.normalizer.unnormalize(x.double()), 128)
    cut = {i: ds.task.obstacle_cutoff_margin for i in range(len(comp.cost_l))}
    amb = _to_supports(_classify(comp, gf, xi, cut), 64).numpy()
    active = float((comp.cost_l[k].factors(xi) > 0).double().mean())
    print(f"{env_id} {mode}: ambiguous support waypoints {amb.mean():.4f} (cap {CAP[robot_id]}), active grid hinges {active:.3f}")
    assert amb.mean() <= CAP[robot_id]
    assert active >= 0.25
    ref = og(x.double()).numpy()
    assert np.abs(ref).max() > 0
    pg = product_guide(ds, *weights).cuda()
    got = pg(x.cuda()).cpu().numpy()
    gp = pg.device_params("cuda")
    assert [gp.fields[i].kind for i in range(gp.n_fields)][k] == _lib.FIELD_GRID and gp.grids
    if mode == "linear":
        assert gp.grids == grid.planes("cuda")[0].data_ptr()                       # the single plane is used in place
    assert got.shape == ref.shape == (B, 64, ds.state_dim)
    assert not got[:, 0].any() and not got[:, -1].any()
    atol = 2e-6 * max(weights[0], 1e-2) / 1e-2
    print(f"  max|diff| outside ambiguous = {np.abs(got - ref)[~amb].max():.3e}")
    np.testing.assert_allclose(got[~amb], ref[~amb], rtol=1e-3, atol=atol)


@pytest.mark.parametrize("env_id,robot_id", FIELD_CASES)
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_occupancy_grid_metrics_flags_vs_fp64_reference(env_id, robot_id, mode):
    """the body of test_gpu_grid_sdf.test_grid_metrics_flags_vs_fp64_reference on a grid made by the distance transform"""
    from oracle import costs as oc
    from oracle.guide import interpolate_points_v1
    ds_prim, ds, _ = _datasets(env_id, robot_id, mode)
    B, n_check = 7, 256
    x = obstacle_hugging_trajs(ds_prim, B, seed=f"g/{env_id}", scale=0.9)
    og, comp, gf, k = _oracle_with_grid(ds_prim, ds)
    xu = og.normalizer.unnormalize(x.double()).float()
    xi = interpolate_points_v1(xu.double(), n_check)
    cut = {i: 0.0 for i in range(len(comp.cost_l))}
    amb = _classify(comp, gf, xi, cut).numpy()
    print(f"{env_id} {mode}: ambiguous interpolated waypoints {amb.mean():.4f} (cap {CAP[robot_id]})")
    assert amb.mean() <= CAP[robot_id]
    hit = torch.zeros(xi.shape[:2], dtype=torch.bool)
    for term in comp.cost_l:
        if isinstance(term, oc.CostCollision):
            keep, term.cutoff = term.cutoff, 0.0
            hit |= (term.factors(xi) > 0).any(-1)
            term.cutoff = keep
    hit = hit.numpy()
    assert hit.any() and not hit.all()
    out, mask = ds.task.trajectory_metrics(xu.cuda(), n_check=n_check, return_mask=True)
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    print(f"  flags differing outside ambiguous: {int((mask != hit)[~amb].sum())}; inside: {int((mask != hit)[amb].sum())} of {int(amb.sum())}")
    assert (mask == hit)[~amb].all()
    np.testing.assert_array_equal(out[:, 0], mask.sum(1))
    np.testing.assert_array_equal(out[:, 3], n_check)


# ------------------------------------------------------------------------------------------------------------------------ 4. identities
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_update_occupancy_then_refresh_equals_a_fresh_guide(mode):
    import mpd_public_amd as m
    env_id, robot_id = "EnvSimple2D", "RobotPointMass"
    ds_prim, ds, grid = _datasets(env_id, robot_id, mode, inflate=0.01)
    _, occ, origin, cell = _primitive_occupancy(env_id, robot_id)
    x = obstacle_hugging_trajs(ds_prim, 7, seed=f"g/{env_id}", scale=0.9).cuda()
    pg = product_guide(ds).cuda()
    first = pg(x)
    xu = ds.unnormalize_trajectories(x)
    m_first = ds.task.trajectory_metrics(xu)
    planes = [p.data_ptr() for p in grid.planes("cuda") if p is not None]
    occ2 = np.roll(occ, (9, -14), (0, 1))                                          # the scene moved
    assert (occ2 != occ).any()
    assert grid.update_occupancy(occ=occ2) is grid
    assert [p.data_ptr() for p in grid.planes("cuda") if p is not None] == planes    # written into the planes the grid already holds
    pg.refresh_grids()
    ds.task.refresh_grids()
    second = pg(x)
    fresh_grid = m.GridSDF.from_occupancy(occ2, origin, cell, mode=mode, inflate=0.01)
    ds2 = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA, sdf_grid=fresh_grid)
    want = product_guide(ds2).cuda()(x)
    assert torch.equal(second, want) and not torch.equal(second, first) and float(second.abs().max()) > 0
    assert torch.equal(ds.task.trajectory_metrics(xu), ds2.task.trajectory_metrics(xu))
    assert not torch.equal(ds.task.trajectory_metrics(xu)[:, 0], m_first[:, 0])
    for a, b in zip(grid.node_values(), fresh_grid.node_values()):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_plan_on_an_occupancy_grid_fused_equals_stepwise(mode):
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    env_id, robot_id, opt, T, B, n0 = "EnvSimple2D", "RobotPointMass", 0, 25, 4, 5
    _, occ, origin, cell = _primitive_occupancy(env_id, robot_id)
    ds0 = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
    task = m.PlanningTask(ds0.env, ds0.robot, obstacle_cutoff_margin=ds0.task.obstacle_cutoff_margin, tensor_args=TA,
                          sdf_grid=m.GridSDF.from_occupancy(occ, origin, cell, mode=mode))
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


def test_experiment_entry_takes_a_grid():
    import mpd_public_amd as m
    from mpd_public_amd.inference import experiment
    import tempfile
    env_id, robot_id = "EnvSimple2D", "RobotPointMass"
    _, occ, origin, cell = _primitive_occupancy(env_id, robot_id)
    grid = m.GridSDF.from_occupancy(occ, origin, cell, mode="linear", inflate=0.01)
    n = 6
    with tempfile.TemporaryDirectory() as tmp:
        kw = dict(model_id=f"{env_id}-{robot_id}", planner_alg="mpd", n_samples=n, debug=False, seed=3)
        r = experiment(results_dir=tmp + "/occ", sdf_grid=grid, **kw)
        base = experiment(results_dir=tmp + "/prim", **kw)
        with pytest.raises(ValueError, match="exclude"):
            experiment(results_dir=tmp + "/both", sdf_grid=grid, sdf_grid_cell_size=0.01, **kw)
    assert r["trajs_iters"].shape == base["trajs_iters"].shape and torch.isfinite(r["trajs_iters"]).all()
    assert 0.0 <= r["fraction_free_trajs"] <= 1.0 and 0.0 <= r["collision_intensity_trajs"] <= 1.0
    nf = 0 if r["trajs_final_free"] is None else r["trajs_final_free"].shape[0]
    nc = 0 if r["trajs_final_coll"] is None else r["trajs_final_coll"].shape[0]
    assert nf + nc == n
    xs = r["trajs_iters"]
    assert torch.equal(xs[0], base["trajs_iters"][0])                # same noise: the chains start equal ...
    assert not torch.equal(xs[-1], base["trajs_iters"][-1])          # ... and the occupancy grid is in use: the guided results differ
