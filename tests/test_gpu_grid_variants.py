"""GPU tests of the kernel variants that a grid field (MPDX_FIELD_GRID) selects together with the robot, the Panda's dense layout, several obstacle
scenes and moving obstacles (the launchers' dispatch: k_guide.hip, launch_guide and mpdx_traj_metrics_mask).  Each test first asserts the descriptor
facts that pick the variant - which field is a grid, n_scenes, track_len, the variant mpdx_guide_variant names - and then compares: against the fp64
oracle with the yardstick of tests/test_gpu_grid_sdf.py (_oracle_with_grid, _classify, _to_supports, CAP, rtol 1e-3 / atol 2e-6) or of
tests/moving_ref.py (guide_ref.judge), or bit for bit against a variant that is itself held to the oracle.

Every guide and metrics variant of the built-in robots and the test that holds it ("=" : bit identity to the variant named):

  guide      robot / layout      static                                     several scenes                                   moving obstacles
  no grid    point mass 2-D      test_gpu_guide_terms (terms, fp64)          test_gpu_scenes::..._vs_oracle_scene_by_scene   test_gpu_moving::..._increment_vs_oracle[pm2-*]
             point mass 3-D      test_gpu_guide_terms (terms, fp64)          = static: test_pm3_scenes_guide[nogrid]         test_gpu_moving::..._increment_vs_oracle[pm3-H24]
             Panda, table        test_gpu_guide_terms (terms, fp64)          test_gpu_scenes::..._vs_oracle_scene_by_scene   test_gpu_moving::..._increment_vs_oracle[panda-H64]
             Panda, dense        test_gpu_guide_terms::test_panda_dense_...  = static: test_gpu_scenes::test_dense_panda_... test_gpu_moving::test_moving_panda_dense_...
  grid       point mass 2-D      test_gpu_grid_sdf::..._increment_vs_oracle  = static: test_gpu_scenes::...[pointmass2d-grid] test_gpu_moving::..._increment_vs_oracle[pm2-H64-grid]
             point mass 3-D      test_pm3_grid_guide_and_metrics_vs_oracle   = static: test_pm3_scenes_guide[grid]           test_gpu_moving::..._increment_vs_oracle[pm3-H24-grid]
             Panda, table        test_gpu_grid_sdf::..._increment_vs_oracle  = static: test_panda_grid_scenes_guide_table    test_gpu_moving::..._increment_vs_oracle[panda-H64-grid]
             Panda, dense        test_panda_dense_grid_vs_oracle             = static: test_panda_grid_scenes_guide_dense    test_panda_dense_grid_vs_oracle (panda-H64-grid)

  metrics    robot               static                                     several scenes                                   moving obstacles
  no grid    point mass 2-D      test_gpu_guide_terms::test_metrics_flags_.. = static: test_gpu_scenes::test_batched_metrics_ test_gpu_moving::test_moving_metrics_flags_..[pm2-H64]
             point mass 3-D      test_gpu_guide_terms::test_metrics_flags_.. = static: test_scenes_metrics[pm3-nogrid]       = static: test_gpu_moving::test_zero_track_changes_no_bit[pm3-H24]
             Panda               test_gpu_guide_terms::test_metrics_flags_.. = static: test_gpu_scenes::test_batched_metrics_ test_gpu_moving::test_moving_metrics_flags_..[panda-H64]
  grid       point mass 2-D      test_gpu_grid_sdf::..._metrics_flags_..     = static: test_scenes_metrics[pm2-grid]         test_gpu_moving::test_moving_metrics_flags_..[pm2-H64-grid]
             point mass 3-D      test_pm3_grid_guide_and_metrics_vs_oracle   = static: test_scenes_metrics[pm3-grid]         test_gpu_moving::test_moving_metrics_flags_..[pm3-H24-grid]
             Panda               test_gpu_grid_sdf::..._metrics_flags_..     = static: test_scenes_metrics[panda-grid]       test_gpu_moving::test_moving_metrics_flags_..[panda-H64-grid]

Scene batches and tracks do not combine (refused on the host), and the point mass has no dense layout.  The grid geometry itself (boxes that link
points leave, node counts that differ per axis, two grids in one block) is tests/test_gpu_grid_edges.py."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import grid_edges_ref as ger
import guide_ref as gr
import moving_ref as mr
from helpers import obstacle_hugging_trajs, product_guide
from scene_ref import N_PER_CONTEXT, SCENE_OF_CONTEXT, single_scene_guides
from test_gpu_grid_sdf import CAP, TA, _classify, _datasets, _oracle_with_grid, _to_supports

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SOC, NPC = SCENE_OF_CONTEXT, N_PER_CONTEXT
WEIGHTS = (1e-2, 1e-7)
PM3_AIM = (1, 3, 4, 11, 14, 0, 6)          # the fixed spheres the 3-D point mass's lines pass through (tests/grid_edges_ref.py::aimed_trajs)
SCENE_CELL = {2: 0.05, 3: 0.05}            # the grid of the scene tests (tests/test_gpu_scenes.py: 0.05 in 2-D)


def _lib():
    from mpd_public_amd import _lib as L
    return L


def _grid_fields(gp):
    L = _lib()
    return [i for i in range(gp.n_fields) if gp.fields[i].kind == L.FIELD_GRID]


def _track_lens(gp):
    L = _lib()
    return [int(gp.fields[i].track_len) for i in range(gp.n_fields) if gp.fields[i].kind == L.FIELD_OBJECTS]


def _variant(gp, B, H, D):
    return int(_lib().load().mpdx_guide_variant(C.byref(gp), B, H, D))


def _check_descriptor(gp, grid_field, n_scenes, track_len, variant=None, shape=None):
    """which field is a grid (index or None), n_scenes (<= 1: one scene), the tracks' lengths (0: none), and - for the guide - the variant"""
    assert _grid_fields(gp) == ([] if grid_field is None else [grid_field])
    if grid_field is not None:
        assert gp.grids and gp.n_grid_floats > 0
    assert (gp.n_scenes if gp.n_scenes > 1 else 1) == n_scenes
    assert max(_track_lens(gp) + [0]) == track_len
    if variant is not None:
        assert _variant(gp, *shape) == variant


# ------------------------------------------------------------------------------------------------------------------------ 1. 3-D point mass, grid
def _compare_guide(comp, gf, og, x, k, cut, H, robot_id, got, what):
    from oracle.guide import interpolate_points_v1
    xi = interpolate_points_v1(og.normalizer.unnormalize(x.double()), 128)
    amb = _to_supports(_classify(comp, gf, xi, {i: cut for i in range(len(comp.cost_l))}), H).numpy()
    active = float((comp.cost_l[k].factors(xi) > 0).double().mean())
    print(f"{what}: ambiguous support waypoints {amb.mean():.4f} (cap {CAP[robot_id]}), active grid hinges {active:.3f}")
    assert amb.mean() <= CAP[robot_id] and active > 0
    ref = og(x.double()).numpy()
    assert np.abs(ref).max() > 0 and got.shape == ref.shape
    assert not got[:, 0].any() and not got[:, -1].any()
    atol = 2e-6 * max(WEIGHTS[0], 1e-2) / 1e-2
    print(f"  max|diff| outside ambiguous = {np.abs(got - ref)[~amb].max():.3e}")
    np.testing.assert_allclose(got[~amb], ref[~amb], rtol=1e-3, atol=atol)


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_pm3_grid_guide_and_metrics_vs_oracle(mode):
    """guide_step_kernel<3, 3, POINTMASS, 8, GRID> and traj_metrics_kernel<3, 3, POINTMASS, GRID>: lines through fixed spheres at mid-time"""
    from oracle import costs as oc
    from oracle.guide import interpolate_points_v1
    env_id, robot_id = "EnvSpheres3D", "RobotPointMass3D"
    ds_prim, ds = _datasets(env_id, robot_id, mode)
    x = ger.aimed_trajs(ds_prim, "variants/pm3", PM3_AIM)
    B, H, D = x.shape
    og, comp, gf, k = _oracle_with_grid(ds_prim, ds, WEIGHTS)
    pg = product_guide(ds, *WEIGHTS).cuda()
    gp = pg.device_params("cuda")
    _check_descriptor(gp, k, 1, 0, 0, (B, H, D))
    got = pg(x.cuda()).cpu().numpy()
    _compare_guide(comp, gf, og, x, k, ds.task.obstacle_cutoff_margin, H, "RobotPointMass", got, f"pm3 {mode}")
    # metrics: the body of test_gpu_grid_sdf.test_grid_metrics_flags_vs_fp64_reference
    n_check = 256
    xu = og.normalizer.unnormalize(x.double()).float()
    xi = interpolate_points_v1(xu.double(), n_check)
    amb = _classify(comp, gf, xi, {i: 0.0 for i in range(len(comp.cost_l))}).numpy()
    assert amb.mean() <= CAP["RobotPointMass"]
    hit = torch.zeros(xi.shape[:2], dtype=torch.bool)
    for term in comp.cost_l:
        if isinstance(term, oc.CostCollision):
            keep, term.cutoff = term.cutoff, 0.0
            hit |= (term.factors(xi) > 0).any(-1)
            term.cutoff = keep
    hit = hit.numpy()
    assert hit.any() and not hit.all()
    _check_descriptor(ds.task._params("cuda"), k, 1, 0)
    out, mask = ds.task.trajectory_metrics(xu.cuda(), n_check=n_check, return_mask=True)
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    print(f"  metrics: flags differing outside ambiguous {int((mask != hit)[~amb].sum())} of {int((~amb).sum())}")
    assert (mask == hit)[~amb].all()
    np.testing.assert_array_equal(out[:, 0], mask.sum(1))


# ------------------------------------------------------------------------------------------------------------------------ 2. Panda, dense, grid
_CHILD_CODE = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import ctypes as C
import numpy as np
import test_gpu_moving as M
import test_gpu_grid_variants as V
out = {{}}
for mode in ("linear", "nearest"):
    for scale in (0.9, 1.06):
        got, gp, shape = V._panda_grid_increment(mode, scale)
        out[f"{{mode}}/{{scale}}"] = got
        out[f"{{mode}}/{{scale}}/variant"] = np.array(V._variant(gp, *shape))
ds, gp, got = M._increment("panda-H64-grid")
out["moving"] = got
out["moving/variant"] = np.array(V._variant(gp, 4, 64, got.shape[2]))
out["moving/track"] = np.array(max(V._track_lens(gp)))
out["moving/grids"] = np.array(V._grid_fields(gp))
np.savez({out!r}, **out)
"""


def _panda_grid_increment(mode, scale):
    """the Panda case of test_gpu_grid_sdf.test_grid_guide_increment_vs_oracle: (increment, params, (B, H, D))"""
    ds_prim, ds = _datasets("EnvSpheres3D", "RobotPanda", mode)
    x = obstacle_hugging_trajs(ds_prim, 7, seed="g/EnvSpheres3D", scale=scale)
    pg = product_guide(ds, *WEIGHTS).cuda()
    got = pg(x.cuda()).cpu().numpy()
    return got, pg.device_params("cuda"), tuple(x.shape)


def test_panda_dense_grid_vs_oracle(tmp_path):
    """guide_step_panda_kernel<DENSE, GRID> and <DENSE, GRID, MOVING>, forced on at these small batches in ONE child process (MPDX_GUIDE_DENSE is
    read once per process): the Panda case of test_gpu_grid_sdf.test_grid_guide_increment_vs_oracle in both modes and both scales, and moving_ref's
    panda-H64-grid.  The child took the dense variant (1), this process takes the table variant (0) for the same blocks."""
    out = tmp_path / "dense_grid.npz"
    code = _CHILD_CODE.format(root=str(ROOT), tests=str(ROOT / "tests"), out=str(out))
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env={**os.environ, "MPDX_GUIDE_DENSE": "1"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(out) as z:
        res = {k: z[k] for k in z.files}
    from oracle.guide import interpolate_points_v1
    for mode in ("linear", "nearest"):
        ds_prim, ds = _datasets("EnvSpheres3D", "RobotPanda", mode)
        og, comp, gf, k = _oracle_with_grid(ds_prim, ds, WEIGHTS)
        gp = product_guide(ds, *WEIGHTS).cuda().device_params("cuda")
        _check_descriptor(gp, k, 1, 0, 0, (7, 64, ds.state_dim))
        for scale in (0.9, 1.06):
            assert int(res[f"{mode}/{scale}/variant"]) == 1
            x = obstacle_hugging_trajs(ds_prim, 7, seed="g/EnvSpheres3D", scale=scale)
            _compare_guide(comp, gf, og, x, k, ds.task.obstacle_cutoff_margin, 64, "RobotPanda", res[f"{mode}/{scale}"], f"panda dense {mode} scale {scale}")
    # the moving case: the dense variant with a grid and a track
    import test_gpu_moving as M
    name = "panda-H64-grid"
    assert int(res["moving/variant"]) == 1 and int(res["moving/track"]) == 64 and res["moving/grids"].size == 1
    ds_m = mr.dataset(name, "cuda")
    gp_m = mr.product(ds_m).cuda().device_params("cuda")
    _check_descriptor(gp_m, int(res["moving/grids"][0]), 1, 64, 0, (4, 64, ds_m.state_dim))
    x, amb, ref = M._reference(name, ds_m)
    gr.judge(res["moving"], ref, amb, mr.WEIGHTS[0], what=f"{name} dense")


# ------------------------------------------------------------------------------------------------------------------------ 3. several scenes
def _scenes_setup(env_id, robot_id, grid):
    import mpd_public_amd as m
    from scene_ref import scene_object_sets
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
    if grid:
        ds.task = m.PlanningTask(ds.env, ds.robot, obstacle_cutoff_margin=ds.task.obstacle_cutoff_margin, sdf_grid=dict(cell_size=SCENE_CELL[ds.env.dim]))
    return ds, m.PlanningScenes(ds.task, scene_object_sets(ds.env.dim))


def _objects_index(ds):
    return [f.name for f in ds.task.get_collision_fields()].index("objects")


def _batched_vs_single(ds, scenes, x, soc, variant):
    """the scene-bound guide over the whole batch against one single-scene guide per scene over the same batch (same per-context range flags), rows
    compared per context, bit for bit; the descriptors of both sides first"""
    L = _lib()
    B, H, D = x.shape
    grid = _objects_index(ds) if ds.task.df_collision_objects.kind == L.FIELD_GRID else None
    bound = product_guide(ds).with_scenes(scenes, soc, NPC).cuda()
    _check_descriptor(bound.device_params("cuda"), grid, scenes.n_scenes, 0, variant, (B, H, D))
    got = bound(x)
    assert got.shape == x.shape and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    lib, st = L.load(), L.current_stream()
    flag = torch.zeros(len(soc), dtype=torch.int32, device="cuda")
    L.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), NPC, B, H, D, st))
    rows = torch.tensor(soc, device="cuda").repeat_interleave(NPC)
    for s, g in enumerate(single_scene_guides(ds, scenes)):
        gp = g.cuda().device_params(x.device)
        _check_descriptor(gp, grid, 1, 0, variant, (B, H, D))
        out = torch.empty_like(x)
        L.check(lib.mpdx_guide_step(C.byref(gp), x.data_ptr(), out.data_ptr(), None, None, flag.data_ptr(), None, NPC, B, H, D, st))
        assert bool((rows == s).any()) and torch.equal(got[rows == s], out[rows == s]), s
        if s:   # the scenes matter on this input
            assert not torch.equal(got[rows == 0], out[rows == 0])


def _scene_trajs(ds, n, seed):
    """normalised [n, 64, D]: tests/helpers.py's lines for the Panda and the 2-D point mass; for the 3-D point mass, whose random lines seldom meet a
    scene's spheres, lines through the spheres of scenes B and C in turn (tests/grid_edges_ref.py::aimed_trajs)"""
    if ds.robot.name == "RobotPointMass" and ds.robot.q_dim == 3:
        from scene_ref import scene_object_sets
        _, sb, sc = scene_object_sets(3)
        centres = np.stack([(sb if i % 2 == 0 else sc).sphere_centers[(i // 2) % 3] for i in range(n)])
        return ger.aimed_trajs(ds, seed, None, centres)
    return obstacle_hugging_trajs(ds, n, seed=seed)


def _scene_inputs(ds, n, tag):
    x = _scene_trajs(ds, n, f"variants/scenes/{tag}")
    x[NPC:2 * NPC] *= 1.12     # context 1 leaves the +-1 range: its whole-tensor clip fires, the other contexts' must not
    return x.cuda()


def test_panda_grid_scenes_guide_table():
    """guide_step_panda_kernel<TABLE, GRID, MULTI_SCENE> at the scene tests' batch (4 contexts x 2)"""
    ds, scenes = _scenes_setup("EnvSpheres3D", "RobotPanda", True)
    _batched_vs_single(ds, scenes, _scene_inputs(ds, len(SOC) * NPC, "panda"), SOC, 0)


def test_panda_grid_scenes_guide_dense():
    """guide_step_panda_kernel<DENSE, GRID, MULTI_SCENE>: 256 contexts x 2 trajectories (the batch from which the launcher takes the dense layout),
    scenes mixed (tests/test_gpu_scenes.py::test_dense_panda_variant_batched_equals_single_scene with a grid)"""
    ds, scenes = _scenes_setup("EnvSpheres3D", "RobotPanda", True)
    n_ctx = 256
    soc = [(5 * c + c // 3) % 3 for c in range(n_ctx)]
    x = obstacle_hugging_trajs(ds, n_ctx * NPC, seed="variants/scenes/dense").cuda()
    _batched_vs_single(ds, scenes, x, soc, 1)


@pytest.mark.parametrize("grid", [False, True], ids=["nogrid", "grid"])
def test_pm3_scenes_guide(grid):
    """guide_step_kernel<3, 3, POINTMASS, 8, GRID?, MULTI_SCENE>"""
    ds, scenes = _scenes_setup("EnvSpheres3D", "RobotPointMass3D", grid)
    _batched_vs_single(ds, scenes, _scene_inputs(ds, len(SOC) * NPC, f"pm3/{grid}"), SOC, 0)


@pytest.mark.parametrize("env_id,robot_id,grid", [("EnvDense2D", "RobotPointMass", True), ("EnvSpheres3D", "RobotPointMass3D", False),
                                                  ("EnvSpheres3D", "RobotPointMass3D", True), ("EnvSpheres3D", "RobotPanda", True)],
                         ids=["pm2-grid", "pm3-nogrid", "pm3-grid", "panda-grid"])
def test_scenes_metrics(env_id, robot_id, grid):
    """traj_metrics_kernel<..., GRID?, MULTI_SCENE> against the single-scene metrics of each context's scene, bit for bit"""
    L = _lib()
    ds, scenes = _scenes_setup(env_id, robot_id, grid)
    B = len(SOC) * NPC
    xu = ds.unnormalize_trajectories(_scene_trajs(ds, B, f"variants/scenes_m/{env_id}/{robot_id}").cuda())
    g = _objects_index(ds) if grid else None
    _check_descriptor(scenes._params(xu.device), g, scenes.n_scenes, 0)
    out, mask = scenes.trajectory_metrics(xu, SOC, NPC, n_check=128, return_mask=True)
    assert out.shape == (B, 4) and mask.shape == (B, 128) and bool(mask.any())
    tasks = [scenes.scene_task(s) for s in range(scenes.n_scenes)]
    per_scene = []
    for c, s in enumerate(SOC):
        _check_descriptor(tasks[s]._params(xu.device), g, 1, 0)
        o, mk = tasks[s].trajectory_metrics(xu[c * NPC:(c + 1) * NPC], n_check=128, return_mask=True)
        assert torch.equal(out[c * NPC:(c + 1) * NPC], o) and torch.equal(mask[c * NPC:(c + 1) * NPC], mk), c
        per_scene.append(mk)
    # the scenes matter: some context of scene B or C has other flags than scene A gives it
    assert any(not torch.equal(per_scene[c], tasks[0].trajectory_metrics(xu[c * NPC:(c + 1) * NPC], n_check=128, return_mask=True)[1]) for c in (0, 2, 3))
    if grid:
        assert L.FIELD_GRID in [f.kind for f in tasks[0].get_collision_fields()]
