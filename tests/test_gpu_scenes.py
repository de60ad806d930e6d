"""GPU checks of the scene batches: contexts with different obstacle scenes in ONE launch of the guide / metrics kernels (MULTI_SCENE instantiations,
csrc/guide.hpp + csrc/scene_table.hpp) against the same contexts run one scene at a time through the single-scene kernels - bit for bit - and
against the oracle (fp64 autograd over oracle/costs.py, scene by scene; tests/scene_ref.py)."""
import ctypes as C
from math import ceil

import numpy as np
import pytest
import torch

from helpers import DIM_MULTS, obstacle_hugging_trajs, product_guide, synth_sd, t
from scene_ref import N_PER_CONTEXT, SCENE_OF_CONTEXT, mismatch_fraction, oracle_increment, scene_dataset, scene_object_sets, single_scene_guides

pytestmark = pytest.mark.gpu

SOC, NPC = SCENE_OF_CONTEXT, N_PER_CONTEXT
B = len(SOC) * NPC


def _setup(env_id, robot_id, **task_kw):
    import mpd_public_amd as m
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args={"device": "cuda", "dtype": torch.float32})
    if task_kw:
        ds.task = m.PlanningTask(ds.env, ds.robot, obstacle_cutoff_margin=ds.task.obstacle_cutoff_margin, **task_kw)
    scenes = m.PlanningScenes(ds.task, scene_object_sets(ds.env.dim))
    return ds, scenes


def _inputs(ds, tag):
    """Normalised [B,64,D] trajectories on which every context is sensitive to its scene (seed chosen with the oracle: each context's increment
    differs between scenes A, B and C)."""
    x = obstacle_hugging_trajs(ds, B, seed=f"scenes/clamp/{tag}")
    x[NPC:2 * NPC] *= 1.12     # context 1 leaves the +-1 range: its whole-tensor clip fires, the other contexts' must not
    return x.cuda()


# ---------------------------------------------------------------------------------------------------------------- 1. guide, gradient only
@pytest.mark.parametrize("env_id,robot_id,task_kw", [("EnvDense2D", "RobotPointMass", {}), ("EnvSpheres3D", "RobotPanda", {}),
                                                      ("EnvDense2D", "RobotPointMass", {"sdf_grid": dict(cell_size=0.05)})],
                         ids=["pointmass2d", "panda", "pointmass2d-grid"])
def test_batched_guide_equals_single_scene_guides(env_id, robot_id, task_kw):
    ds, scenes = _setup(env_id, robot_id, **task_kw)
    x = _inputs(ds, env_id)
    bound = product_guide(ds).with_scenes(scenes, SOC, NPC).cuda()
    got = bound(x)
    assert got.shape == x.shape and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    singles = [g.cuda() for g in single_scene_guides(ds, scenes)]
    ref = [singles[s](x[c * NPC:(c + 1) * NPC]) for c, s in enumerate(SOC)]
    for c in range(len(SOC)):
        assert torch.equal(got[c * NPC:(c + 1) * NPC], ref[c]), c
    # the scenes matter on this input: a context against another scene's guide gives another increment
    for c, s in enumerate(SOC):
        for other in range(scenes.n_scenes):
            if other != s:
                assert not torch.equal(ref[c], singles[other](x[c * NPC:(c + 1) * NPC])), (c, s, other)
    with pytest.raises(ValueError, match="batch"):
        bound(x[:NPC])


def test_dense_panda_variant_batched_equals_single_scene():
    """From batch 512 on the Panda guide runs its dense variant (no FK table in LDS, two workgroups per CU) - another instantiation, so the one
    case above the small shapes: 256 contexts x 2 trajectories, scenes mixed, against the single-scene dense kernel per scene over the same batch
    (same per-context range flags), rows compared per context."""
    from mpd_public_amd import _lib
    ds, scenes = _setup("EnvSpheres3D", "RobotPanda")
    n_ctx, D = 256, ds.state_dim
    nB = n_ctx * NPC
    soc = [(5 * c + c // 3) % 3 for c in range(n_ctx)]
    x = obstacle_hugging_trajs(ds, nB, seed="scenes/dense").cuda()
    got = product_guide(ds).with_scenes(scenes, soc, NPC).cuda()(x)
    assert bool(torch.isfinite(got).all())
    lib, st = _lib.load(), _lib.current_stream()
    flag = torch.zeros(n_ctx, dtype=torch.int32, device="cuda")
    _lib.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), NPC, nB, 64, D, st))
    rows = torch.tensor(soc, device="cuda").repeat_interleave(NPC)
    for s, g in enumerate(single_scene_guides(ds, scenes)):
        out = torch.empty_like(x)
        _lib.check(lib.mpdx_guide_step(C.byref(g.cuda().device_params(x.device)), x.data_ptr(), out.data_ptr(), None, None, flag.data_ptr(), None, NPC, nB, 64, D, st))
        assert int((rows == s).sum()) > 100 and torch.equal(got[rows == s], out[rows == s]), s
        if s:
            assert not torch.equal(got[rows == 0], out[rows == 0])


def test_one_scene_params_take_the_single_scene_kernels():
    """n_scenes = 1 with scene members that n_scenes = 2 would refuse: the block is a single-scene block, same bits as the zero block."""
    from mpd_public_amd import _lib
    ds, _ = _setup("EnvDense2D", "RobotPointMass")
    x = _inputs(ds, "one")
    pg = product_guide(ds).cuda()
    ref = pg(x)
    gp = type(pg.device_params(x.device)).from_buffer_copy(pg.device_params(x.device))
    gp.n_scenes, gp.scene_stride, gp.scene_of_ctx, gp.scene_n_per_ctx = 1, 3, None, -1
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty_like(x)
    lib, st = _lib.load(), _lib.current_stream()
    _lib.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), B, B, 64, 4, st))
    _lib.check(lib.mpdx_guide_step(C.byref(gp), x.data_ptr(), out.data_ptr(), None, None, flag.data_ptr(), None, B, B, 64, 4, st))
    assert torch.equal(out, ref)


# ---------------------------------------------------------------------------------------------------------------- 2. guided plan
@pytest.mark.parametrize("env_id,robot_id,opt", [("EnvDense2D", "RobotPointMass", 0), ("EnvSpheres3D", "RobotPanda", 1)], ids=["pointmass2d", "panda"])
def test_batched_guided_plan_equals_single_scene_plans(env_id, robot_id, opt):
    """The fused plan with the scene-bound guide == one single-scene plan per context on the same noise slices, bit for bit; context 1 starts from
    1.5 x the noise, so that its range test fires in the early guided iterations and the others' does not.  The same on the step-by-step loop."""
    import mpd_public_amd as m
    from mpd_public_amd.parallel import plan_contexts
    T, n0 = 25, 2
    ds, scenes = _setup(env_id, robot_id)
    D, qd = ds.state_dim, ds.state_dim // 2
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
    noise = t(f"scenes_noise/{env_id}", (T + n0 + 1, B, 64, D)).cuda()
    noise[0, NPC:2 * NPC] *= 1.5
    cfg = lambda tag, c: ds.normalizer.normalize(torch.cat([t(f"scenes_{tag}{c}/{env_id}", (qd,), "uniform", 0.6).cuda(), torch.zeros(qd, device="cuda")]))
    starts, goals = torch.stack([cfg("s", c) for c in range(len(SOC))]), torch.stack([cfg("g", c) for c in range(len(SOC))])
    pg = product_guide(ds).cuda()
    singles = [g.cuda() for g in single_scene_guides(ds, scenes)]
    kw = dict(n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5, n_guide_steps=5, t_start_guide=ceil(0.25 * T))
    batched, (lo, hi) = plan_contexts(dm, starts, goals, NPC, horizon=64, noise=noise, guide=pg, scenes=scenes, scene_of_context=SOC, **kw)
    assert (lo, hi) == (0, len(SOC)) and batched.shape == (B, 64, D) and bool(torch.isfinite(batched).all())
    sep = []
    for c, s in enumerate(SOC):
        nz = noise[:, c * NPC:(c + 1) * NPC].contiguous()
        x, _ = dm.plan({0: starts[c], 63: goals[c]}, NPC, 64, noise=nz, return_chain=False, guide=singles[s], **kw)
        assert torch.equal(batched[c * NPC:(c + 1) * NPC], x), c
        sep.append(x)
    # the scene reaches the plan: a context of scene B or C planned against scene A ends elsewhere
    differs = []
    for c in (0, 2, 3):
        xA, _ = dm.plan({0: starts[c], 63: goals[c]}, NPC, 64, noise=noise[:, c * NPC:(c + 1) * NPC].contiguous(), return_chain=False, guide=singles[0], **kw)
        differs.append(not torch.equal(xA, sep[c]))
    assert any(differs)
    # plan() directly, n_per_context taken from the bound guide; a batch of another shape is refused
    bound = pg.with_scenes(scenes, SOC, NPC)
    hs, hg = starts.repeat_interleave(NPC, 0).contiguous(), goals.repeat_interleave(NPC, 0).contiguous()
    x2, _ = dm.plan({0: hs, 63: hg}, B, 64, noise=noise, return_chain=False, guide=bound, **kw)
    assert torch.equal(x2, batched)
    with pytest.raises(ValueError):
        dm.plan({0: hs[:NPC], 63: hg[:NPC]}, NPC, 64, noise=noise[:, :NPC].contiguous(), return_chain=False, guide=bound, **kw)
    # step-by-step protocol loop (one call per step; the guide's own range test per context)
    loop = dm.run_inference(None, {0: hs, 63: hg}, n_samples=B, horizon=64, fused=False, noise=noise, guide=bound, **kw)
    assert loop.shape == (B, 64, D)
    for c, s in enumerate(SOC):
        nz = noise[:, c * NPC:(c + 1) * NPC].contiguous()
        x = dm.run_inference(None, {0: starts[c], 63: goals[c]}, n_samples=NPC, horizon=64, fused=False, noise=nz, guide=singles[s], **kw)
        assert torch.equal(loop[c * NPC:(c + 1) * NPC], x), c


# ---------------------------------------------------------------------------------------------------------------- 3. metrics
@pytest.mark.parametrize("env_id,robot_id", [("EnvDense2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")], ids=["pointmass2d", "panda"])
def test_batched_metrics_equal_single_scene_metrics(env_id, robot_id):
    ds, scenes = _setup(env_id, robot_id)
    xu = ds.unnormalize_trajectories(obstacle_hugging_trajs(ds, B, seed=f"scenes_m/{env_id}").cuda())
    out, mask = scenes.trajectory_metrics(xu, SOC, NPC, n_check=128, return_mask=True)
    assert out.shape == (B, 4) and mask.shape == (B, 128)
    tasks = [scenes.scene_task(s) for s in range(scenes.n_scenes)]
    per_scene = []
    for c, s in enumerate(SOC):
        o, mk = tasks[s].trajectory_metrics(xu[c * NPC:(c + 1) * NPC], n_check=128, return_mask=True)
        assert torch.equal(out[c * NPC:(c + 1) * NPC], o) and torch.equal(mask[c * NPC:(c + 1) * NPC], mk), c
        per_scene.append(mk)
    assert bool(mask.any())
    # the scenes matter: some context of scene B or C has other flags than scene A gives it
    assert any(not torch.equal(per_scene[c], tasks[0].trajectory_metrics(xu[c * NPC:(c + 1) * NPC], n_check=128, return_mask=True)[1]) for c in (0, 2, 3))
    assert torch.equal(scenes.trajectory_metrics(xu, SOC, NPC, n_check=128), out)
    # the derived figures take the assignment too
    m4 = scenes.trajectory_metrics(xu, SOC, NPC)
    assert scenes.compute_fraction_free_trajs(xu, SOC, NPC) == float((m4[:, 0] == 0).float().mean())
    assert scenes.compute_collision_intensity_trajs(xu, SOC, NPC) == float((m4[:, 0] / m4[:, 3]).mean())
    tc, ic, tf, i_f, _ = scenes.get_trajs_collision_and_free(xu, SOC, NPC, return_indices=True)
    assert sorted(ic.tolist() + i_f.tolist()) == list(range(B)) and ic.tolist() == torch.nonzero(m4[:, 0] > 0).flatten().tolist()
    with pytest.raises(ValueError):
        scenes.trajectory_metrics(xu, [0, 1, 3, 2], NPC)
    with pytest.raises(ValueError):
        scenes.trajectory_metrics(xu, SOC[:3], NPC)


def test_metrics_closed_form_sphere_only_in_one_scene():
    """An empty 2-D world; scene B alone holds one sphere (centre (0.2, 0.1), radius 0.155).  The straight line y = 0.1 from x = -0.5 to x = 0.7, checked
    on 121 waypoints (x_i = -0.5 + i / 100), collides where |x_i - 0.2| < 0.155 + 0.01 (the link radius): i = 54 ... 86, 33 waypoints - in B's
    contexts, and nowhere in A's."""
    import mpd_public_amd as m
    from mpd_public_amd.planning import Env
    e = m.ObjectSet.empty()
    env = Env("Empty2D", 2, m.ObjectSet.empty(), m.ObjectSet.empty())
    task = m.PlanningTask(env, m.make_robot("RobotPointMass"))
    ball = m.ObjectSet(np.array([[0.2, 0.1, 0.0]], np.float32), np.array([0.155], np.float32), e.box_centers, e.box_half)
    scenes = m.PlanningScenes(task, [e, ball])
    H = 64
    s = torch.linspace(0, 1, H, dtype=torch.float64).reshape(1, H, 1)
    line = torch.cat([-0.5 + 1.2 * s, torch.full_like(s, 0.1), torch.zeros(1, H, 2, dtype=torch.float64)], -1).float()
    xu = line.expand(6, H, 4).contiguous().cuda()
    soc = [1, 0, 1]
    out, mask = scenes.trajectory_metrics(xu, soc, 2, n_check=121, return_mask=True)
    xs = -0.5 + np.arange(121) / 100.0
    want = np.abs(xs - 0.2) < 0.165
    assert want.sum() == 33 and np.abs(np.abs(xs - 0.2) - 0.165).min() > 4e-3    # no waypoint near the boundary: the fp32 flags are decided
    for b in range(6):
        hit = soc[b // 2] == 1
        assert out[b, 0].item() == (33 if hit else 0) and out[b, 3].item() == 121, b
        assert mask[b].cpu().numpy().tolist() == (want.tolist() if hit else [False] * 121), b
    assert torch.allclose(out[:, 1], torch.full((6,), 1.2, device="cuda"), rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 4. oracle
@pytest.mark.parametrize("env_id,robot_id", [("EnvDense2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")], ids=["pointmass2d", "panda"])
def test_batched_guide_vs_oracle_scene_by_scene(env_id, robot_id):
    """The batched increment against fp64 autograd of oracle.costs evaluated scene by scene: the project's guide tolerance,
    1e-3 rel / 2e-6 abs on >= 99 % of the waypoints, at the reference's weights.  Inputs: tests/helpers.py::obstacle_hugging_trajs (the fp32 oracle
    stays inside the same cap on them: tests/test_scenes_cpu.py)."""
    ds, scenes = _setup(env_id, robot_id)
    x = obstacle_hugging_trajs(ds, B, seed=f"scenes/{env_id}")
    ref = oracle_increment(ds, scenes, SOC, NPC, x, torch.float64).numpy()
    got = product_guide(ds).with_scenes(scenes, SOC, NPC).cuda()(x.cuda()).cpu().numpy()
    assert got.shape == ref.shape and np.abs(ref).max() > 0
    assert not got[:, 0].any() and not got[:, -1].any()
    frac, bad = mismatch_fraction(got, ref)
    print(f"{env_id}: {bad.sum()} of {bad.size} waypoints outside 1e-3 rel / 2e-6 abs; max|diff| = {np.abs(got - ref).max():.3e}")
    assert frac < 0.01, f"{bad.sum()} of {bad.size} waypoints differ; max|diff|={np.abs(got - ref).max():.3e}"
    np.testing.assert_allclose(got[~bad], ref[~bad], rtol=1e-3, atol=2e-6)


# ---------------------------------------------------------------------------------------------------------------- 5. clamp
@pytest.mark.parametrize("env_id,robot_id", [("EnvDense2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")], ids=["pointmass2d", "panda"])
def test_scene_index_is_clamped_by_the_kernels(env_id, robot_id):
    """The Python layer range-checks the assignment; the C ABI cannot (the table is device memory), so the kernels clamp: an entry >= n_scenes
    selects the last scene, a negative one the first - finite output, equal to what the clamped table gives."""
    from mpd_public_amd import _lib
    import mpd_public_amd as m
    ds, scenes = _setup(env_id, robot_id)
    D = ds.state_dim
    x = _inputs(ds, env_id)
    bound = product_guide(ds).with_scenes(scenes, [2, 0, 2, 0], NPC).cuda()
    ref = bound(x)
    gp, table = m.PlanningScenes.bind(bound.device_params(x.device), [7, -3, 2 ** 31 - 1, 0], NPC, x.device)
    lib, st = _lib.load(), _lib.current_stream()
    flag = torch.zeros(len(SOC), dtype=torch.int32, device="cuda")
    out = torch.empty_like(x)
    _lib.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), NPC, B, 64, D, st))
    _lib.check(lib.mpdx_guide_step(C.byref(gp), x.data_ptr(), out.data_ptr(), None, None, flag.data_ptr(), None, NPC, B, 64, D, st))
    assert bool(torch.isfinite(out).all()) and torch.equal(out, ref)
    xu = ds.unnormalize_trajectories(x)
    want = scenes.trajectory_metrics(xu, [2, 0, 2, 0], NPC, n_check=64)
    mgp, mtable = m.PlanningScenes.bind(scenes._params(x.device), [7, -3, 2 ** 31 - 1, 0], NPC, x.device)
    o4 = torch.empty((B, 4), dtype=torch.float32, device="cuda")
    _lib.check(lib.mpdx_traj_metrics(C.byref(mgp), xu.contiguous().data_ptr(), o4.data_ptr(), 64, B, 64, D, st))
    assert torch.equal(o4, want)
