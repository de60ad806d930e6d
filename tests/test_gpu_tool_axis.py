"""GPU tests of the tool-axis constraint of chain robots (planning.CostToolAxis; csrc/chain.hpp: the fifth cost slot of guide_step_chain_kernel and
traj_tool_chain_kernel): the guide increment against the fp64 autograd reference of tests/tool_ref.py, off means off, apply mode, descent, the
metrics, the plan's identities, scene batches and the experiment() entry.

Robots, horizons, inputs and seeds are those of tests/test_gpu_chain.py (chain_ref.chain_trajs); what the comparison presupposes - the reference's
own fp32-against-fp64 error, the share of active hinges, the share of points on the hinge's edge - is asserted from the reference alone before the
kernel's output is looked at."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from chain_ref import chain_trajs, description, mismatch_fraction, probe_configs, product_robot
from helpers import DIM_MULTS, synth_sd, t
from scene_ref import N_PER_CONTEXT, scene_dataset, scene_object_sets
import tool_ref as tr

pytestmark = pytest.mark.gpu

CASES = [("R1", 64), ("R3", 64), ("R3", 24), ("R8", 64), ("Panda", 64), ("R3", 96), ("R1", 9)]   # tests/test_gpu_chain.py::CASES
B = 3
SEED = "0"
W = (1e-2, 1e-7)
QD = {"R1": 1, "R3": 3, "R8": 8, "Panda": 7}
# frame = n_joints everywhere, n_joints - 1 as well on R3, R8 and the Panda (the joints above the frame get exactly 0)
VARIANTS = [(n, h, QD[n]) for n, h in CASES] + [(n, h, QD[n] - 1) for n, h in CASES if n in ("R3", "R8", "Panda")]


def _n_interp(H):
    return 128 if 128 <= 8 * H else 2 * H + 1


@functools.lru_cache(maxsize=None)
def _case(name, H):
    """(dataset on the GPU, description, normalised x [B, H, D] on the CPU)"""
    import mpd_public_amd as m
    ds = m.TrajectoryDataset("EnvSpheres3D", product_robot(name), n_support_points=H, tensor_args={"device": "cuda", "dtype": torch.float32})
    x = chain_trajs(ds.robot.q_dim, B, H, f"chain/{name}/{H}/{SEED}", probes=probe_configs(name, ds))
    return ds, description(name), x


@functools.lru_cache(maxsize=None)
def _reference(name, H, frame, setting):
    """fp64 increment of a variant in a setting, computed once and read-only; the reference-only conditions are asserted here."""
    from oracle.guide import interpolate_points_v1
    ds, desc, x = _case(name, H)
    tilt = tr.MAX_TILT[name, H, frame]
    tool = tr.ToolAxisRef(desc, frame, tilt)
    og, _ = tr.oracle_guide_tool(ds, desc, tool, setting, *W, n_interp=_n_interp(H))
    ref = og(x.double()).numpy()
    ref.setflags(write=False)
    active, edge = tr.hinge_conditions(tool, interpolate_points_v1(og.normalizer.unnormalize(x.double()), _n_interp(H)))
    og32, _ = tr.oracle_guide_tool(ds, desc, tr.ToolAxisRef(desc, frame, tilt, dtype=torch.float32), setting, *W, n_interp=_n_interp(H))
    got32 = og32(x.float()).numpy()
    frac32, _ = mismatch_fraction(got32, ref, tr.W_TOOL)
    print(f"{name} H={H} frame {frame} {setting}: {100 * active:.1f} % of the points have an active hinge, {100 * edge:.3f} % within 1e-5 of the edge; reference fp32 vs "
          f"fp64 leaves out {100 * frac32:.3f} % of the waypoints, max|diff| = {np.abs(got32 - ref).max():.2e} at max|ref| = {np.abs(ref).max():.2e}")
    assert 0.10 <= active <= 0.90
    assert edge < 0.01
    assert frac32 < 0.005
    assert np.abs(ref).max() > 0
    return ref


def _guide(name, H, frame, setting, max_tilt=None, w_tool=tr.W_TOOL):
    ds = _case(name, H)[0]
    pg, tool = tr.product_guide_tool(ds, frame, tr.MAX_TILT[name, H, frame] if max_tilt is None else max_tilt, setting, *W, w_tool=w_tool, n_interp=_n_interp(H))
    return pg.cuda(), tool


def _check_increment(got, ref, what):
    frac, bad = mismatch_fraction(got, ref, tr.W_TOOL)
    print(f"{what}: {int(bad.sum())} of {bad.size} waypoints outside 1e-3 rel / 2e-6 abs; max|diff| = {np.abs(got - ref).max():.3e}; max|ref| = {np.abs(ref).max():.3e}")
    assert not got[:, 0].any() and not got[:, -1].any()      # the endpoints are zeroed exactly
    assert frac <= 0.01, f"{what}: {100 * frac:.2f} % of the waypoints differ"
    np.testing.assert_allclose(got[~bad], ref[~bad], rtol=1e-3, atol=2e-6)


def _apply(pg, xg, hs, hg):
    """One apply-mode launch on a copy of xg: (y, max|y| flag as float)."""
    from mpd_public_amd import _lib
    n, H, D = xg.shape
    lib, gp, st = _lib.load(), pg.device_params(xg.device), _lib.current_stream()
    flag_in = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.mpdx_absmax(xg.data_ptr(), flag_in.data_ptr(), n, n, H, D, st))
    flag_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = xg.clone()
    _lib.check(lib.mpdx_guide_step(C.byref(gp), y.data_ptr(), None, hs.data_ptr(), hg.data_ptr(), flag_in.data_ptr(), flag_out.data_ptr(), n, n, H, D, st))
    return y, flag_out.view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------- 5. increment
@pytest.mark.parametrize("setting", tr.SETTINGS)
@pytest.mark.parametrize("name,H,frame", VARIANTS, ids=[f"{n}-H{h}-f{f}" for n, h, f in VARIANTS])
def test_tool_increment_vs_fp64_reference(name, H, frame, setting):
    """Gradient-only mode against the fp64 autograd reference under the project's yardstick (1e-3 relative / 2e-6 absolute, at
    most 1 % of the waypoints left out, endpoints exactly zero).  With the term alone, the velocity dims and every joint above the frame get exactly 0."""
    ref = _reference(name, H, frame, setting)
    ds, desc, x = _case(name, H)
    pg, _ = _guide(name, H, frame, setting)
    got = pg(x.cuda())
    assert got.shape == (B, H, ds.state_dim)
    got = got.cpu().numpy()
    _check_increment(got, ref, f"{name} H={H} frame {frame} {setting}")
    if setting == "alone":
        assert not got[..., frame:].any()
        assert got[..., :frame].any()


# ---------------------------------------------------------------------------------------------------------------- 6. off means off
def _plan_model(D, T=5):
    import mpd_public_amd as m
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[0])
    net.load_state_dict(synth_sd(D, 0), strict=True)
    # (cosine: the reference's exponential formula gives non-finite buffers at 5 steps)
    return m.GaussianDiffusionModel(model=net, variance_schedule="cosine", n_diffusion_steps=T, predict_epsilon=True).cuda().eval()


@pytest.mark.parametrize("name", ["R3", "Panda"])
def test_a_term_that_is_never_active_changes_nothing(name):
    """max_tilt = pi: the hinge is never active.  With the term on (any weight), apply mode gives x and absmax_out bit-equal to the launch without
    the term; a plan that draws its noise inside the guide kernel gives the same bits too - with four fields and the term, three waves draw the noise
    instead of four."""
    from helpers import product_guide
    ds, desc, x = _case(name, 64)
    D = ds.state_dim
    assert len(ds.task.get_collision_fields()) == 4
    pg_off = product_guide(ds, *W).cuda()
    pg_on, _ = _guide(name, 64, QD[name], "full", max_tilt=math.pi, w_tool=7.0)
    xg = x.cuda()
    assert torch.equal(pg_on(xg), pg_off(xg))
    hs, hg = t(f"tool_hs/{name}", (B, D), "uniform").cuda(), t(f"tool_hg/{name}", (B, D), "uniform").cuda()
    (y_on, f_on), (y_off, f_off) = _apply(pg_on, xg, hs, hg), _apply(pg_off, xg, hs, hg)
    assert torch.equal(y_on, y_off) and torch.equal(f_on, f_off) and not torch.equal(y_on, xg)
    # the drawn noise: in-kernel Philox draw (noise=None, no pre-generated tensor); the guided steps draw it in the guide kernel
    dm = _plan_model(D)
    dm.in_kernel_noise_min_bytes = 0
    cfg = lambda tag: ds.normalizer.normalize(torch.cat([t(f"tool_plan_{tag}/{name}", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    hc = {0: cfg("s"), 63: cfg("g")}
    kw = dict(n_diffusion_steps_without_noise=2, noise_std_extra_schedule_fn=lambda tt: 0.5, n_guide_steps=2, t_start_guide=3, return_chain=False)
    plans = []
    for pg in (pg_on, pg_off, None):
        dm.manual_seed(11)
        plans.append(dm.plan(hc, B, 64, guide=pg, **kw)[0])
    assert bool(torch.isfinite(plans[0]).all()) and torch.equal(plans[0], plans[1]) and not torch.equal(plans[1], plans[2])


# ---------------------------------------------------------------------------------------------------------------- 7. apply mode
@pytest.mark.parametrize("name,H", [("R3", 64), ("R1", 9)])
def test_apply_mode_is_x_plus_the_increment(name, H):
    """y == x + increment with the hard conditions written and max|x_new| flagged, bit for bit."""
    ds, desc, x = _case(name, H)
    D = ds.state_dim
    pg, _ = _guide(name, H, QD[name], "full")
    xg = x.cuda()
    inc = pg(xg)
    assert float(inc.abs().max()) > 0
    hs, hg = t(f"tool_hs/{name}", (B, D), "uniform").cuda(), t(f"tool_hg/{name}", (B, D), "uniform").cuda()
    want = xg + inc
    want[:, 0], want[:, -1] = hs, hg
    y, flag = _apply(pg, xg, hs, hg)
    assert torch.equal(y, want)
    assert torch.equal(flag, want.abs().reshape(1, -1).max(1)[0])


# ---------------------------------------------------------------------------------------------------------------- 8. descent
def test_descent_on_the_panda_chain():
    """Panda chain, H = 64, the term alone, weight 1e-2, max_tilt 0.3, frame 7: 100 apply-mode iterations with the hard conditions equal to the
    trajectory's own endpoints.  The fp64 reference brings every trajectory's cost to at most 0.05 of its initial value (asserted from the reference
    alone); the GPU's final trajectories, evaluated with the fp64 cost, are at most 0.10 of it."""
    from oracle.guide import interpolate_points_v1
    ds, desc, x = _case("Panda", 64)
    tool = tr.ToolAxisRef(desc, 7, 0.3)
    og, _ = tr.oracle_guide_tool(ds, desc, tool, "alone", *W)
    cost = lambda xn: tool(interpolate_points_v1(og.normalizer.unnormalize(xn.double()), 128))
    c0 = cost(x)
    xr = x.double().clone()
    for _ in range(100):
        xr = xr + og(xr)
    ratio_ref = (cost(xr) / c0).numpy()
    print(f"fp64 reference: cost after 100 iterations / initial cost = {ratio_ref}, initial {c0.numpy()}")
    assert (c0 > 0).all() and (ratio_ref <= 0.05).all()
    pg, _ = _guide("Panda", 64, 7, "alone", max_tilt=0.3)
    y = x.cuda()
    hs, hg = y[:, 0].contiguous(), y[:, -1].contiguous()
    for _ in range(100):
        y, _flag = _apply(pg, y, hs, hg)
    ratio = (cost(y.cpu()) / c0).numpy()
    print(f"GPU: cost after 100 iterations / initial cost = {ratio}")
    assert torch.equal(y[:, 0], hs) and torch.equal(y[:, -1], hg)
    assert (ratio <= 0.10).all()


# ---------------------------------------------------------------------------------------------------------------- 9. metrics
@pytest.mark.parametrize("name", ["R3", "Panda"])
def test_tool_metrics_vs_fp64_reference(name):
    from mpd_public_amd import _lib
    from oracle.guide import interpolate_points_v1
    from oracle.normalizer import LimitsNormalizer
    ds, desc, x = _case(name, 64)
    frame, n_check = QD[name], 256
    tilt = tr.MAX_TILT[name, 64, frame]
    tool = tr.ToolAxisRef(desc, frame, tilt)
    nrm = LimitsNormalizer(ds.normalizer.mins.cpu(), ds.normalizer.maxs.cpu())
    nrm.mins, nrm.maxs = nrm.mins.double(), nrm.maxs.double()
    xu32 = nrm.unnormalize(x.double()).float()          # what the kernel is given
    d = tool.d(interpolate_points_v1(xu32.double(), n_check))
    slack = tool.cos_min - d
    band = slack.abs() <= 1e-5
    print(f"{name}: {int(band.sum())} of {band.numel()} points within 1e-5 of cos(max_tilt); {int((slack > 0).sum())} are tilted too far")
    assert float(band.double().mean()) <= 0.01 and bool((slack > 0).any()) and bool((slack < 0).any())
    pg, cost = _guide(name, 64, frame, "alone")
    gp = pg.device_params("cuda")
    xg = xu32.cuda()
    out = torch.empty((B, 2), dtype=torch.float32, device="cuda")
    mask = torch.empty((B, n_check), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().mpdx_traj_tool_metrics(C.byref(gp), xg.data_ptr(), out.data_ptr(), mask.data_ptr(), n_check, B, 64, ds.state_dim, _lib.current_stream()))
    out, mask = out.cpu(), mask.cpu().bool()
    assert torch.equal(mask[~band], (slack > 0)[~band])
    assert torch.equal(out[:, 1], mask.sum(1).float())
    print(f"{name}: max |min d - fp64| = {float((out[:, 0].double() - d.min(1)[0]).abs().max()):.2e}")
    assert float((out[:, 0].double() - d.min(1)[0]).abs().max()) <= 1e-5
    # the task's method: the angles of those figures, the same counts and flags; without a mask: the same two tensors
    ang, n_bad, mk = ds.task.tool_axis_metrics(xg, cost, n_check=n_check, return_mask=True)
    assert torch.equal(ang.cpu(), torch.acos(out[:, 0].clamp(-1.0, 1.0))) and torch.equal(n_bad.cpu(), out[:, 1]) and torch.equal(mk.cpu(), mask)
    np.testing.assert_allclose(ang.cpu().double().numpy(), torch.acos(d.min(1)[0].clamp(-1, 1)).numpy(), atol=1e-4)
    ang2, n_bad2 = ds.task.tool_axis_metrics(xg, cost, n_check=n_check)
    assert torch.equal(ang2, ang) and torch.equal(n_bad2, n_bad)
    with pytest.raises(RuntimeError):
        ds.task.tool_axis_metrics(xu32, cost)          # the GPU only


# ---------------------------------------------------------------------------------------------------------------- 10. plan
def _plan_setup():
    ds = _case("R3", 64)[0]
    D, T, n0 = ds.state_dim, 5, 2
    dm = _plan_model(D, T)
    noise = t("chain_plan_noise", (T + n0 + 1, 4, 64, D))[:, :B].contiguous().cuda()
    cfg = lambda tag, c: ds.normalizer.normalize(torch.cat([t(f"chain_plan_{tag}{c}", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    starts, goals = torch.stack([cfg("s", c) for c in range(4)]), torch.stack([cfg("g", c) for c in range(4)])
    kw = dict(n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5, n_guide_steps=2, t_start_guide=3)
    return ds, dm, noise, starts, goals, kw


def test_plan_fused_equals_the_step_by_step_loop_with_the_term():
    """The assertion of tests/test_gpu_chain.py::test_plan_fused_equals_the_step_by_step_loop with the term in the guide; the term moved the plan."""
    from helpers import product_guide
    ds, dm, noise, starts, goals, kw = _plan_setup()
    pg, _ = _guide("R3", 64, 3, "full")
    hc = {0: starts[0], 63: goals[0]}
    fused, _ = dm.plan(hc, B, 64, noise=noise, return_chain=False, guide=pg, **kw)
    loop = dm.run_inference(None, hc, n_samples=B, horizon=64, fused=False, noise=noise, guide=pg, **kw)
    assert fused.shape == (B, 64, 6) and bool(torch.isfinite(fused).all())
    assert torch.equal(fused, loop)
    without, _ = dm.plan(hc, B, 64, noise=noise, return_chain=False, guide=product_guide(ds, *W).cuda(), **kw)
    assert not torch.equal(without, fused)


def test_scene_batch_equals_single_scene_launches_with_the_term():
    """Two scenes x 2 trajectories of R3 in one guide launch == the two single-scene launches, bit for bit, the term in every guide."""
    import mpd_public_amd as m
    ds = _case("R3", 64)[0]
    sets = scene_object_sets(3)
    scenes = m.PlanningScenes(ds.task, [sets[2], sets[1]])
    soc, npc = [1, 0], N_PER_CONTEXT
    x = chain_trajs(3, 2 * npc, 64, "chain/scenes", probes=probe_configs("R3", ds)).cuda()
    tilt = tr.MAX_TILT["R3", 64, 3]
    pg, _ = _guide("R3", 64, 3, "full")
    got = pg.with_scenes(scenes, soc, npc).cuda()(x)
    singles = [tr.product_guide_tool(scene_dataset(ds, scenes, s), 3, tilt, "full", *W)[0].cuda() for s in range(2)]
    ref = [singles[s](x[c * npc:(c + 1) * npc]) for c, s in enumerate(soc)]
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    for c in range(2):
        assert torch.equal(got[c * npc:(c + 1) * npc], ref[c]), c
    # the term reaches the scene launch: the same batch through a scene guide without it differs
    from helpers import product_guide
    assert not torch.equal(got, product_guide(ds, *W).with_scenes(scenes, soc, npc).cuda()(x))


# ---------------------------------------------------------------------------------------------------------------- 11. entry
def test_experiment_with_a_tool_axis():
    import mpd_public_amd as m
    from mpd_public_amd.inference import experiment
    rob = m.RobotChain.panda()
    res = experiment(model_id="EnvSpheres3D-RobotPanda", robot=rob, tool_axis=dict(max_tilt=0.3), n_samples=B,
                     model_args=dict(n_diffusion_steps=5, variance_schedule="cosine"), results_dir=None)
    assert {"tool_tilt_max", "fraction_within_tilt", "trajs_iters", "fraction_free_trajs", "t_total"} <= set(res)
    assert res["tool_tilt_max"].shape == (B,) and bool(torch.isfinite(res["tool_tilt_max"]).all()) and 0.0 <= res["fraction_within_tilt"] <= 1.0
    final = res["trajs_iters"][-1]
    assert final.shape == (B, 64, 14) and bool(torch.isfinite(final).all())
    # start and goal satisfy the constraint: the last frame's z against the world's z, float64, within max_tilt + the IK's rot_tol
    for q in (final[0, 0, :7], final[0, -1, :7]):
        _p, R = rob.fk(q.cpu().double().numpy())
        assert math.acos(min(1.0, max(-1.0, float(R[2, 2])))) <= 0.3 + 1e-3
    assert "tool_tilt_max" not in experiment(model_id="EnvSpheres3D-RobotPanda", robot=rob, n_samples=B, model_args=dict(n_diffusion_steps=5, variance_schedule="cosine"),
                                             results_dir=None)
    with pytest.raises(ValueError, match=r"RobotChain\.panda\(\)"):
        experiment(model_id="EnvSpheres3D-RobotPanda", tool_axis=dict(max_tilt=0.3), n_samples=B, model_args=dict(n_diffusion_steps=5, variance_schedule="cosine"),
                   results_dir=None)


def test_the_library_refuses_a_bad_tool_block():
    """The host checks of include/mpdx.h surface as Python exceptions naming the member; the baseline planners and the grid bake refuse the term."""
    from mpd_public_amd import _lib
    ds, desc, x = _case("R3", 64)
    D = ds.state_dim
    pg, _ = _guide("R3", 64, 3, "full")
    good = pg.device_params("cuda")
    xg = x.cuda()
    lib, st = _lib.load(), _lib.current_stream()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty_like(xg)

    def step(gp):
        _lib.check(lib.mpdx_guide_step(C.byref(gp), xg.data_ptr(), out.data_ptr(), None, None, flag.data_ptr(), None, B, B, 64, D, st), "mpdx_guide_step")

    def edited(**kw):
        gp = _lib.GuideParams.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                for j in range(3):
                    getattr(gp, k)[j] = v[j]
            else:
                setattr(gp, k, v)
        return gp

    step(edited())
    for kw, member in [(dict(tool_frame=4), "tool_frame"), (dict(tool_frame=-1), "tool_frame"), (dict(tool_axis=(0.0, 0.0, 1.01)), "tool_axis"),
                       (dict(tool_axis=(float("nan"), 0.0, 1.0)), "tool_axis"), (dict(tool_world=(0.0, 0.0, 0.0)), "tool_world"),
                       (dict(tool_world=(float("inf"), 0.0, 0.0)), "tool_world"), (dict(tool_cos_min=1.5), "tool_cos_min"), (dict(tool_cos_min=-1.5), "tool_cos_min"),
                       (dict(tool_cos_min=float("nan")), "tool_cos_min"), (dict(tool_weight=float("inf")), "tool_weight"), (dict(tool_weight=float("nan")), "tool_weight")]:
        with pytest.raises(RuntimeError, match=member):
            step(edited(**kw))
    with pytest.raises(RuntimeError, match=r"RobotChain\.panda\(\)"):
        step(edited(robot=_lib.ROBOT_PANDA))
    # the metrics entry point needs the term; the planners and the bake refuse it
    o2 = torch.empty((B, 2), device="cuda")
    with pytest.raises(RuntimeError, match="tool_frame"):
        _lib.check(lib.mpdx_traj_tool_metrics(C.byref(edited(tool_frame=0)), xg.data_ptr(), o2.data_ptr(), None, 64, B, 64, D, st), "mpdx_traj_tool_metrics")
    buf = torch.zeros(4096, device="cuda")
    ibuf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    gopts = _lib.GpmpOpts(1.0, 10.0, 0.1, 1e-6, 1e6, 1.0, 1)
    with pytest.raises(RuntimeError, match="tool_frame"):
        _lib.check(lib.mpdx_gpmp_step(C.byref(good), C.byref(gopts), xg.data_ptr(), out.data_ptr(), buf.data_ptr(), B, 64, D, 1, st), "mpdx_gpmp_step")
    ropts = _lib.RrtOpts()
    ropts.step, ropts.max_nodes, ropts.max_iters, ropts.max_connect_steps, ropts.n_edge_checks = 0.1, 16, 4, 4, 8
    with pytest.raises(RuntimeError, match="tool_frame"):
        _lib.check(lib.mpdx_rrt_connect(C.byref(good), C.byref(ropts), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ibuf.data_ptr(), ibuf.data_ptr(), ibuf.data_ptr(),
                                        ibuf.data_ptr(), 1, st), "mpdx_rrt_connect")
    with pytest.raises(RuntimeError, match="tool_frame"):
        _lib.check(lib.mpdx_rrt_paths(C.byref(good), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ibuf.data_ptr(), ibuf.data_ptr(), buf.data_ptr(), None, 1, 16, 8,
                                      0.1, 8, 1, st), "mpdx_rrt_paths")
    n3, o3 = (C.c_int * 3)(4, 4, 4), (C.c_float * 3)(0.0, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="tool_frame"):
        _lib.check(lib.mpdx_sdf_grid_bake(C.byref(good), 1, buf.data_ptr(), None, C.byref(n3), C.byref(o3), 0.1, st), "mpdx_sdf_grid_bake")
