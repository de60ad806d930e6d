"""GPU tests of the cost values and clearances (mpdx_traj_costs, csrc/costs.hpp; PlanningTask.trajectory_costs, PlanningScenes.trajectory_costs,
GuideManagerTrajectoriesWithVelocity.costs, experiment(report_costs=True)) against the fp64 oracle composites.

The allowance of every comparison comes from tests/cost_ref.py::yardstick: 8 x the error of the torch-fp32 oracle against the fp64 oracle on the same
inputs, per term, plus n_factors_active x 2^-22 x max(1, largest |coordinate|) - never from the kernel's output.  Every comparison prints its largest
error beside the allowance before it asserts.  The conditions on the inputs (every slot reached, both classes in the flag batches) are asserted from the
reference alone in tests/test_cost_cpu.py.
"""
import pytest
import torch

import cost_ref as cr
import guide_ref as gr

pytestmark = pytest.mark.gpu

KW = dict(return_clearance=True, return_point_costs=True)


def _bit_equal(a, b, what):
    for key in ("terms", "total", "clearance", "point_costs"):
        x, y = getattr(a, key), getattr(b, key)
        assert (x is None) == (y is None), (what, key)
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y), f"{what}: {key} differs, max |diff| = {float((x - y).abs().max()):.3e}"


def _rows(d, sl):
    return {k: (v[sl] if torch.is_tensor(v) and v.dim() > 0 and k in ("terms", "total", "clearance", "point_costs") else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------------------------ 1. terms against fp64
@pytest.mark.parametrize("robot_id,H,n_points", cr.TERM_CASES, ids=cr.TERM_IDS)
def test_terms_clearance_and_point_costs_vs_fp64(robot_id, H, n_points):
    c, og, c64, c32, xu = cr.term_case(robot_id, H)
    ds = c["ds"]
    comp = cr.product_composite(ds)
    names = gr.term_names(ds)
    for N in [n_points] + ([H] if H in (8, 24) else []):       # (n_points == H: the supports themselves)
        ref, allow, _ = cr.yardstick(c64, c32, xu, N)
        got = ds.task.trajectory_costs(xu.cuda(), comp, n_points=N, **KW)
        assert got.names == names and got.point_costs.shape == (xu.shape[0], N, len(names) - 1)
        cr.compare(got, ref, allow, f"{robot_id} H={H} N={N} B={xu.shape[0]}", names)
        for nm in gr.ZERO_RUNS.get(robot_id, ()):             # a field no trajectory comes near: exactly zero, as in the reference
            k = names.index(nm)
            assert not ref["terms"][:, k].any() and not got.terms[:, k].any(), nm
        one = ds.task.trajectory_costs(xu[:1].cuda(), comp, n_points=N, **KW)        # a launch with B = 1
        cr.compare(one, _rows(ref, slice(0, 1)), _rows(allow, slice(0, 1)), f"{robot_id} H={H} N={N} B=1", names)
        assert torch.equal(one.terms, got.terms[:1]) and torch.equal(one.clearance, got.clearance[:1])
    assert torch.equal(got.min_clearance, got.clearance.amin(-1))
    assert torch.allclose(got.total, got.terms @ got.weights)


# ------------------------------------------------------------------------------------------------------------------------ 2. grid fields
@pytest.mark.parametrize("case,mode", cr.GRID_CASES, ids=[f"{c}-{m}" for c, m in cr.GRID_CASES])
def test_grid_field_terms_vs_fp64_with_clamped_points(case, mode):
    import grid_edges_ref as ge
    from grid_ref import GridField
    prim, gds = cr.grid_dataset(case, mode)
    g = gds.task.df_collision_objects.grid
    sdf, grad = g.node_values("cuda")             # the device bake's node values: the lookup is what is compared
    field = GridField(sdf.cpu(), g.origin, g.cell, g.mode, None if grad is None else grad.cpu())
    og, c64, c32 = cr.grid_oracles(prim, field)
    xu = cr.unnormalised32(og, ge.trajs(case))
    ref, allow, _ = cr.yardstick(c64, c32, xu, 128)
    rob = c64.cost_l[0].robot
    clamped = ge.clamped_points(field, rob.link_points(ref["xi"][..., : rob.q_dim]))
    k = [f.name for f in prim.task.get_collision_fields()].index("objects")
    print(f"{case} {mode}: grid {g.shape}, {int(clamped.any(-1).sum())} of {clamped[..., 0].numel()} link points outside the box; grid term up to "
          f"{float(ref['terms'][:, k].max()):.3f}")
    assert bool(clamped.any()) and bool((~clamped.any(-1)).any()) and float(ref["terms"][:, k].max()) > 0
    names = [f.name for f in gds.task.get_collision_fields()] + ["gp"]
    got = gds.task.trajectory_costs(xu.cuda(), cr.product_composite(gds), n_points=128, **KW)
    cr.compare(got, ref, allow, f"grid {case} {mode}", names)


# ------------------------------------------------------------------------------------------------------------------------ 3. a moving field
@pytest.mark.parametrize("name", ["pm2-H64", "panda-H64"])
def test_moving_field_vs_fp64_and_zero_track_equals_static(name):
    import moving_ref as mr
    mc = mr.case(name)
    ds = mc["ds"]
    c32 = mr.oracle(ds, dtype=torch.float32)[1]
    xu = cr.unnormalised32(mc["og"], mc["x"])
    ref, allow, _ = cr.yardstick(mc["comp"], c32, xu, 128)
    names = [f.name for f in ds.task.get_collision_fields()] + ["gp"]
    k = names.index("moving_objects")
    assert float(ref["terms"][:, k].max()) > 0
    got = ds.task.trajectory_costs(xu.cuda(), mr.product(ds).cost, n_points=128, **KW)
    cr.compare(got, ref, allow, f"moving {name}", names)
    zero, static = mr.dataset(name, track="zero"), mr.dataset(name, track=None)
    a = zero.task.trajectory_costs(xu.cuda(), mr.product(zero).cost, n_points=128, **KW)
    b = static.task.trajectory_costs(xu.cuda(), mr.product(static).cost, n_points=128, **KW)
    assert zero.task.has_tracks and not static.task.has_tracks
    _bit_equal(a, b, f"{name}: zero track against the static block")
    assert not torch.equal(a.terms[:, k], got.terms[:, k])          # (the bent track is in use)
    with pytest.raises(ValueError):                                  # H against the track, before any device work
        ds.task.trajectory_costs(xu[:, :32].cuda(), mr.product(ds).cost)


# ------------------------------------------------------------------------------------------------------------------------ 4. scenes
@pytest.mark.parametrize("robot_id", ["RobotPointMass", "chain:R3"])
def test_every_context_equals_the_single_scene_call_of_its_scene(robot_id):
    import mpd_public_amd as m
    import scene_ref
    c, og, _, _, xu = cr.term_case(robot_id, 64)
    ds = c["ds"]
    sets = scene_ref.scene_object_sets(ds.env.dim)
    scenes = m.PlanningScenes(ds.task, [sets[2], sets[1]])
    soc, npc = [1, 0], 3
    xg = xu[:6].cuda()
    got = scenes.trajectory_costs(xg, cr.product_composite(ds), soc, npc, n_points=128, **KW)
    assert got.terms.shape == (6, len(gr.term_names(ds)))
    for ctx, s in enumerate(soc):
        d = scene_ref.scene_dataset(ds, scenes, s)
        one = d.task.trajectory_costs(xg[ctx * npc:(ctx + 1) * npc], cr.product_composite(d), n_points=128, **KW)
        sl = slice(ctx * npc, (ctx + 1) * npc)
        assert torch.equal(got.terms[sl], one.terms) and torch.equal(got.clearance[sl], one.clearance) and torch.equal(got.point_costs[sl], one.point_costs), (ctx, s)
    k = gr.term_names(ds).index("extra_objects")
    assert not torch.equal(got.terms[:3, k], got.terms[3:, k]) and float(got.terms[:, k].max()) > 0      # (the scenes differ and are reached)
    with pytest.raises(ValueError):
        scenes.trajectory_costs(xg, cr.product_composite(ds), [0, 2], npc)


# ------------------------------------------------------------------------------------------------------------------------ 5. the tool-axis term
@pytest.mark.parametrize("name,frame", [("R3", 3), ("R3", 2), ("Panda", 7)], ids=["R3-f3", "R3-f2-middle", "Panda-f7"])
def test_tool_axis_slot_and_point_column_vs_fp64(name, frame):
    import chain_ref
    import tool_ref as tr
    c, og, _, _, xu = cr.term_case(gr.CHAIN + name, 64)
    ds, desc, tilt = c["ds"], chain_ref.description(name), tr.MAX_TILT[(name, 64, frame)]
    comps = [tr.oracle_guide_tool(ds, desc, tr.ToolAxisRef(desc, frame, tilt, dtype=dt), "full")[1] for dt in (torch.float64, torch.float32)]
    ref, allow, _ = cr.yardstick(comps[0], comps[1], xu, 128)
    pg, _tool = tr.product_guide_tool(ds, frame, tilt, "full")
    names = [f.name for f in ds.task.get_collision_fields()] + ["tool_axis", "gp"]
    k = names.index("tool_axis")
    share = float((ref["point_costs"][..., -1] > 0).double().mean())
    print(f"tool {name} frame {frame}: hinge active on {100 * share:.1f} % of the points; term up to {float(ref['terms'][:, k].max()):.3f}")
    assert 0.02 < share < 0.98
    got = ds.task.trajectory_costs(xu.cuda(), pg.cost, n_points=128, **KW)
    assert got.names == names and got.point_costs.shape[-1] == len(names) - 1
    cr.compare(got, ref, allow, f"tool {name} frame {frame}", names)
    alone = ds.task.trajectory_costs(xu.cuda(), _tool, n_points=128, return_point_costs=True)       # a single term, wrapped: the same bits
    assert alone.names == ["tool_axis"] and torch.equal(alone.terms[:, 0], got.terms[:, k]) and torch.equal(alone.point_costs[..., 0], got.point_costs[..., -1])


# ------------------------------------------------------------------------------------------------------------------------ 6. the GP prior
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("robot_id,H", [("RobotPointMass", 64), ("RobotPanda", 128)])
def test_gp_prior_half_factor_and_sigma(robot_id, H, half):
    import mpd_public_amd as m
    from oracle import costs as oc
    c, og, c64, c32, xu = cr.term_case(robot_id, H)
    ds = c["ds"]
    comps = [oc.CostComposite(cc.cost_l[-1].robot, 64, [oc.CostGPTrajectory(cc.cost_l[-1].robot, 64, 5.0 / H, sigma_gp=2.0, half_factor=half)], weights_cost_l=[1.0])
             for cc in (c64, c32)]
    ref, allow, _ = cr.yardstick(comps[0], comps[1], xu, H)
    term = m.CostGPTrajectory(ds.robot, H, 5.0 / H, sigma_gp=2.0, half_factor=half)
    got = ds.task.trajectory_costs(xu.cuda(), term)
    assert got.names == ["gp"] and got.clearance is None and got.point_costs is None and got.min_clearance is None
    cr.compare(got, ref, allow, f"gp {robot_id} H={H} half={half}", ["gp"])
    full = ds.task.trajectory_costs(xu.cuda(), cr.product_composite(ds))              # sigma 1, no half factor: 4 x (8 x) this value
    ratio = full.terms[:, -1] / got.terms[:, 0]
    assert torch.allclose(ratio, torch.full_like(ratio, 8.0 if half else 4.0), rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------ 7. determinism
def test_two_calls_give_the_same_bits():
    c, og, _, _, xu = cr.term_case("RobotPanda", 64)
    comp = cr.product_composite(c["ds"])
    a = c["ds"].task.trajectory_costs(xu.cuda(), comp, n_points=257, **KW)
    b = c["ds"].task.trajectory_costs(xu.cuda(), comp, n_points=257, **KW)
    _bit_equal(a, b, "two calls")
    assert torch.isfinite(a.terms).all() and torch.isfinite(a.clearance).all() and torch.isfinite(a.point_costs).all()


# ------------------------------------------------------------------------------------------------------------------------ 8. against the metrics kernel
@pytest.mark.parametrize("robot_id", cr.FLAG_CASES)
def test_clearance_sign_is_the_collision_flag_of_the_metrics_kernel(robot_id):
    ds, xu, slack = cr.flag_batch(robot_id)
    collides, decided = cr.flag_classes(slack)
    assert int((collides & decided).sum()) >= 3 and int((~collides & decided).sum()) >= 3 and float((~decided).double().mean()) <= 0.10
    comp = cr.product_composite(ds)
    n_coll = len(ds.task.get_collision_fields())
    tc = ds.task.trajectory_costs(xu.cuda(), comp, n_points=cr.N_FLAG, **KW)
    met, mask = ds.task.trajectory_metrics(xu.cuda(), n_check=cr.N_FLAG, return_mask=True)
    neg, hit = (tc.min_clearance < 0).cpu(), (met[:, 0] > 0).cpu()
    print(f"{robot_id}: {int(hit.sum())} of {hit.numel()} trajectories collide by the metrics kernel, {int(neg.sum())} have a negative clearance; "
          f"{int((~decided).sum())} undecided by the reference")
    assert torch.equal(neg[decided], hit[decided]) and torch.equal(hit[decided], collides[decided])
    # a point the metrics kernel flags penetrates some field by its link radius: its hinge at margin = radius + cutoff is at least the cutoff margin
    summed = tc.point_costs[..., :n_coll].sum(-1)
    cut = ds.task.obstacle_cutoff_margin
    assert bool(mask.any()) and float(summed[mask].min()) >= cut * (1 - 1e-5), float(summed[mask].min())
    # and the smallest clearance is the reference's largest slack, negated (a coarse guard: the per-field clearance is held to its allowance in the term tests)
    err = (tc.min_clearance.cpu().double() + slack.amax(-1)).abs()
    print(f"{robot_id}: min clearance against -max slack: max err {float(err.max()):.3e}")
    assert float(err.max()) < 1e-4, float(err.max())


# ------------------------------------------------------------------------------------------------------------------------ 9. the guide's own costs
@pytest.mark.parametrize("robot_id", ["RobotPointMass", "RobotPanda", "chain:R3"])
def test_guide_costs_equal_the_task_costs_of_the_unnormalised_trajectories(robot_id):
    ds = gr.cover_dataset(robot_id, 64, device="cuda")
    guide = gr.product_run(ds, dict(weights=cr.WEIGHTS, only=None, clip_grad=True, gp_half_factor=False))
    x = gr.case(robot_id, 64)["x"].cuda()
    a = guide.costs(x, **KW)
    b = ds.task.trajectory_costs(ds.unnormalize_trajectories(x), guide.cost, n_points=guide.num_interpolated_points_for_collision, **KW)
    _bit_equal(a, b, f"guide.costs {robot_id}")
    assert a.names == gr.term_names(ds) and a.weights.tolist() == pytest.approx([1e-2] * (len(a.names) - 1) + [1e-7])
    off = gr.product_run(ds, dict(weights=cr.WEIGHTS, only=None, clip_grad=True, gp_half_factor=False))
    off.interpolate_trajectories_for_collision = False            # interpolation off: the supports
    _bit_equal(off.costs(x, **KW), ds.task.trajectory_costs(ds.unnormalize_trajectories(x), off.cost, n_points=64, **KW), "guide.costs without interpolation")
    import mpd_public_amd as m
    from helpers import toy_cost
    with pytest.raises(NotImplementedError, match="callable"):
        m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost).costs(x)


def test_scene_bound_guide_costs_equal_the_scene_costs():
    import mpd_public_amd as m
    import scene_ref
    ds = gr.cover_dataset("RobotPointMass", 64, device="cuda")
    sets = scene_ref.scene_object_sets(ds.env.dim)
    scenes = m.PlanningScenes(ds.task, [sets[2], sets[1]])
    guide = gr.product_run(ds, dict(weights=cr.WEIGHTS, only=None, clip_grad=True, gp_half_factor=False)).with_scenes(scenes, [1, 0], 3)
    x = gr.case("RobotPointMass", 64)["x"][:6].cuda()
    a = guide.costs(x, **KW)
    b = scenes.trajectory_costs(ds.unnormalize_trajectories(x), guide.cost, [1, 0], 3, n_points=128, **KW)
    _bit_equal(a, b, "a scene-bound guide's costs")
    k = a.names.index("extra_objects")
    plain = gr.product_run(ds, dict(weights=cr.WEIGHTS, only=None, clip_grad=True, gp_half_factor=False)).costs(x)
    assert not torch.equal(a.terms[:, k], plain.terms[:, k]) and torch.equal(a.terms[:, -1], plain.terms[:, -1])     # the scenes' extras, the same GP prior
    with pytest.raises(ValueError, match="bound"):
        guide.costs(x[:4])


# ------------------------------------------------------------------------------------------------------------------------ 10. the entry
def test_experiment_reports_costs_only_when_asked(tmp_path):
    from mpd_public_amd.inference import experiment
    n = 6
    kw = dict(model_id="EnvSimple2D-RobotPointMass", planner_alg="mpd", n_samples=n, debug=True, seed=3, weight_grad_cost_collision=1e-1,
              model_args=dict(n_diffusion_steps=8, variance_schedule="cosine", unet_dim_mults_option=0))
    r = experiment(results_dir=str(tmp_path / "on"), report_costs=True, **kw)
    base = experiment(results_dir=str(tmp_path / "off"), **kw)
    new = {"cost_guide_trajs_final", "cost_guide_terms_trajs_final", "min_clearance_trajs_final"}
    assert set(r) - set(base) == new and set(base) - set(r) == set()
    assert r["cost_guide_trajs_final"].shape == (n,) and torch.isfinite(r["cost_guide_trajs_final"]).all()
    terms = r["cost_guide_terms_trajs_final"]
    assert terms["names"] == ["objects", "workspace", "extra_objects", "gp"] and terms["terms"].shape == (n, 4)
    assert torch.allclose(terms["terms"] @ terms["weights"], r["cost_guide_trajs_final"])
    assert r["min_clearance_trajs_final"].shape == (n,)
    assert torch.equal(r["trajs_iters"], base["trajs_iters"]) and r["idx_best_traj"] == base["idx_best_traj"]       # nothing on the plan path changes
