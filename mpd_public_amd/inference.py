"""experiment() - drop-in for scripts/inference/inference.py:34-352 (the planning entry).

Same keyword arguments and defaults, same result dictionary / pickle keys (including the reference's swapped
'cost_path_length_trajs_final_free' <-> 'cost_smoothness_trajs_final_free', inference.py:345-346).  Differences, all
forced by what the reference tree does not contain:
  * trained weights / args.yaml / dataset are Google-Drive downloads (README.md:69-72).  If `model_dir` holds
    `args.yaml` + `checkpoints/{ema_,}model_current_state_dict.pth` they are loaded (state-dict keys are identical);
    otherwise formula-defined synthetic weights are used and `model_id` picks env/robot by name.
  * `experiment_launcher` decorators are replaced by plain kwargs; rendering (inference.py:356-434) is out of scope.
"""
from __future__ import annotations

import os
import pickle
import time
from math import ceil

import torch

from . import synthetic as syn
from .datasets import TrajectoryDataset
from .diffusion_model import GaussianDiffusionModel
from .guides import GuideManagerTrajectoriesWithVelocity
from .planning import CostCollision, CostComposite, CostGPTrajectory, compute_path_length, compute_smoothness, compute_variance_waypoints
from .sample_functions import ddpm_sample_fn, guide_gradient_steps
from .temporal_unet import TemporalUnet, UNET_DIM_MULTS


def _synthetic_args():
    # launch_train_01.py:51-84 is the only record of trained hyper-parameters
    return dict(variance_schedule="exponential", n_diffusion_steps=25, predict_epsilon=True, unet_input_dim=32,
                unet_dim_mults_option=1, use_ema=True, include_velocity=True)


def _tool_axis_endpoints(task, dataset, cost, gen, seed, device, max_tries=100):
    """Start and goal configurations under a CostToolAxis: each is a task.ik_coll_free_q solution for a reachable target whose orientation satisfies
    the constraint - position and rotation of the frame at a random collision-free configuration, the rotation turned by the smallest rotation that
    takes the tool axis onto the world axis (tilt 0).  The goal is the solution nearest to the start among those farther than the dataset's
    threshold_start_goal_pos (the pattern of goal_ee_pos)."""
    import numpy as np
    robot = task.robot
    start = None
    for k in range(max_tries):
        q = task.random_coll_free_q(n_samples=1, device=device, generator=gen)[0]
        p, R = robot.fk(q.cpu().numpy(), frame=cost.frame)
        w, u = R @ cost.axis, cost.world_axis
        v, c = np.cross(w, u), float(w @ u)
        if c < -1.0 + 1e-9:          # exactly opposite: half a turn about any axis perpendicular to u
            e = np.eye(3)[int(np.argmin(np.abs(u)))]
            n = np.cross(u, e) / np.linalg.norm(np.cross(u, e))
            Rmin = 2.0 * np.outer(n, n) - np.eye(3)
        else:                        # Rodrigues, written in v = w x u (|v| = sin, c = cos)
            K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
            Rmin = np.eye(3) + K + K @ K / (1.0 + c)
        try:
            q_ik = task.ik_coll_free_q(torch.from_numpy(p).float(), torch.from_numpy(Rmin @ R).float(), n_samples=16, device=device, seed=seed + k, frame=cost.frame)
        except ValueError:
            continue
        if start is None:
            start = q_ik[0]
            continue
        dist = torch.linalg.norm(q_ik - start, dim=-1)
        far = dist > dataset.threshold_start_goal_pos
        if bool(far.any()):
            return start, q_ik[far][torch.argmin(dist[far])]
    raise ValueError("No pair of collision free configurations satisfies the tool-axis constraint")


N_SUPPORT_POINTS = 64   # the horizon of every shipped configuration (TrajectoryDataset's default)


def _moving_sphere_set(moving_sphere, env_id, n_support_points=N_SUPPORT_POINTS):
    """experiment(moving_sphere=(c0, c1, r)): the sphere at c0 as an ObjectSet on the straight track to c1."""
    import numpy as np
    from .planning import ObjectSet, make_env, _pad3
    dim = make_env(env_id).dim
    try:
        c0, c1, r = moving_sphere
        c0, c1, r = np.asarray(c0, np.float64).reshape(-1), np.asarray(c1, np.float64).reshape(-1), float(r)
    except (TypeError, ValueError):
        raise ValueError(f"moving_sphere takes (c0, c1, r): two centres and a radius, got {moving_sphere!r}") from None
    if c0.shape != (dim,) or c1.shape != (dim,) or not (np.isfinite(c0).all() and np.isfinite(c1).all()):
        raise ValueError(f"moving_sphere: c0 and c1 must be finite points of the {dim}-D workspace of {env_id}, got {c0.tolist()} and {c1.tolist()}")
    if not (r > 0 and np.isfinite(r)):
        raise ValueError(f"moving_sphere: the radius must be positive and finite, got {r!r}")
    z = ObjectSet.empty()
    return ObjectSet(_pad3(c0, dim), np.array([r], np.float32), z.box_centers, z.box_half).with_linear_motion(np.zeros(dim), c1 - c0, n_support_points)


def experiment(model_id: str = "EnvSpheres3D-RobotPanda", planner_alg: str = "mpd", use_guide_on_extra_objects_only: bool = False,
               n_samples: int = 50, start_guide_steps_fraction: float = 0.25, n_guide_steps: int = 5,
               n_diffusion_steps_without_noise: int = 5, weight_grad_cost_collision: float = 1e-2,
               weight_grad_cost_smoothness: float = 1e-7, factor_num_interpolated_points_for_collision: float = 1.5,
               trajectory_duration: float = 5.0, device: str = "cuda", debug: bool = True, render: bool = False, seed: int = 30,
               results_dir: str = "logs", model_dir: str = None, model_args: dict = None, sdf_grid_cell_size: float = None,
               sdf_grid_mode: str = "linear", robot=None, goal_ee_pos=None, goal_ee_rot=None, goal_ee_frame=None, tool_axis=None,
               weight_grad_cost_tool_axis: float = 1e-2, sdf_grid=None, moving_sphere=None, report_costs: bool = False, **kwargs):
    """report_costs (extension; False = the results are what they were): evaluate the guide's cost composite on the final trajectories
    (GuideManagerTrajectoriesWithVelocity.costs, mpdx_traj_costs) - the results gain `cost_guide_trajs_final` ([n_samples], the weighted total the guide
    optimised), `cost_guide_terms_trajs_final` (dict(names=, weights=, terms=[n_samples, n_terms] unweighted)) and `min_clearance_trajs_final` ([n_samples],
    the smallest distance less the link radius over every collision field; negative: it collides).  `idx_best_traj` keeps the reference's rule (path length
    plus smoothness).
    moving_sphere (extension; None = every obstacle is static, as before): (c0, c1, r) - one more sphere of radius r that moves at constant velocity
    from centre c0 at the first support point to c1 at the last (2 or 3 coordinates each, the workspace's).  It is a further collision field of the task
    (planning.PlanningTask(moving_objects=...)): its cost enters the composite as the extra objects' does, the guide pushes every support away from
    the sphere's position at that support's own time, and the reported figures (free / colliding trajectories, collision intensity) are time-aware.
    A task that is already full (the Panda: self, fixed, workspace, extra) gives the extras' place to the moving sphere.  Start and goal are drawn
    against the static fields.
    tool_axis (extension; None = no such term, as before): dict(frame=, axis=, world_axis=, max_tilt=) - the arguments of planning.CostToolAxis, every
    key optional - adds the tool-axis constraint to the guide with weight `weight_grad_cost_tool_axis` ("carry it upright": the frame's axis stays
    within max_tilt radians of the world axis along the whole trajectory).  A chain robot (the Panda as robot=RobotChain.panda()).  Start and goal are
    then task.ik_coll_free_q solutions for two reachable end-effector targets whose orientation satisfies the constraint exactly (the pose of a random
    collision-free configuration, turned by the smallest rotation that aligns the axis); the results gain `tool_tilt_max` ([n_samples], the largest
    tilt of each final trajectory in radians) and `fraction_within_tilt` (the share of final trajectories with no point beyond max_tilt).  The term
    acts in the guide only: it is no part of the prior's training, and the baseline planners of generate_trajectories do not honour it.
    goal_ee_pos / goal_ee_rot / goal_ee_frame (extension; None = a random goal configuration, as before): the goal as an end-effector target -
    the point [x, y, z] (and the [3, 3] orientation) the frame `goal_ee_frame` (default: the last) is to reach.  The goal configuration is then the
    task.ik_coll_free_q solution nearest to the start in joint space among those farther than the dataset's threshold_start_goal_pos; the results
    gain `goal_ee_pos` and `goal_ee_error` (|FK(goal) - target| in float64).  A chain robot or the Panda.
    robot (extension): a planning.RobotChain that replaces the robot named in `model_id` (the environment is still taken from it).
    sdf_grid_cell_size / sdf_grid_mode (extension): None (default) keeps the primitive tables; a cell size makes the task's FIXED objects a
    signed-distance grid baked on the device ('linear' interpolation or 'nearest' node, planning.PlanningTask(sdf_grid=...)).
    sdf_grid (extension; None = as above): a grid_sdf.GridSDF - GridSDF.from_occupancy / from_points / from_mesh - passed through to the task as its objects field;
    not together with sdf_grid_cell_size."""
    torch.manual_seed(seed)
    if not torch.cuda.is_available():
        raise RuntimeError("mpd_public_amd.inference needs an AMD GPU (no CPU fallback)")
    tensor_args = {"device": torch.device(device), "dtype": torch.float32}
    if planner_alg not in ("mpd", "diffusion_prior_then_guide", "diffusion_prior"):
        raise NotImplementedError(planner_alg)
    run_prior_only = planner_alg == "diffusion_prior"
    run_prior_then_guidance = planner_alg == "diffusion_prior_then_guide"

    args = _synthetic_args()
    ckpt = None
    if model_dir is not None and os.path.exists(os.path.join(model_dir, "args.yaml")):
        import yaml
        with open(os.path.join(model_dir, "args.yaml")) as f:
            args.update(yaml.safe_load(f))
        ckpt = os.path.join(model_dir, "checkpoints", "ema_model_current_state_dict.pth" if args.get("use_ema") else "model_current_state_dict.pth")
    if model_args:
        args.update(model_args)
    env_id, robot_id = model_id.split("-")

    if sdf_grid is not None and sdf_grid_cell_size is not None:
        raise ValueError("sdf_grid (a GridSDF) and sdf_grid_cell_size (bake one from the primitives) exclude each other")
    if sdf_grid is None and sdf_grid_cell_size is not None:
        sdf_grid = dict(cell_size=float(sdf_grid_cell_size), mode=sdf_grid_mode)
    moving_objects, use_extra = None, True
    if moving_sphere is not None:
        moving_objects = _moving_sphere_set(moving_sphere, env_id)
        use_extra = not (robot is None and robot_id == "RobotPanda")   # (self + fixed + workspace + extra: full - the moving sphere takes the extras' place)
    dataset = TrajectoryDataset(env_id=env_id, robot_id=robot if robot is not None else robot_id, use_extra_objects=use_extra, obstacle_cutoff_margin=0.05,
                                include_velocity=args["include_velocity"], tensor_args=tensor_args, sdf_grid=sdf_grid, n_support_points=N_SUPPORT_POINTS,
                                moving_objects=moving_objects)
    n_support_points, robot, task = dataset.n_support_points, dataset.robot, dataset.task
    dt = trajectory_duration / n_support_points
    robot.dt = dt
    tool_cost = None
    if tool_axis is not None:   # (checked before the model is built: a robot that cannot take the term is refused at once)
        from .planning import CostToolAxis
        unknown = set(tool_axis) - {"frame", "axis", "world_axis", "max_tilt"}
        if unknown:
            raise ValueError(f"tool_axis takes frame, axis, world_axis, max_tilt (got {sorted(tool_axis)})")
        tool_cost = CostToolAxis(robot, n_support_points, tensor_args=tensor_args, **tool_axis)

    unet = TemporalUnet(state_dim=dataset.state_dim, n_support_points=n_support_points, unet_input_dim=args["unet_input_dim"],
                        dim_mults=UNET_DIM_MULTS[args["unet_dim_mults_option"]],
                        self_attention=bool(args.get("self_attention", False)))   # (the key of a run that built TemporalUnet(self_attention=True); absent: False)
    model = GaussianDiffusionModel(model=unet, variance_schedule=args["variance_schedule"], n_diffusion_steps=args["n_diffusion_steps"],
                                   predict_epsilon=args["predict_epsilon"])
    if ckpt is not None and os.path.exists(ckpt):
        model.load_state_dict(torch.load(ckpt, map_location="cpu"))
        # The reference derives the normaliser limits from the training dataset (normalization.py:92-93) and the obstacles /
        # link spheres from torch_robotics; neither travels with a checkpoint.  `model_dir/limits.yaml`
        # ({mins: [D], maxs: [D]}) supplies the limits; without it trained weights would be run against SYNTHETIC
        # normalisation - refuse unless the caller opts in.
        lim = os.path.join(model_dir, "limits.yaml")
        if os.path.exists(lim):
            import yaml
            with open(lim) as f:
                lm = yaml.safe_load(f)
            from .datasets import LimitsNormalizer, GaussianNormalizer, Identity
            if len(lm["mins"]) != dataset.state_dim or len(lm["maxs"]) != dataset.state_dim:
                raise ValueError(f"{lim}: expected {dataset.state_dim} mins/maxs")
            kind = lm.get("normalizer", "LimitsNormalizer")   # (written by train.py of this package; the limits are final: a Safe / Fixed one is a LimitsNormalizer here)
            if kind == "GaussianNormalizer":
                dataset.normalizer = GaussianNormalizer(lm["means"], lm["stds"], lm["mins"], lm["maxs"]).to(tensor_args["device"])
            elif kind == "Identity":
                dataset.normalizer = Identity(lm["mins"], lm["maxs"]).to(tensor_args["device"])
            else:
                dataset.normalizer = LimitsNormalizer(lm["mins"], lm["maxs"]).to(tensor_args["device"])
        elif not kwargs.get("allow_synthetic_limits", False):
            raise RuntimeError(f"{model_dir} holds trained weights but no limits.yaml: the normaliser limits (and the environment "
                               "geometry) of this package are synthetic stand-ins (DESIGN.md section 5) and would not match the "
                               "training data.  Provide model_dir/limits.yaml {mins, maxs} or pass allow_synthetic_limits=True.")
        else:
            import warnings
            warnings.warn("trained checkpoint combined with SYNTHETIC normaliser limits / environment geometry: plans and metrics "
                          "are not comparable with the reference's", RuntimeWarning)
    else:
        unet.load_state_dict(syn.synth_state_dict({k: tuple(v.shape) for k, v in unet.state_dict().items()}))
    model = model.to(tensor_args["device"]).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    model.manual_seed(seed)
    model.warmup(horizon=n_support_points, device=device)

    gen = torch.Generator(device=tensor_args["device"]).manual_seed(seed)
    start_state_pos = goal_state_pos = None
    for _ in range(100):
        q_free = task.random_coll_free_q(n_samples=2, device=tensor_args["device"], generator=gen)
        start_state_pos, goal_state_pos = q_free[0], q_free[1]
        if torch.linalg.norm(start_state_pos - goal_state_pos) > dataset.threshold_start_goal_pos:
            break
    if start_state_pos is None or goal_state_pos is None:
        raise ValueError("No collision free configuration was found")
    if tool_cost is not None:
        start_state_pos, goal_state_pos = _tool_axis_endpoints(task, dataset, tool_cost, gen, seed, tensor_args["device"])
    goal_ee_error = None
    if goal_ee_pos is not None:
        from .ik import chain_of
        ik_kw = {} if goal_ee_frame is None else dict(frame=int(goal_ee_frame))
        q_ik = task.ik_coll_free_q(goal_ee_pos, goal_ee_rot, n_samples=32, device=tensor_args["device"], seed=seed, **ik_kw)
        dist = torch.linalg.norm(q_ik - start_state_pos, dim=-1)
        far = dist > dataset.threshold_start_goal_pos
        if not bool(far.any()):
            raise ValueError("No collision free configuration reaches the target farther than threshold_start_goal_pos from the start")
        goal_state_pos = q_ik[far][torch.argmin(dist[far])]
        p_goal, _ = chain_of(robot).fk(goal_state_pos.cpu(), frame=goal_ee_frame)
        goal_ee_error = float(torch.linalg.norm(p_goal - torch.as_tensor(goal_ee_pos, dtype=torch.float64).reshape(3)))

    hard_conds = dataset.get_hard_conditions(torch.vstack((start_state_pos, goal_state_pos)), normalize=True)
    collision_fields = task.get_collision_fields_extra_objects() if use_guide_on_extra_objects_only else task.get_collision_fields()
    if use_guide_on_extra_objects_only and moving_objects is not None:   # (the moving sphere's cost enters the composite the way the extra objects' does)
        collision_fields = [f for f in collision_fields if f is not None] + task.get_collision_fields_moving_objects()
    cost_l = [CostCollision(robot, n_support_points, field=f, sigma_coll=1.0, tensor_args=tensor_args) for f in collision_fields]
    weights = [weight_grad_cost_collision] * len(cost_l)
    if tool_cost is not None:
        cost_l.append(tool_cost)
        weights.append(weight_grad_cost_tool_axis)
    cost_l.append(CostGPTrajectory(robot, n_support_points, dt, sigma_gp=1.0, tensor_args=tensor_args))
    weights.append(weight_grad_cost_smoothness)
    cost_composite = CostComposite(robot, n_support_points, cost_l, weights_cost_l=weights, tensor_args=tensor_args)
    guide = GuideManagerTrajectoriesWithVelocity(dataset, cost_composite, clip_grad=True, interpolate_trajectories_for_collision=True,
                                                 num_interpolated_points=ceil(n_support_points * factor_num_interpolated_points_for_collision),
                                                 tensor_args=tensor_args).to(tensor_args["device"])
    t_start_guide = ceil(start_guide_steps_fraction * model.n_diffusion_steps)
    sample_fn_kwargs = dict(guide=None if (run_prior_then_guidance or run_prior_only) else guide, n_guide_steps=n_guide_steps,
                            t_start_guide=t_start_guide, noise_std_extra_schedule_fn=lambda x: 0.5)

    t_cold = None
    if kwargs.get("warm_plan", False):
        # extension, OFF by default (so that `t_total` below covers what the reference's does: the first plan of the process, inference.py:248-259):
        # warm_plan=True runs one throwaway plan of the SAME shape in front of the timed one.  model.warmup() above mirrors the reference's (one U-Net
        # pass at batch 2); the first plan of a process additionally loads every kernel's code object, sizes the workspaces for n_samples, raises LDS
        # limits and uploads the guide's tables - 5 ... 60 ms (measured: 12.2 / 67 ms for the first plan against 7.3 / 6.6 ms for the next ones).
        # Both times are recorded (`t_total_cold` beside `t_total`); the noise stream is re-seeded: the timed plan is bit for bit the one an
        # un-warmed call would have produced.
        torch.cuda.synchronize()
        tc = time.perf_counter()
        model.run_inference(None, hard_conds, n_samples=n_samples, horizon=n_support_points, return_chain=True, sample_fn=ddpm_sample_fn,
                            **sample_fn_kwargs, n_diffusion_steps_without_noise=n_diffusion_steps_without_noise)
        torch.cuda.synchronize()
        t_cold = time.perf_counter() - tc
        model.manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trajs_normalized_iters = model.run_inference(None, hard_conds, n_samples=n_samples, horizon=n_support_points, return_chain=True,
                                                 sample_fn=ddpm_sample_fn, **sample_fn_kwargs,
                                                 n_diffusion_steps_without_noise=n_diffusion_steps_without_noise)
    torch.cuda.synchronize()
    t_total = time.perf_counter() - t0
    if debug:
        print(f"t_model_sampling: {t_total:.3f} sec")

    if run_prior_then_guidance:
        n_post = (t_start_guide + n_diffusion_steps_without_noise) * n_guide_steps
        hc_b = {k: v.reshape(1, -1).expand(n_samples, -1).contiguous() for k, v in hard_conds.items()}
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        trajs, post = trajs_normalized_iters[-1].clone(), []
        for _ in range(n_post):
            trajs = guide_gradient_steps(trajs, hard_conds=hc_b, guide=guide, n_guide_steps=1, unnormalize_data=False)
            post.append(trajs)
        trajs_normalized_iters = torch.cat((trajs_normalized_iters, torch.stack(post, dim=0)))
        torch.cuda.synchronize()
        t_total += time.perf_counter() - t1

    trajs_iters = dataset.unnormalize_trajectories(trajs_normalized_iters)
    trajs_final = trajs_iters[-1]
    trajs_final_coll, trajs_final_coll_idxs, trajs_final_free, trajs_final_free_idxs, _ = task.get_trajs_collision_and_free(trajs_final, return_indices=True)
    success_free_trajs = task.compute_success_free_trajs(trajs_final)
    fraction_free_trajs = task.compute_fraction_free_trajs(trajs_final)
    collision_intensity_trajs = task.compute_collision_intensity_trajs(trajs_final)
    if debug:
        print(f"success: {success_free_trajs}\npercentage free trajs: {fraction_free_trajs*100:.2f}\n"
              f"percentage collision intensity: {collision_intensity_trajs*100:.2f}")

    traj_final_free_best = idx_best_traj = cost_best_free_traj = cost_smoothness = cost_path_length = cost_all = None
    variance_waypoint_trajs_final_free = None
    if trajs_final_free is not None:
        cost_smoothness = compute_smoothness(trajs_final_free, robot)
        cost_path_length = compute_path_length(trajs_final_free, robot)
        cost_all = cost_path_length + cost_smoothness
        idx_best_traj = torch.argmin(cost_all).item()
        traj_final_free_best = trajs_final_free[idx_best_traj]
        cost_best_free_traj = torch.min(cost_all).item()
        variance_waypoint_trajs_final_free = compute_variance_waypoints(trajs_final_free, robot)
        if debug:
            print(f"cost smoothness: {cost_smoothness.mean():.4f}  cost path length: {cost_path_length.mean():.4f}  cost best: {cost_best_free_traj:.3f}")

    results_data_dict = {
        "trajs_iters": trajs_iters, "trajs_final_coll": trajs_final_coll, "trajs_final_coll_idxs": trajs_final_coll_idxs,
        "trajs_final_free": trajs_final_free, "trajs_final_free_idxs": trajs_final_free_idxs,
        "success_free_trajs": success_free_trajs, "fraction_free_trajs": fraction_free_trajs,
        "collision_intensity_trajs": collision_intensity_trajs, "idx_best_traj": idx_best_traj,
        "traj_final_free_best": traj_final_free_best, "cost_best_free_traj": cost_best_free_traj,
        "cost_path_length_trajs_final_free": cost_smoothness,   # sic: swapped in the reference (inference.py:345-346)
        "cost_smoothness_trajs_final_free": cost_path_length,
        "cost_all_trajs_final_free": cost_all, "variance_waypoint_trajs_final_free": variance_waypoint_trajs_final_free,
        "t_total": t_total,
    }
    if t_cold is not None:   # warm_plan=True: `t_total` above timed a warmed plan; the first plan of the process (what the reference's t_total covers) took this
        results_data_dict["t_total_cold"] = t_cold
    if goal_ee_pos is not None:
        results_data_dict["goal_ee_pos"] = torch.as_tensor(goal_ee_pos, dtype=torch.float32).reshape(3)
        results_data_dict["goal_ee_error"] = goal_ee_error
    if tool_cost is not None:
        tilt, n_bad = task.tool_axis_metrics(trajs_final, tool_cost)
        results_data_dict["tool_tilt_max"] = tilt
        results_data_dict["fraction_within_tilt"] = float((n_bad == 0).float().mean())
        if debug:
            print(f"tool axis: largest tilt {float(tilt.max()):.3f} rad (allowed {tool_cost.max_tilt:.3f}); within the tilt: {results_data_dict['fraction_within_tilt']*100:.2f} %")
    if report_costs:
        tc = guide.costs(trajs_normalized_iters[-1], return_clearance=True)
        results_data_dict["cost_guide_trajs_final"] = tc.total
        results_data_dict["cost_guide_terms_trajs_final"] = dict(names=list(tc.names), weights=tc.weights, terms=tc.terms)
        results_data_dict["min_clearance_trajs_final"] = tc.min_clearance
        if debug and idx_best_traj is not None:
            i_best = int(trajs_final_free_idxs[idx_best_traj])
            print(f"guide cost of the best free trajectory: {float(tc.total[i_best]):.4g}  (" + ", ".join(f"{n} {float(v):.4g}" for n, v in zip(tc.names, tc.terms[i_best]))
                  + ")" + (f"; clearance {float(tc.min_clearance[i_best]):.4f}" if tc.min_clearance is not None else ""))
    if results_dir:
        out_dir = os.path.join(results_dir, model_id, "results_inference", str(seed))
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "results_data_dict.pickle"), "wb") as handle:
            pickle.dump(results_data_dict, handle, protocol=pickle.HIGHEST_PROTOCOL)
    if render:
        raise NotImplementedError("rendering (inference.py:356-434: matplotlib videos + IsaacGym) is out of scope")
    return results_data_dict


def _mesh_grid_args(a: dict) -> dict:
    """--sdf_grid_mesh PATH of the command line: the mesh becomes a GridSDF over the task's workspace (GridSDF.from_mesh, at --sdf_grid_cell_size, in
    --sdf_grid_mode) and goes to experiment(sdf_grid=...); experiment's own sdf_grid_cell_size stays unset (it would bake the primitives)."""
    path = a.pop("sdf_grid_mesh")
    if path is None:
        return a
    if a["sdf_grid_cell_size"] is None:
        raise SystemExit("--sdf_grid_mesh needs --sdf_grid_cell_size")
    from .planning import GridSDF, make_env
    ws_min, ws_max = make_env(a["model_id"].split("-")[0]).limits
    a["sdf_grid"] = GridSDF.from_mesh(path, None, ws_min, ws_max, a["sdf_grid_cell_size"], mode=a["sdf_grid_mode"])
    a["sdf_grid_cell_size"] = None
    return a


def _depth_grid_args(a: dict) -> dict:
    """--sdf_grid_depth FILE.npz of the command line: depth [n, h, w] (metres, or uint16 millimetres), intrinsics [n, 4] (fx, fy, cx, cy) and
    world_from_cam [n, 4, 4] are fused into a GridSDF over the task's workspace (GridSDF.from_depth, at --sdf_grid_cell_size, in --sdf_grid_mode)
    that goes to experiment(sdf_grid=...), as _mesh_grid_args does with a mesh."""
    path = a.pop("sdf_grid_depth", None)
    if path is None:
        return a
    if a.get("sdf_grid") is not None:
        raise SystemExit("--sdf_grid_depth and --sdf_grid_mesh exclude each other")
    if a["sdf_grid_cell_size"] is None:
        raise SystemExit("--sdf_grid_depth needs --sdf_grid_cell_size")
    import numpy as np
    from .planning import GridSDF, make_env
    with np.load(path) as z:
        missing = [k for k in ("depth", "intrinsics", "world_from_cam") if k not in z]
        if missing:
            raise SystemExit(f"--sdf_grid_depth {path}: the archive lacks {', '.join(missing)} (depth [n, h, w], intrinsics [n, 4], world_from_cam [n, 4, 4])")
        depth, intrinsics, poses = z["depth"], z["intrinsics"], z["world_from_cam"]
    ws_min, ws_max = make_env(a["model_id"].split("-")[0]).limits
    a["sdf_grid"] = GridSDF.from_depth(list(depth), intrinsics, list(poses), ws_min, ws_max, a["sdf_grid_cell_size"], mode=a["sdf_grid_mode"],
                                       depth_scale=0.001 if depth.dtype == np.uint16 else 1.0)
    a["sdf_grid_cell_size"] = None
    return a


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_id", default="EnvSpheres3D-RobotPanda")
    ap.add_argument("--planner_alg", default="mpd")
    ap.add_argument("--n_samples", type=int, default=50)
    ap.add_argument("--seed", type=int, default=30)
    ap.add_argument("--results_dir", default="logs")
    ap.add_argument("--model_dir", default=None, help="a results directory of mpd_public_amd.train (args.yaml, limits.yaml, checkpoints/): plan with its trained weights")
    ap.add_argument("--n_diffusion_steps_without_noise", type=int, default=5)
    ap.add_argument("--sdf_grid_cell_size", type=float, default=None, help="fixed objects as a signed-distance grid of this cell size (default: primitive tables)")
    ap.add_argument("--sdf_grid_mode", default="linear", choices=["linear", "nearest"])
    ap.add_argument("--sdf_grid_mesh", default=None, metavar="PATH",
                    help="fixed objects from a triangle mesh (.obj / .stl, closed, in the workspace frame) as a signed-distance grid; needs --sdf_grid_cell_size")
    ap.add_argument("--sdf_grid_depth", default=None, metavar="NPZ",
                    help="the obstacles from depth frames (an .npz of depth [n, h, w] in metres or uint16 millimetres, intrinsics [n, 4] = fx, fy, cx, cy, "
                         "world_from_cam [n, 4, 4]; OpenCV camera frame) fused into a signed-distance grid; needs --sdf_grid_cell_size")
    ap.add_argument("--goal_ee_pos", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="plan to this end-effector position (inverse kinematics) instead of a random goal configuration")
    ap.add_argument("--tool_upright", type=float, default=None, metavar="MAX_TILT_DEG",
                    help="carry the tool upright: the last frame's z axis stays within this many degrees of the world's z (a chain robot; RobotPanda runs as RobotChain.panda())")
    ap.add_argument("--moving_sphere", type=float, nargs="+", default=None, metavar="V",
                    help="one more sphere that moves at constant velocity during the plan: the coordinates of its centre at the first support point, then those "
                         "at the last, then its radius (5 numbers in a 2-D workspace, 7 in 3-D)")
    ap.add_argument("--report_costs", action="store_true",
                    help="also report the guide's cost composite on the final trajectories: the weighted total, every term, and the clearance to the obstacles")
    a = _depth_grid_args(_mesh_grid_args(vars(ap.parse_args())))
    ms = a.pop("moving_sphere")
    if ms is not None:
        if len(ms) not in (5, 7):
            raise SystemExit("--moving_sphere takes the coordinates of c0, then those of c1, then the radius: 5 numbers (2-D) or 7 (3-D)")
        k = len(ms) // 2
        a["moving_sphere"] = (ms[:k], ms[k: 2 * k], ms[-1])
    upright = a.pop("tool_upright")
    if upright is not None:
        import math
        from .planning import RobotChain
        if not a["model_id"].endswith("-RobotPanda"):
            raise SystemExit("--tool_upright needs a chain robot: on the command line that is the Panda (model_id ...-RobotPanda)")
        a.update(robot=RobotChain.panda(), tool_axis=dict(max_tilt=math.radians(upright)))
    experiment(**a)
