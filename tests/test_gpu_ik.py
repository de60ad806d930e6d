"""GPU tests of the chain-robot inverse kinematics (csrc/ik.hpp: ik_solve_kernel behind mpdx_ik_solve; mpd_public_amd.solve_ik,
PlanningTask.ik_coll_free_q, experiment(goal_ee_pos=...)) against the torch reference of tests/ik_ref.py.

1. one step      q_out - q_init of one iteration (adaptive off, lambda 1e-2, caller seeds) against the fp64 reference step.  Yardstick: the
                 reference's own fp32 step against fp64, worst case per robot; the kernel may deviate from fp64 by 4 x that (summation order,
                 sinf / cosf, Cholesky ordering), floor 16 * 2^-24 * max(1, |q|inf).
                 Measured on the MI355X (max |step - fp64 step| over last + intermediate frame, position + pose, (n, R) in (1, 1), (3, 64), (1, 65), (3, 65)):
                 one step R1: reference fp32 vs fp64 2.277e-07; kernel vs fp64 2.126e-07; bound 2.859e-06
                 one step R3: reference fp32 vs fp64 2.199e-06; kernel vs fp64 1.370e-06; bound 8.796e-06
                 one step R8: reference fp32 vs fp64 2.294e-05; kernel vs fp64 3.577e-05; bound 9.175e-05
                 one step Panda: reference fp32 vs fp64 1.307e-05; kernel vs fp64 9.849e-06; bound 5.228e-05
                 one step R8[:2]: reference fp32 vs fp64 5.830e-07; kernel vs fp64 9.205e-07; bound 2.479e-06
                 one step R8[:4]: reference fp32 vs fp64 2.897e-06; kernel vs fp64 3.634e-06; bound 1.159e-05
                 one step R8[:5]: reference fp32 vs fp64 4.996e-06; kernel vs fp64 5.121e-06; bound 1.998e-05
                 one step R8[:6]: reference fp32 vs fp64 1.566e-05; kernel vs fp64 1.229e-05; bound 6.264e-05
                 (R8[:k]: the 8-joint robot cut after k joints; with R1, R3, Panda and R8 every instantiation, 1 ... 8 joints, runs)
2. independence  a target solved alone is bit-equal to the same target inside a batch of 3
3. seeds         max_iters = 0, q_init = NULL: the seeds are fmaf(hi - lo, u, lo) of the Philox uniforms of tests/philox_ref.py to one float32 ulp
                 of the span hi - lo (with hi - lo taken in float32 as the kernel takes it, what is left is u's rounding, at most span * 2^-25 =
                 1/2 ulp of the span, and the fma's own, at most 1/2 ulp of the result, which is smaller than the span)
4. convergence   the cases of ik_ref.convergence_case (their reference-only side is tests/test_ik_cpu.py)
5. interface     task.ik_coll_free_q and experiment(goal_ee_pos=...)"""
import functools

import numpy as np
import pytest
import torch

import ik_ref
import philox_ref
from chain_ref import description, product_robot

pytestmark = pytest.mark.gpu

OFFSET = (0.05, -0.02, 0.11)
SHAPES = [(1, 1), (3, 64), (1, 65), (3, 65)]


_fk_slack = ik_ref.fk_slack   # twice the largest |FK_fp32 - FK_fp64| the reference shows on the configurations


# ---------------------------------------------------------------------------------------------------------------- 1. one step
@functools.lru_cache(maxsize=None)
def _one_step_inputs(name):
    """[(frame, pose, n, R, q0 [n, R, qd] float32, tpos [n, 3] float32, trot [n, 3, 3] float32)] of a robot, from a fixed generator"""
    rng = np.random.default_rng(77 + len(name))
    qd = len(description(name)["joints"])
    out = []
    for frame in sorted({qd, max(1, qd // 2)}):
        for pose in (False, True):
            for n, R in SHAPES:
                q0 = ik_ref.random_q(name, (n, R), rng)
                tpos, trot = ik_ref.target_of(name, ik_ref.random_q(name, (n,), rng), frame=frame, offset=OFFSET)
                out.append((frame, pose, n, R, q0, tpos.float(), trot.float()))
    return out


@pytest.mark.parametrize("name", ["R1", "R3", "R8", "Panda", "R8[:2]", "R8[:4]", "R8[:5]", "R8[:6]"])   # every instantiation: 1 ... 8 joints
def test_one_step_against_the_fp64_reference(name):
    import mpd_public_amd as m
    rob = product_robot(name)
    yard = got = qmax = 0.0
    for frame, pose, n, R, q0, tpos, trot in _one_step_inputs(name):
        kw = dict(frame=frame, offset=OFFSET, rot_weight=ik_ref.ROT_WEIGHT if pose else 0.0, adaptive=False, lambda_init=1e-2)
        r64, r32 = ik_ref.IKRef(name, torch.float64, **kw), ik_ref.IKRef(name, torch.float32, **kw)
        _, qc64, _, _ = r64.step(q0.double(), 1e-2, tpos.double()[:, None, :], trot.double()[:, None, :, :])
        _, qc32, _, _ = r32.step(q0, 1e-2, tpos[:, None, :], trot[:, None, :, :])
        step64 = qc64 - q0.double()
        yard = max(yard, float((qc32.double() - q0.double() - step64).abs().max()))
        res = m.solve_ik(rob, tpos, trot if pose else None, frame=frame, offset=OFFSET, n_restarts=R, q_init=q0, max_iters=1, adaptive=False, lambda_init=1e-2,
                         rot_weight=ik_ref.ROT_WEIGHT, pos_tol=1e-9, rot_tol=1e-9)   # (tolerances no seed meets: every restart takes the step)
        q = res.q.cpu()
        assert q.shape == (n, R, rob.q_dim) and bool(torch.isfinite(q).all())
        assert bool((res.iters.cpu() == 1).all()) and not bool(res.converged.any())
        assert torch.equal(q[..., frame:], q0[..., frame:]), (name, frame, pose, n, R)       # joints above the frame: bit-unchanged
        assert float(step64[..., :frame].abs().max()) > 1e-3                                      # the step is not trivially zero
        got = max(got, float((q.double() - q0.double() - step64).abs().max()))
        qmax = max(qmax, float(q0.abs().max()))
    bound = max(4.0 * yard, 16 * 2.0 ** -24 * max(1.0, qmax))
    print(f"one step {name}: reference fp32 vs fp64 {yard:.3e}; kernel vs fp64 {got:.3e}; bound {bound:.3e}")
    assert got <= bound, (name, got, yard, bound)


# ---------------------------------------------------------------------------------------------------------------- 2. batch independence
@pytest.mark.parametrize("name,pose", [("R3", False), ("Panda", True)])
def test_a_target_alone_equals_the_target_in_a_batch(name, pose):
    import mpd_public_amd as m
    rob = product_robot(name)
    rng = np.random.default_rng(5)
    n, R = 3, 65
    q0 = ik_ref.random_q(name, (n, R), rng)
    tpos, trot = ik_ref.target_of(name, ik_ref.random_q(name, (n,), rng, margin=0.3), offset=OFFSET)
    tpos, trot = tpos.float(), trot.float()
    kw = dict(offset=OFFSET, n_restarts=R, max_iters=100)
    full = m.solve_ik(rob, tpos, trot if pose else None, q_init=q0, **kw)
    assert bool(full.converged.any()) and int(full.iters.max()) > 1
    for i in range(n):
        one = m.solve_ik(rob, tpos[i:i + 1], trot[i:i + 1] if pose else None, q_init=q0[i:i + 1], **kw)
        for a, b in ((one.q, full.q), (one.pos_err, full.pos_err), (one.rot_err, full.rot_err), (one.converged, full.converged), (one.iters, full.iters)):
            assert torch.equal(a[0], b[i]), (name, i)


# ---------------------------------------------------------------------------------------------------------------- 3. seeds
@pytest.mark.parametrize("name", ["R3", "R8", "R8[:5]", "R8[:6]"])   # 5 and 6 joints: the second Philox block part-filled
def test_philox_seeds(name):
    import mpd_public_amd as m
    rob = product_robot(name)
    n, R, seed, qd = 3, 65, 0x1234567890ABCDEF, rob.q_dim
    tpos = torch.zeros((n, 3))
    a = m.solve_ik(rob, tpos, n_restarts=R, max_iters=0, seed=seed)
    b = m.solve_ik(rob, tpos, n_restarts=R, max_iters=0, seed=seed)
    c = m.solve_ik(rob, tpos, n_restarts=R, max_iters=0, seed=seed + 1)
    assert torch.equal(a.q, b.q) and torch.equal(a.pos_err, b.pos_err) and not torch.equal(a.q, c.q)
    assert not bool(a.iters.any()) and a.q.shape == (n, R, qd)
    lo, hi = (np.asarray(v, np.float32) for v in rob.q_limits)
    span = (hi - lo).astype(np.float32)
    i, r = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(R, dtype=np.uint64), indexing="ij")
    u = np.concatenate([philox_ref.uniform4(seed, (i << np.uint64(32)) | (np.uint64(2) * r + np.uint64(k))) for k in (0, 1)], -1)[..., :qd]
    want = lo.astype(np.float64) + span.astype(np.float64) * u
    got = a.q.cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= np.spacing(span)).all(), np.abs(got - want).max()
    assert (got >= lo).all() and (got <= hi).all()
    # the errors of the untouched seeds are those of the fp64 FK
    perr = (ik_ref.IKRef(name, torch.float64).pose(a.q.cpu().double())[0]).norm(dim=-1)
    assert float((a.pos_err.cpu().double() - perr).abs().max()) <= _fk_slack(name, a.q)


def test_caller_seeds_are_clamped_into_the_limits():
    """max_iters = 0: seeds outside the limits come back clamped, seeds inside bit for bit"""
    import mpd_public_amd as m
    rob = product_robot("R3")
    lo, hi = (torch.tensor(np.asarray(v, np.float32)) for v in rob.q_limits)
    q0 = ik_ref.random_q("R3", (2, 65), np.random.default_rng(9))
    q0[0, 3], q0[1, 64] = hi + 0.5, lo - 2.0
    res = m.solve_ik(rob, torch.zeros((2, 3)), n_restarts=65, q_init=q0, max_iters=0)
    assert torch.equal(res.q.cpu(), torch.minimum(torch.maximum(q0, lo), hi)) and not bool(res.iters.any())


# ---------------------------------------------------------------------------------------------------------------- 4. convergence
@pytest.mark.parametrize("pose", [False, True], ids=["position", "pose"])
@pytest.mark.parametrize("name", ik_ref.CONV_ROBOTS)
def test_convergence(name, pose):
    import mpd_public_amd as m
    c = ik_ref.convergence_case(name, pose)
    rob = product_robot(name)
    tpos, trot = c["tpos"].float(), c["trot"].float()
    res = m.solve_ik(rob, tpos, trot if pose else None, offset=ik_ref.CONV_OFFSET, n_restarts=ik_ref.CONV_R, q_init=c["seeds"], max_iters=ik_ref.CONV_ITERS,
                     rot_weight=ik_ref.ROT_WEIGHT, pos_tol=1e-4, rot_tol=1e-3, **ik_ref.LAMBDA)
    q, conv = res.q.cpu(), res.converged.cpu()
    lo, hi = (torch.tensor(np.asarray(v, np.float32)) for v in rob.q_limits)
    assert bool((q >= lo).all() and (q <= hi).all())
    check = ik_ref.IKRef(name, torch.float64, **c["kw"])
    ep, eR, tr = check.errors(q.double(), tpos.double()[:, None, :], trot.double()[:, None, :, :])
    perr, rerr = ep.norm(dim=-1), eR.norm(dim=-1)
    slack = _fk_slack(name, q, offset=ik_ref.CONV_OFFSET)
    ref32 = ik_ref.reference_solution(name, pose, torch.float32)
    print(f"convergence {name} {'pose' if pose else 'position'}: converged per target {conv.sum(1).tolist()} (fp32 reference {ref32['converged'].sum(1).tolist()}); "
          f"slack {slack:.3e}; worst fp64 error of a converged restart {float(perr[conv].max()) if conv.any() else float('nan'):.3e} / "
          f"{float(rerr[conv].max()) if conv.any() and pose else 0.0:.3e}; max |err_out - fp64| {float((res.pos_err.cpu().double() - perr).abs().max()):.3e}")
    assert bool(conv.any(1).all()), conv.sum(1).tolist()                                      # no target is unsolved
    assert int(conv.sum()) >= 0.5 * int(ref32["converged"].sum())
    assert float(perr[conv].max()) <= 1e-4 + slack
    assert float((res.pos_err.cpu().double() - perr).abs().max()) <= slack
    if pose:
        assert float(rerr[conv].max()) <= 1e-3 + slack and bool((tr[conv] > 1).all())
        assert float((res.rot_err.cpu().double() - rerr).abs().max()) <= slack
    else:
        assert not bool(res.rot_err.any())
    assert int(res.iters.max()) <= ik_ref.CONV_ITERS and bool((res.iters.cpu()[~conv] == ik_ref.CONV_ITERS).all())


# ---------------------------------------------------------------------------------------------------------------- 5. interface
@pytest.mark.parametrize("name", ["Panda", "R3"])
def test_ik_coll_free_q(name):
    import mpd_public_amd as m
    rob = product_robot(name)
    task = m.TrajectoryDataset("EnvSpheres3D", rob, tensor_args={"device": "cuda", "dtype": torch.float32}).task
    gen = torch.Generator(device="cuda").manual_seed(11)
    q_free = task.random_coll_free_q(n_samples=1, device="cuda", generator=gen)
    target, _ = rob.fk(q_free[0].cpu(), offset=OFFSET)
    q = task.ik_coll_free_q(target, n_samples=8, offset=OFFSET, n_restarts=256, seed=3)
    assert 1 <= q.shape[0] <= 8 and q.shape[1] == rob.q_dim and q.is_cuda
    p, _ = rob.fk(q.cpu(), offset=OFFSET)
    err = (p - target).norm(dim=-1)
    slack = _fk_slack(name, q, offset=OFFSET)
    print(f"ik_coll_free_q {name}: {q.shape[0]} configurations, fp64 position errors {err.tolist()}")
    assert float(err.max()) <= 1e-4 + slack
    traj = torch.cat([q, torch.zeros_like(q)], -1)[:, None, :].expand(-1, 2, -1).contiguous()
    assert bool((task.trajectory_metrics(traj, n_check=2)[:, 0] == 0).all())
    d = torch.cdist(q.cpu(), q.cpu()) + 10 * torch.eye(q.shape[0])
    assert float(d.min()) > 0.05
    with pytest.raises(ValueError, match="No collision free configuration reaches the target"):
        task.ik_coll_free_q([5.0, 5.0, 5.0], n_restarts=64)


def test_experiment_plans_to_an_end_effector_goal():
    import mpd_public_amd as m
    from mpd_public_amd.inference import experiment
    chain = m.RobotChain.panda()
    task = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args={"device": "cuda", "dtype": torch.float32}).task
    q_free = task.random_coll_free_q(n_samples=1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    target, _ = chain.fk(q_free[0].cpu())
    kw = dict(model_id="EnvSpheres3D-RobotPanda", n_samples=4, model_args=dict(n_diffusion_steps=5, variance_schedule="cosine"), results_dir=None, debug=False)
    res = experiment(goal_ee_pos=target.tolist(), **kw)
    base = experiment(**kw)
    keys = {"trajs_iters", "trajs_final_coll", "trajs_final_coll_idxs", "trajs_final_free", "trajs_final_free_idxs", "success_free_trajs",
            "fraction_free_trajs", "collision_intensity_trajs", "idx_best_traj", "traj_final_free_best", "cost_best_free_traj",
            "cost_path_length_trajs_final_free", "cost_smoothness_trajs_final_free", "cost_all_trajs_final_free", "variance_waypoint_trajs_final_free",
            "t_total"}
    assert set(base) == keys and set(res) == keys | {"goal_ee_pos", "goal_ee_error"}
    final = res["trajs_iters"][-1]
    assert final.shape == (4, 64, 14) and bool(torch.isfinite(final).all())
    q_goal = final[:, -1, :7].cpu()
    p, _ = chain.fk(q_goal)
    slack = _fk_slack("Panda", q_goal)
    err = (p - target).norm(dim=-1)
    print(f"experiment(goal_ee_pos): tool position error of the last waypoints {err.tolist()}, goal_ee_error {res['goal_ee_error']:.3e}, slack {slack:.3e}")
    assert float(err.max()) <= 1e-4 + slack and 0.0 <= res["goal_ee_error"] <= 1e-4 + slack
    assert torch.allclose(res["goal_ee_pos"].double(), target, atol=1e-7)
    assert float((final[:, 0, :7] - base["trajs_iters"][-1][:, 0, :7]).abs().max()) == 0.0     # the start is drawn as before
