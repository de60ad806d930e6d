"""CPU references for the GPMP2 step tests (plain torch, float64; no GPU, no library call): the normwise backward error of a step against
the oracle's system, the "which trajectories can an fp32 evaluation not decide" predicate, the Levenberg-Marquardt judge restated from
include/mpdx.h, the test trajectories, and the table of (H, n_interp) cases test_gpu_gpmp_step.py runs (kept here so that the CPU suite can
check the table's ambiguity caps without a GPU)."""
import numpy as np
import torch

from helpers import obstacle_hugging_trajs, oracle_guide
from oracle import gpmp as ogpmp
from oracle.guide import interpolate_points_v1
from oracle.normalizer import LimitsNormalizer

DT, SIGMA_GP, SIGMA_OBS = 5.0 / 64, 1.0, 2e-2
B_CASE = 4
ETA_CEIL, ETA_FACTOR = 2e-6, 32.0      # eta_gpu <= 32 eta_ref32 and never above 2e-6 (a factor 4.5 under the smallest defect measured: 9.1e-6)

PM, PANDA = ("EnvDense2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")
PM3 = ("EnvSpheres3D", "RobotPointMass3D")     # the 3-D point mass (q_dim 3 / ws_dim 3 instantiation of the step kernel)
# (env, robot, H, n_interp [None: interpolation off], lambda).  Level sizes of the solver's tree: n = H - 2, halved until 1.  The two
# lambda = 1e-6 repeats: point mass with uneven segments and odd levels (46, 23, 11, 5, 2, 1), Panda with the all-even tree (16, 8, 4, 2, 1).
STEP_CASES = ([PM + (H, N, 1e-2) for H, N in ((4, 8), (5, 10), (6, 12), (10, 20), (18, 36), (24, 128), (34, 68), (40, 80), (48, 128), (96, 128),
                                              (128, 128), (128, 256), (24, None))]
            + [PANDA + (H, N, 1e-2) for H, N in ((4, 8), (5, 10), (6, 12), (10, 20), (18, 36), (24, 48), (34, 68), (40, 128), (48, 96))]
            + [PM + (48, 128, 1e-6), PANDA + (18, 36, 1e-6)]
            + [PM3 + (H, N, 1e-2) for H, N in ((5, 10), (24, 48))])


def level_sizes(H):
    n, out = H - 2, []
    while n >= 1:
        out.append(n)
        n >>= 1
    return out


def linearisation_parts(robot_id, H, N):
    """the thread mapping gpmp_lm_kernel's linearisation takes (csrc/planner.hpp): four threads per point when 4 N fit the 512 threads and
    the two extra term arrays fit the system's storage, else two."""
    qd = {"RobotPanda": 7, "RobotPointMass3D": 3}.get(robot_id, 2)
    msz, dd = qd * (qd + 1) // 2 + qd + 1, 4 * qd * qd
    return 4 if (4 * N <= 512 and 2 * N * msz <= 2 * (H - 2) * dd) else 2


# ---------------------------------------------------------------------------------------------------------------- trajectories, oracle terms
def gpmp_case(ds, H, B=B_CASE):
    """[B, H, D] float32 raw-unit test trajectories: the obstacle-hugging family of the planner tests at 64 supports, rows picked
    (H <= 64) or linearly interpolated along the horizon (H > 64)."""
    env_id = type(ds.env).__name__
    xn = obstacle_hugging_trajs(ds, B, seed=f"gpmp2/{env_id}", scale=0.9)
    xu = LimitsNormalizer(ds.normalizer.mins.cpu(), ds.normalizer.maxs.cpu()).unnormalize(xn).double()
    if H <= 64:
        xu = xu[:, torch.linspace(0, 63, H, dtype=torch.float64).round().long()]
    else:
        xu = interpolate_points_v1(xu, H)
    return xu.float().contiguous()


def oracle_terms(ds, dtype=torch.float64):
    """(robot, collision terms) of oracle/costs.py for the dataset's task, cutoff margin as the planner's."""
    _, comp = oracle_guide(ds, 1.0, 1.0, clip_grad=False, dtype=dtype)
    coll = comp.cost_l[:-1]
    for c in coll:
        c.cutoff = ds.task.obstacle_cutoff_margin
    return coll[0].robot, coll


def points_of(theta, n_interp):
    """the points the collision factors are evaluated on: theta [..., H, D] -> [..., N, D]"""
    return interpolate_points_v1(theta, n_interp) if n_interp else theta


# ---------------------------------------------------------------------------------------------------------------- the metric
def backward_error(A, g, delta_free):
    """normwise backward error of delta as a solution of A delta = -g:  eta = |A delta + g|_2 / (|A|_2 |delta|_2 + |g|_2)  (Rigal & Gaches):
    the size, relative to (A, g), of the smallest perturbation of the system that delta solves exactly.  float64 throughout."""
    A, g, d = A.double(), g.double().reshape(-1), delta_free.double().reshape(-1)
    num = torch.linalg.norm(A @ d + g)
    den = torch.linalg.matrix_norm(A, 2) * torch.linalg.norm(d) + torch.linalg.norm(g)
    return float(num / den)


def solve_step(A, g, H, D):
    out = torch.zeros((H, D), dtype=A.dtype)
    out[1:-1] = -torch.linalg.solve(A, g).reshape(H - 2, D)
    return out


def step_ref32(ds, theta, n_interp, lam):
    """the oracle's step evaluated ENTIRELY in float32 (collision terms, forward-mode Jacobian, normal equations, pivoted dense solve)"""
    robot, coll = oracle_terms(ds, torch.float32)
    A, g, _ = ogpmp.normal_equations(theta.float(), robot, coll, DT, SIGMA_GP, SIGMA_OBS, n_interp or 0, lam)
    return solve_step(A, g, *theta.shape)


_RECORDS = {}


def oracle_record(ds, theta, n_interp, lam):
    """the fp64 system, step and objective of ONE float32 trajectory theta [H, D] (CPU), the all-fp32 oracle's backward error on it and its
    ambiguity flag - computed once per (task, trajectory bits, n_interp, lambda) and shared by the tests that need it; callers do not
    modify it."""
    key = (type(ds.env).__name__, ds.robot.name, tuple(theta.shape), n_interp, float(lam), theta.numpy().tobytes())
    if key not in _RECORDS:
        robot, coll = oracle_terms(ds)
        A, g, F = ogpmp.normal_equations(theta.double(), robot, coll, DT, SIGMA_GP, SIGMA_OBS, n_interp or 0, lam)
        d32 = step_ref32(ds, theta, n_interp, lam)
        amb = bool(factor_ambiguity(coll, points_of(theta.double()[None], n_interp))[0])
        _RECORDS[key] = dict(A=A, g=g, F=float(F), want=solve_step(A, g, *theta.shape), eta_ref32=backward_error(A, g, d32[1:-1]), ambiguous=amb)
    return _RECORDS[key]


# ---------------------------------------------------------------------------------------------------------------- ambiguity
def factor_ambiguity(collision_costs, xi, eps=1e-5):
    """xi [B, N, D] float64 interpolated points -> [B] bool: the trajectory has a collision factor whose form (active or not, which
    primitive, which box face) changes within eps of the point - two correct evaluations in different precisions may then linearise two
    different systems, and neither is wrong.  Decided from the float64 oracle alone:
      (1) a hinge of any field (objects, workspace faces, self pairs) with |margin - distance| < eps;
      (2) a link sphere whose objects-field hinge is active or within eps of it (slack > -eps) and whose two nearest primitives are within eps;
      (3) such a sphere within eps of a face plane (|d_j| < eps, d = |p - c| - h) of a box it is within the margin of."""
    xi = xi.double()
    amb = torch.zeros(xi.shape[0], dtype=torch.bool)
    for term in collision_costs:
        rob, f = term.robot, term.field
        pts = rob.link_points(xi[..., : rob.q_dim])          # [B, N, K, dim]
        radii = rob.radii.double()
        if f.kind == "objects":
            margin = radii + term.cutoff
            parts, box_d = [], None
            if f.sphere_radii.numel():
                parts.append(torch.linalg.norm(pts.unsqueeze(-2) - f.sphere_centers.double(), dim=-1) - f.sphere_radii.double())
            if f.box_centers.numel():
                box_d = (pts.unsqueeze(-2) - f.box_centers.double()).abs() - f.box_half.double()      # [B, N, K, nb, dim]
                box_sd = torch.minimum(box_d.amax(-1), torch.zeros_like(box_d[..., 0])) + torch.linalg.norm(torch.relu(box_d), dim=-1)
                parts.append(box_sd)
            sd = torch.cat(parts, -1)                           # [B, N, K, n_prims]
            slack = margin - sd.amin(-1)
            bad = slack.abs() < eps
            near = slack > -eps
            if sd.shape[-1] > 1:
                two = sd.topk(2, dim=-1, largest=False)[0]
                bad |= near & ((two[..., 1] - two[..., 0]) < eps)
            if box_d is not None:
                within = (margin.unsqueeze(-1) - box_sd) > -eps                                      # [B, N, K, nb]
                bad |= near & (within & (box_d.abs() < eps).any(-1)).any(-1)
            amb |= bad.flatten(1).any(1)
        elif f.kind == "workspace":
            m = (radii + term.cutoff).unsqueeze(-1)
            s = torch.cat([m - (pts - f.ws_min.double()), m - (f.ws_max.double() - pts)], -1)
            amb |= (s.abs() < eps).flatten(1).any(1)
        else:
            a, b = pts[..., f.pairs[:, 0], :], pts[..., f.pairs[:, 1], :]
            s = radii[f.pairs[:, 0]] + radii[f.pairs[:, 1]] - torch.linalg.norm(a - b, dim=-1)
            amb |= (s.abs() < eps).flatten(1).any(1)
    return amb


# ---------------------------------------------------------------------------------------------------------------- the judge
def lm_expect(F_cur, lam, n_acc, F_cand, opts, first, solve):
    """What one mpdx_gpmp_step call does with the pending candidate (include/mpdx.h, mpdx_gpmp_opts), in float32 arithmetic:
    -> dict(accept, F, lam [negative: converged], n_acc, F_cand, proposes [delta is a new proposal, not zeros])."""
    f32 = np.float32
    F_cur, lam, F_cand = f32(F_cur), f32(lam), f32(F_cand)
    accept = bool(first or ((not opts.adaptive or F_cand < F_cur) and not np.isnan(F_cand)))   # the first call takes the (zero) proposal
    converged = False
    if accept and not first:
        n_acc += 1
        if opts.adaptive:
            lam = max(f32(lam * f32(opts.lambda_down)), f32(opts.lambda_min))
            converged = bool(F_cur - F_cand <= f32(1e-7) * F_cur)
    elif not accept:
        converged = bool(lam >= f32(opts.lambda_max))              # a rejection with lambda at its ceiling: nothing left to try
        if not converged:
            lam = min(f32(lam * f32(opts.lambda_up)), f32(opts.lambda_max))
    return dict(accept=accept, F=float(F_cand if accept else F_cur), lam=float(-lam if converged else lam), n_acc=float(n_acc),
                F_cand=float(F_cand), proposes=bool(solve and not converged))
