"""solve_ik() - inverse kinematics of a chain robot on the GPU: end-effector targets -> sets of joint configurations.

An extension (the reference takes every goal as a joint configuration, scripts/inference/inference.py:161): batched damped least squares
(Levenberg-Marquardt) from many seeds per target, one launch of csrc/ik.hpp behind mpdx_ik_solve (arithmetic in include/mpdx.h).  The restarts
that converge sample the solution set of a redundant arm; PlanningTask.ik_coll_free_q filters them for collisions and
parallel.plan_contexts can plan to all of them in one batch.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .planning import RobotChain

_PANDA_CHAIN = None


def chain_of(robot) -> RobotChain:
    """The RobotChain the solver runs on: the robot itself, or RobotChain.panda() for the built-in RobotPanda (the same arm as a table)."""
    global _PANDA_CHAIN
    if isinstance(robot, RobotChain):
        return robot
    if getattr(robot, "robot_id", None) == _lib.ROBOT_PANDA:
        if _PANDA_CHAIN is None:
            _PANDA_CHAIN = RobotChain.panda()
        return _PANDA_CHAIN
    raise ValueError(f"solve_ik needs a RobotChain or RobotPanda; {getattr(robot, 'name', type(robot).__name__)} has no kinematic chain")


@dataclass
class IKResult:
    """Per (target, restart); a single target (target_pos of shape [3]) drops the leading axis."""
    q: torch.Tensor           # [n, R, q_dim] final configurations, inside the joint limits
    pos_err: torch.Tensor     # [n, R] |p - p*|
    rot_err: torch.Tensor     # [n, R] |e_R| (0 for a position-only solve)
    converged: torch.Tensor   # [n, R] bool
    iters: torch.Tensor       # [n, R] int32 iterations used


def solve_ik(robot, target_pos, target_rot=None, *, frame=None, offset=(0.0, 0.0, 0.0), n_restarts=64, q_init=None, max_iters=100, pos_tol=1e-4,
             rot_tol=1e-3, rot_weight=0.3, seed=0, device="cuda", lambda_init=1e-2, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-6,
             lambda_max=1e4, adaptive=True) -> IKResult:
    """target_pos [3] or [n, 3]; target_rot None (position only) or [3, 3] / [n, 3, 3] rotation matrices of the frame in the world.
    frame: 1 ... q_dim (default: the last); offset: the tool point in that frame.  q_init [n, n_restarts, q_dim] (or [n_restarts, q_dim] for a
    single target) replaces the Philox seeds drawn inside the joint limits from `seed`; it is clamped into the limits (by the kernel).
    rot_weight (metres per radian) weighs the orientation rows of the residual against the position rows."""
    chain = chain_of(robot)
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("mpd_public_amd.solve_ik needs an AMD GPU (no CPU fallback)")
    qd = chain.q_dim
    tp = torch.as_tensor(target_pos, dtype=torch.float32).cpu()
    single = tp.dim() == 1
    tp = tp.reshape(-1, 3)
    n = tp.shape[0]
    if target_rot is None:
        tr, w_r = torch.eye(3).expand(n, 3, 3), 0.0
    else:
        tr, w_r = torch.as_tensor(target_rot, dtype=torch.float32).cpu().reshape(-1, 3, 3), float(rot_weight)
        if tr.shape[0] != n:
            raise ValueError(f"target_rot: {tr.shape[0]} rotations for {n} positions")
        if not w_r > 0:
            raise ValueError("rot_weight must be positive when target_rot is given")
    target = torch.cat([tp, tr.reshape(n, 9)], 1).contiguous().to(device)
    R = int(n_restarts)
    o = _lib.IkOpts()
    o.frame = qd if frame is None else int(frame)
    o.offset = (C.c_float * 3)(*[float(v) for v in offset])
    lo, hi = chain.q_limits
    o.q_lo = (C.c_float * 8)(*([float(v) for v in lo] + [0.0] * (8 - qd)))
    o.q_hi = (C.c_float * 8)(*([float(v) for v in hi] + [0.0] * (8 - qd)))
    o.rot_weight, o.pos_tol, o.rot_tol = w_r, float(pos_tol), float(rot_tol)
    o.lambda_init, o.lambda_up, o.lambda_down, o.lambda_min, o.lambda_max = float(lambda_init), float(lambda_up), float(lambda_down), float(lambda_min), float(lambda_max)
    o.adaptive, o.max_iters, o.seed = int(bool(adaptive)), int(max_iters), int(seed) & 0xFFFFFFFFFFFFFFFF
    if q_init is not None:
        q_init = torch.as_tensor(q_init, dtype=torch.float32).to(device)
        if q_init.numel() != n * R * qd or q_init.shape[-1] != qd:
            raise ValueError(f"q_init: [{n}, {R}, {qd}] is expected, got {tuple(q_init.shape)}")
        q_init = q_init.reshape(n, R, qd).contiguous()
    table = torch.from_numpy(chain.table()).to(device)   # (under 1.3 KB: rebuilt per call, so a chain edited between calls is the chain solved)
    gp = _lib.GuideParams()
    gp.robot, gp.q_dim, gp.ws_dim = _lib.ROBOT_CHAIN, qd, 3
    gp.chain, gp.n_chain_floats = table.data_ptr(), table.numel()
    q_out = torch.empty((n, max(R, 1), qd), dtype=torch.float32, device=device)
    err = torch.empty((n, max(R, 1), 2), dtype=torch.float32, device=device)
    status = torch.empty((n, max(R, 1)), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().mpdx_ik_solve(C.byref(gp), C.byref(o), target.data_ptr(), _lib.ptr(q_init), q_out.data_ptr(), err.data_ptr(), status.data_ptr(),
                                             n, R, _lib.current_stream()), "mpdx_ik_solve")
        target.record_stream(torch.cuda.current_stream())
        table.record_stream(torch.cuda.current_stream())
        if q_init is not None:
            q_init.record_stream(torch.cuda.current_stream())
    res = IKResult(q_out, err[..., 0], err[..., 1], (status & 1).bool(), status >> 8)
    if single:
        res = IKResult(res.q[0], res.pos_err[0], res.rot_err[0], res.converged[0], res.iters[0])
    return res
