"""Reference side of the chain-robot inverse kinematics (mpdx_ik_solve, mpd_public_amd.solve_ik): a torch restatement of one
Levenberg-Marquardt iteration and of the whole loop, in a chosen dtype, on chain_ref.RobotChainRef.frames.  Written from the description in
include/mpdx.h, not from csrc/ik.hpp:

  FK         frames T_0 ... T_n of RobotChainRef; O_j, z_j = origin and third rotation column of T_j; tool point p = O_f + Rot_f offset
  residual   e = [p - p*; w_r e_R],  e_R = 1/2 sum_i Rot_f[:, i] x R*[:, i];  w_r = 0: the three position rows only
  Jacobian   of the residual, one column per joint j <= f: revolute [z_j x (p - O_j); -w_r z_j], prismatic [z_j; 0]; joints j > f: zero columns
             (the rotation block is the geometric-Jacobian Gauss-Newton approximation: d e_R / dq = -J_w to first order in e_R)
  solve      (J^T J + lambda I) dq = -J^T e   (the product floors a Cholesky pivot rounding has pushed below lambda; not needed, not restated here)
  candidate  q_c = clamp(q + dq, q_lo, q_hi); adaptive: accept iff F_c < F (F = 1/2 |e|^2), then lambda <- max(lambda down, lambda_min), else
             lambda <- min(lambda up, lambda_max); not adaptive: always accept, lambda fixed
  stop       before every iteration: |p - p*| <= pos_tol (and, w_r > 0, |e_R| <= rot_tol and trace(Rot_f^T R*) > 1), or max_iters iterations done

Also the shared fixtures of tests/test_ik_cpu.py and tests/test_gpu_ik.py (the convergence cases with their seeds, computed once)."""
import functools

import numpy as np
import torch

from chain_ref import RobotChainRef, description

LAMBDA = dict(lambda_init=1e-2, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-6, lambda_max=1e4)   # solve_ik's defaults
ROT_WEIGHT = 0.3


class IKRef:
    def __init__(self, name_or_desc, dtype=torch.float64, frame=None, offset=(0.0, 0.0, 0.0), rot_weight=0.0, pos_tol=1e-4, rot_tol=1e-3, adaptive=True,
                 lambda_init=1e-2, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-6, lambda_max=1e4):
        self.desc = description(name_or_desc) if isinstance(name_or_desc, str) else name_or_desc
        self.dtype = dtype
        self.rob = RobotChainRef(self.desc, dtype)
        self.n = self.rob.q_dim
        self.frame = self.n if frame is None else int(frame)
        assert 1 <= self.frame <= self.n
        self.offset = torch.tensor(list(offset), dtype=dtype)
        self.w = float(rot_weight)
        self.pos_tol, self.rot_tol, self.adaptive = pos_tol, rot_tol, adaptive
        self.lam0, self.up, self.down, self.lmin, self.lmax = lambda_init, lambda_up, lambda_down, lambda_min, lambda_max
        # the limits as the product holds them (float32 values), in the reference's dtype
        self.lo = torch.tensor(np.asarray(self.desc["q_limits"][0], np.float32)).to(dtype)
        self.hi = torch.tensor(np.asarray(self.desc["q_limits"][1], np.float32)).to(dtype)
        self.prismatic = [k in ("prismatic", 1) for _R, _t, k in self.desc["joints"]]

    # ---- one evaluation
    def pose(self, q):
        """(p [..., 3], Rot [..., 3, 3], frames) of the tool point / frame f"""
        fr = self.rob.frames(q)
        T = fr[self.frame]
        Rot = T[..., :3, :3]
        return T[..., :3, 3] + (Rot @ self.offset), Rot, fr

    def errors(self, q, tpos, trot):
        """e_p [..., 3], e_R [..., 3], trace [...] at q"""
        p, Rot, _ = self.pose(q)
        tpos, trot = tpos.to(self.dtype), trot.to(self.dtype)
        eR = 0.5 * torch.cross(Rot.transpose(-1, -2), trot.transpose(-1, -2).expand_as(Rot), dim=-1).sum(-2)
        tr = (Rot * trot).sum((-1, -2))
        return p - tpos, eR, tr

    def residual(self, q, tpos, trot):
        ep, eR, tr = self.errors(q, tpos, trot)
        e = torch.cat([ep, self.w * eR], -1) if self.w > 0 else ep
        return e, torch.linalg.norm(ep, dim=-1), (torch.linalg.norm(eR, dim=-1) if self.w > 0 else torch.zeros_like(tr)), tr

    def jacobian(self, q):
        """the residual's Jacobian [..., 3 | 6, n]"""
        p, _Rot, fr = self.pose(q)
        cols = []
        rows = 6 if self.w > 0 else 3
        for j in range(self.n):
            if j + 1 > self.frame:
                cols.append(torch.zeros(q.shape[:-1] + (rows,), dtype=self.dtype))
                continue
            O, z = fr[j + 1][..., :3, 3], fr[j + 1][..., :3, 2]
            if self.prismatic[j]:
                jv, jw = z, torch.zeros_like(z)
            else:
                jv, jw = torch.cross(z, p - O, dim=-1), z
            cols.append(torch.cat([jv, -self.w * jw], -1) if self.w > 0 else jv)
        return torch.stack(cols, -1)

    def converged(self, perr, rerr, tr):
        c = perr <= self.pos_tol
        if self.w > 0:
            c = c & (rerr <= self.rot_tol) & (tr > 1)
        return c

    # ---- one iteration at damping lam ([...] or a float): (dq, q_c, F, F_c)
    def step(self, q, lam, tpos, trot):
        q = q.to(self.dtype)
        e, _, _, _ = self.residual(q, tpos, trot)
        J = self.jacobian(q)
        lam = torch.as_tensor(lam, dtype=self.dtype).expand(q.shape[:-1])
        A = J.transpose(-1, -2) @ J + lam[..., None, None] * torch.eye(self.n, dtype=self.dtype)
        g = (J.transpose(-1, -2) @ e[..., None])
        dq = -torch.linalg.solve(A, g)[..., 0]
        qc = torch.minimum(torch.maximum(q + dq, self.lo), self.hi)
        ec, _, _, _ = self.residual(qc, tpos, trot)
        return dq, qc, 0.5 * (e * e).sum(-1), 0.5 * (ec * ec).sum(-1)

    # ---- the loop: q0 [..., n] seeds; tpos [..., 3], trot [..., 3, 3] broadcastable to them
    def solve(self, q0, tpos, trot, max_iters=100):
        q = q0.to(self.dtype).clone()
        lead = q.shape[:-1]
        lam = torch.full(lead, self.lam0, dtype=self.dtype)
        running = torch.ones(lead, dtype=torch.bool)
        conv = torch.zeros(lead, dtype=torch.bool)
        iters = torch.zeros(lead, dtype=torch.int32)
        perr = torch.zeros(lead, dtype=self.dtype)
        rerr = torch.zeros(lead, dtype=self.dtype)
        for it in range(max_iters + 1):
            _, pe, re, tr = self.residual(q, tpos, trot)
            perr = torch.where(running, pe, perr)
            rerr = torch.where(running, re, rerr)
            c = self.converged(pe, re, tr)
            conv = torch.where(running, c, conv)
            running = running & ~c & (it < max_iters)
            if not bool(running.any()):
                break
            _dq, qc, F, Fc = self.step(q, lam, tpos, trot)
            if self.adaptive:
                acc = Fc < F
                lam_new = torch.where(acc, torch.clamp(lam * self.down, min=self.lmin), torch.clamp(lam * self.up, max=self.lmax))
                lam = torch.where(running, lam_new, lam)
            else:
                acc = torch.ones(lead, dtype=torch.bool)
            q = torch.where((running & acc)[..., None], qc, q)
            iters = iters + running.to(torch.int32)
        return dict(q=q, pos_err=perr, rot_err=rerr, converged=conv, iters=iters)


def target_of(name, q_star, frame=None, offset=(0.0, 0.0, 0.0)):
    """(p* [..., 3], R* [..., 3, 3]) = the fp64 pose of the tool point at q_star"""
    ref = IKRef(name, torch.float64, frame=frame, offset=offset)
    p, Rot, _ = ref.pose(torch.as_tensor(q_star, dtype=torch.float64))
    return p, Rot


def random_q(name, shape, rng, margin=0.0):
    """float32 configurations inside the joint limits from a numpy generator"""
    lo, hi = (np.asarray(v, np.float32) for v in description(name)["q_limits"])
    u = rng.random(tuple(shape) + (lo.size,))
    span = (hi - lo).astype(np.float64)
    return torch.tensor((lo + span * (margin + (1 - 2 * margin) * u)).astype(np.float32)).clamp(torch.tensor(lo), torch.tensor(hi))


# ---------------------------------------------------------------------------------------------------------------- the convergence cases
CONV_ROBOTS = ("R3", "R8", "Panda")
CONV_OFFSET = (0.04, -0.03, 0.08)
CONV_N, CONV_R, CONV_ITERS = 4, 64, 100


@functools.lru_cache(maxsize=None)
def convergence_case(name, pose):
    """dict(q_star [4, n], tpos [4, 3], trot [4, 3, 3] (fp64), seeds [4, 64, n] float32, kw) of one convergence case: targets FK(q*) of 4 random
    q* inside the limits, 64 seeds per target uniform in the limits, from a fixed numpy generator; last frame, tool point CONV_OFFSET.  The q*
    span the whole joint ranges, but for the pose case of the 8-joint robot, where they come from the middle 30 % of every range: a solver
    that only clamps at the limits reaches a pose next to the limits of that robot from too few of 64 uniform seeds for a test of the
    arithmetic (test_ik_cpu.py checks that the reference solves every target of every case)."""
    rng = np.random.default_rng(1)
    q_star = random_q(name, (CONV_N,), rng, margin=0.35 if (name == "R8" and pose) else 0.0)
    tpos, trot = target_of(name, q_star, offset=CONV_OFFSET)
    seeds = random_q(name, (CONV_N, CONV_R), rng)
    kw = dict(offset=CONV_OFFSET, rot_weight=ROT_WEIGHT if pose else 0.0, pos_tol=1e-4, rot_tol=1e-3, adaptive=True, **LAMBDA)
    return dict(q_star=q_star, tpos=tpos, trot=trot, seeds=seeds, kw=kw)


@functools.lru_cache(maxsize=None)
def reference_solution(name, pose, dtype):
    """the reference's solve of a convergence case in `dtype` (shared, never modified)"""
    c = convergence_case(name, pose)
    ref = IKRef(name, dtype, **c["kw"])
    return ref.solve(c["seeds"], c["tpos"][:, None, :], c["trot"][:, None, :, :], max_iters=CONV_ITERS)
