"""Host-side descriptors of the planning problem: environments, robots, the planning task and the cost terms.

In the reference these come from the un-vendored `torch_robotics` / `mp_baselines` submodules (empty in the reference
tree): envs `EnvSimple2D / EnvDense2D / EnvNarrowPassageDense2D / EnvSpheres3D`, robots `RobotPointMass / RobotPanda`,
`PlanningTask`, and `CostCollision / CostGPTrajectory / CostComposite` (scripts/inference/inference.py:14,107-123,
188-225).  Here they are thin DESCRIPTORS with the reference's constructor signatures; the arithmetic runs in the HIP
guide kernel (csrc/guide.hpp).  Geometry is synthetic and formula-defined - the authors'
environments are not in the reference tree.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import synthetic as syn
from . import _lib
from .grid_sdf import GRID_MODES, MESH_SIGNS, GridSDF, grid_spec_for, _check_mesh, _mesh_vertices, _occupancy_bytes  # noqa: F401  (the grid module's names, as they were importable from here)

# ------------------------------------------------------------------------------------------------ geometry


@dataclass
class ObjectSet:
    """sphere + axis-aligned box primitives; rows padded to 3-D (z = 0 in 2-D).

    track (extension; None = the set does not move): [H, dim] or [H, 3] - row h is the rigid translation of ALL the set's primitives at the time of
    support point h, relative to the centres above (include/mpdx.h, the track members of mpdx_field).  No rotation, one track per set."""
    sphere_centers: np.ndarray  # [ns, 3]
    sphere_radii: np.ndarray    # [ns]
    box_centers: np.ndarray     # [nb, 3]
    box_half: np.ndarray        # [nb, 3]
    track: Optional[np.ndarray] = None

    @staticmethod
    def empty():
        z3, z1 = np.zeros((0, 3), np.float32), np.zeros((0,), np.float32)
        return ObjectSet(z3, z1, z3.copy(), z3.copy())

    def with_linear_motion(self, start_offset, end_offset, n_support_points):
        """A copy of the set on a straight constant-velocity track: translated by start_offset at the first support point and by end_offset at the
        last of n_support_points (offsets of 2 or 3 coordinates)."""
        H = int(n_support_points)
        if H < 2:
            raise ValueError(f"n_support_points={n_support_points}: a track has at least 2 rows")
        a, b = (np.asarray(v, np.float64).reshape(-1) for v in (start_offset, end_offset))
        if a.shape != b.shape or a.size not in (2, 3):
            raise ValueError(f"start_offset / end_offset: two vectors of 2 or 3 coordinates are expected, got {a.shape} and {b.shape}")
        s = np.linspace(0.0, 1.0, H)[:, None]
        return ObjectSet(self.sphere_centers, self.sphere_radii, self.box_centers, self.box_half, ((1.0 - s) * a + s * b).astype(np.float32))

    def track_rows(self, n_support_points):
        """The track as the kernels read it: [H, 4] float32 rows (ox, oy, oz, 0).  ValueError unless it has n_support_points rows of 2 or 3 entries."""
        t = np.asarray(self.track, np.float32)
        if t.ndim != 2 or t.shape[1] not in (2, 3):
            raise ValueError(f"track: [H, dim] or [H, 3] is expected, got {t.shape}")
        if not np.isfinite(t).all():
            raise ValueError("track: non-finite entry (the kernels do not fault on one, but what the field then reports is not defined)")
        if t.shape[0] != int(n_support_points):
            raise ValueError(f"track has {t.shape[0]} rows for n_support_points={n_support_points}: one row per support point")
        rows = np.zeros((t.shape[0], 4), np.float32)
        rows[:, : t.shape[1]] = t
        return rows

    def prim_floats(self):
        sp = np.concatenate([self.sphere_centers, self.sphere_radii[:, None]], 1).astype(np.float32).reshape(-1)
        bx = np.concatenate([self.box_centers, self.box_half], 1).astype(np.float32).reshape(-1)
        return sp, bx


def _pad3(a, dim):
    a = np.asarray(a, np.float32).reshape(-1, dim)
    return np.concatenate([a, np.zeros((a.shape[0], 3 - dim), np.float32)], 1)


class Env:
    def __init__(self, name: str, dim: int, fixed: ObjectSet, extra: ObjectSet, limits=(-1.0, 1.0)):
        self.name, self.dim, self.obj_fixed, self.obj_extra = name, dim, fixed, extra
        self.limits = (np.full(dim, limits[0], np.float32), np.full(dim, limits[1], np.float32))


def _spheres(tag, n, dim, rlo, rhi, lo=-0.9, hi=0.9):
    c = syn.hash_uniform(f"{tag}/centers", n * dim, lo, hi).reshape(n, dim)
    r = syn.hash_uniform(f"{tag}/radii", n, rlo, rhi) if rhi > rlo else np.full(n, rlo)
    return _pad3(c, dim), r.astype(np.float32)


def _boxes(tag, n, dim, half, lo=-0.9, hi=0.9):
    c = syn.hash_uniform(f"{tag}/centers", n * dim, lo, hi).reshape(n, dim)
    h = np.full((n, dim), half, np.float32)
    hp = np.concatenate([h, np.full((n, 3 - dim), 1.0, np.float32)], 1)  # 2-D boxes are unbounded along the unused axis
    return _pad3(c, dim), hp


def make_env(env_id: str) -> Env:
    """Synthetic stand-ins for the reference's environments."""
    if env_id == "EnvSimple2D":
        sc, sr = _spheres("simple2d/s", 8, 2, 0.1, 0.2)
        bc, bh = _boxes("simple2d/b", 2, 2, 0.1)
        ec, er = _spheres("simple2d/es", 2, 2, 0.1, 0.15)
        ebc, ebh = _boxes("simple2d/eb", 2, 2, 0.08)
        return Env(env_id, 2, ObjectSet(sc, sr, bc, bh), ObjectSet(ec, er, ebc, ebh))
    if env_id in ("EnvDense2D", "EnvNarrowPassageDense2D"):
        sc, sr = _spheres("dense2d/s", 20, 2, 0.125, 0.125)
        bc, bh = _boxes("dense2d/b", 6, 2, 0.1)
        if env_id == "EnvNarrowPassageDense2D":  # two wall boxes leaving a 0.1 gap at x = 0
            wc = _pad3([[0.0, 0.525], [0.0, -0.525]], 2)
            wh = np.array([[0.05, 0.475, 1.0], [0.05, 0.475, 1.0]], np.float32)
            bc, bh = np.concatenate([bc, wc]), np.concatenate([bh, wh])
        ec, er = _spheres("dense2d/es", 2, 2, 0.1, 0.125)
        ebc, ebh = _boxes("dense2d/eb", 2, 2, 0.08)
        return Env(env_id, 2, ObjectSet(sc, sr, bc, bh), ObjectSet(ec, er, ebc, ebh))
    if env_id == "EnvSpheres3D":
        sc, sr = _spheres("spheres3d/s", 15, 3, 0.15, 0.15, -0.8, 0.8)
        sc[:, 2] = 0.2 + 0.8 * (sc[:, 2] + 0.8) / 1.6  # keep them in the arm's workspace (z in [0.2, 1.0])
        ec, er = _spheres("spheres3d/es", 2, 3, 0.12, 0.15, -0.6, 0.6)
        ec[:, 2] = 0.3 + 0.5 * (ec[:, 2] + 0.6) / 1.2
        z = ObjectSet.empty()
        env = Env(env_id, 3, ObjectSet(sc, sr, z.box_centers, z.box_half), ObjectSet(ec, er, z.box_centers.copy(), z.box_half.copy()))
        env.limits = (np.array([-1.0, -1.0, -0.1], np.float32), np.array([1.0, 1.0, 1.5], np.float32))
        return env
    raise NotImplementedError(env_id)


# ------------------------------------------------------------------------------------------------ robots


class RobotPointMass:
    name = "RobotPointMass"

    def __init__(self, q_dim=2, link_margin=0.01, tensor_args=None, **kw):
        self.q_dim, self.link_margin, self.dt = q_dim, link_margin, None
        self.robot_id = _lib.ROBOT_POINTMASS

    def get_position(self, x):
        return x[..., : self.q_dim]

    def get_velocity(self, x):
        return x[..., self.q_dim: 2 * self.q_dim]


class RobotPanda:
    name = "RobotPanda"

    def __init__(self, tensor_args=None, **kw):
        self.q_dim, self.link_margin, self.dt = 7, 0.0, None
        self.robot_id = _lib.ROBOT_PANDA

    get_position = RobotPointMass.get_position
    get_velocity = RobotPointMass.get_velocity


# the package's Panda geometry (csrc/guide.hpp kPanda*): modified-DH rows (alpha_{i-1}, a_{i-1}, d_i), link spheres (frame 1..7, offset along the
# frame's z, radius) and self-collision pairs
PANDA_MDH_ALPHA = (0.0, -math.pi / 2, math.pi / 2, math.pi / 2, -math.pi / 2, math.pi / 2, math.pi / 2)
PANDA_MDH_A = (0.0, 0.0, 0.0, 0.0825, -0.0825, 0.0, 0.088)
PANDA_MDH_D = (0.333, 0.0, 0.316, 0.0, 0.384, 0.0, 0.0)
PANDA_LINK_SPHERES = ((1, -0.15, 0.10), (1, 0.0, 0.10), (3, -0.15, 0.09), (3, 0.0, 0.09), (4, 0.0, 0.09), (5, -0.25, 0.08),
                      (5, -0.12, 0.08), (5, 0.0, 0.08), (7, 0.0, 0.07), (7, 0.107, 0.06), (7, 0.17, 0.06))
PANDA_SELF_PAIRS = ((8, 0), (8, 1), (8, 2), (9, 0), (9, 1), (9, 2), (9, 3), (10, 0), (10, 1), (10, 2), (10, 3), (10, 4))


class RobotChain:
    """A serial kinematic chain described by a table (an extension: the reference builds one of its own robots by name); the guide and metrics
    kernels of csrc/chain.hpp run on it (robot id MPDX_ROBOT_CHAIN, table layout and forward kinematics in include/mpdx.h).

    joints      one (R, t, type) per joint, base to tip: R [3, 3] rotation and t [3] translation of the joint frame in its parent frame at
                q = 0; type 'revolute' (0: about the joint frame's z) or 'prismatic' (1: along it).  T_j = T_{j-1} [R | t] M(q_j).
    spheres     one (frame, offset [3], radius) per link collision sphere: frame 0 = the fixed base, k = moves with joint k (1-based)
    self_pairs  (a, b) sphere index pairs of the self-collision field (none: the task has no self field)
    q_limits    (lo [n], hi [n]) joint limits, default (-pi, pi); v_limit: the velocity limit of the synthetic normaliser
    At most 8 joints, 16 spheres and 24 pairs; 3-D workspaces, primitive / workspace / self fields (no signed-distance grid)."""

    def __init__(self, joints, spheres, self_pairs=(), q_limits=None, v_limit=2.5, name="RobotChain"):
        joints, spheres, self_pairs = list(joints), list(spheres), [tuple(p) for p in self_pairs]
        nj, ns, npair = len(joints), len(spheres), len(self_pairs)
        if not 1 <= nj <= _lib.ROBOT_CHAIN_MAX_JOINTS:
            raise ValueError(f"joints: {nj} joints, 1 ... {_lib.ROBOT_CHAIN_MAX_JOINTS} are supported")
        if not 1 <= ns <= _lib.ROBOT_CHAIN_MAX_SPHERES:
            raise ValueError(f"spheres: {ns} spheres, 1 ... {_lib.ROBOT_CHAIN_MAX_SPHERES} are supported")
        if npair > _lib.ROBOT_CHAIN_MAX_PAIRS:
            raise ValueError(f"self_pairs: {npair} pairs, at most {_lib.ROBOT_CHAIN_MAX_PAIRS} are supported")
        types = {"revolute": _lib.ROBOT_CHAIN_REVOLUTE, "prismatic": _lib.ROBOT_CHAIN_PRISMATIC, 0: 0, 1: 1}
        self.joint_R, self.joint_t, self.joint_type = np.zeros((nj, 3, 3)), np.zeros((nj, 3)), np.zeros(nj, np.int32)
        for j, jt in enumerate(joints):
            if len(jt) != 3:
                raise ValueError(f"joints[{j}]: (R [3, 3], t [3], type) is expected")
            R, t = np.asarray(jt[0], np.float64), np.asarray(jt[1], np.float64)
            if R.shape != (3, 3) or t.shape != (3,) or not (np.isfinite(R).all() and np.isfinite(t).all()):
                raise ValueError(f"joints[{j}]: R must be a finite [3, 3] matrix and t a finite 3-vector")
            if np.abs(R.astype(np.float32) @ R.astype(np.float32).T - np.eye(3, dtype=np.float32)).max() > 1e-4:
                raise ValueError(f"joints[{j}]: R is not orthonormal to 1e-4")
            if isinstance(jt[2], (bool, float)) or jt[2] not in types:
                raise ValueError(f"joints[{j}]: type {jt[2]!r} ('revolute' / 0 or 'prismatic' / 1)")
            self.joint_R[j], self.joint_t[j], self.joint_type[j] = R, t, types[jt[2]]
        self.sphere_frame, self.sphere_offset, self.sphere_radius = np.zeros(ns, np.int32), np.zeros((ns, 3)), np.zeros(ns)
        for k, sp in enumerate(spheres):
            if len(sp) != 3:
                raise ValueError(f"spheres[{k}]: (frame, offset [3], radius) is expected")
            fr, off, rad = int(sp[0]), np.asarray(sp[1], np.float64), float(sp[2])
            if fr != sp[0] or not 0 <= fr <= nj:
                raise ValueError(f"spheres[{k}]: frame {sp[0]!r} outside 0 ... n_joints ({nj})")
            if off.shape != (3,) or not np.isfinite(off).all():
                raise ValueError(f"spheres[{k}]: offset must be a finite 3-vector")
            if not (rad > 0 and math.isfinite(rad)):
                raise ValueError(f"spheres[{k}]: radius must be positive and finite")
            self.sphere_frame[k], self.sphere_offset[k], self.sphere_radius[k] = fr, off, rad
        for k, pr in enumerate(self_pairs):
            if len(pr) != 2 or any(int(v) != v or not 0 <= int(v) < ns for v in pr):
                raise ValueError(f"self_pairs[{k}]: indices {pr!r} outside the {ns} spheres")
        self.self_pairs = np.asarray(self_pairs, np.int32).reshape(-1, 2)
        if q_limits is None:
            q_limits = (np.full(nj, -math.pi), np.full(nj, math.pi))
        lo, hi = (np.asarray(v, np.float32).reshape(-1) for v in q_limits)
        if lo.shape != (nj,) or hi.shape != (nj,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi <= lo).any():
            raise ValueError(f"q_limits: (lo [{nj}], hi [{nj}]) with lo < hi is expected")
        if not (float(v_limit) > 0 and math.isfinite(float(v_limit))):
            raise ValueError("v_limit must be positive and finite")
        self.q_limits, self.v_limit = (lo, hi), float(v_limit)
        self.name, self.q_dim, self.link_margin, self.dt = name, nj, 0.0, None
        self.robot_id = _lib.ROBOT_CHAIN

    get_position = RobotPointMass.get_position
    get_velocity = RobotPointMass.get_velocity

    @property
    def n_spheres(self) -> int:
        return len(self.sphere_radius)

    @property
    def n_pairs(self) -> int:
        return len(self.self_pairs)

    def limits(self):
        """(mins [D], maxs [D]) of the synthetic trajectory normaliser: the joint limits, then +-v_limit."""
        vv = np.full(self.q_dim, self.v_limit, np.float32)
        return np.concatenate([self.q_limits[0], -vv]), np.concatenate([self.q_limits[1], vv])

    def table(self) -> np.ndarray:
        """The float32 chain table of include/mpdx.h (integer entries as int32 bit patterns)."""
        nj, ns, npair = self.q_dim, self.n_spheres, self.n_pairs
        H, JF, SF = _lib.ROBOT_CHAIN_HEADER_FLOATS, _lib.ROBOT_CHAIN_JOINT_FLOATS, _lib.ROBOT_CHAIN_SPHERE_FLOATS
        tab = np.zeros(H + JF * nj + SF * ns + 2 * npair, np.float32)
        ti = tab.view(np.int32)
        ti[0], ti[1], ti[2] = nj, ns, npair
        for j in range(nj):
            o = H + JF * j
            tab[o: o + 9], tab[o + 9: o + 12], ti[o + 12] = self.joint_R[j].reshape(-1), self.joint_t[j], self.joint_type[j]
        for k in range(ns):
            o = H + JF * nj + SF * k
            ti[o], tab[o + 1: o + 4], tab[o + 4] = self.sphere_frame[k], self.sphere_offset[k], self.sphere_radius[k]
        o = H + JF * nj + SF * ns
        ti[o: o + 2 * npair] = self.self_pairs.reshape(-1)
        return tab

    def fk(self, q, frame=None, offset=(0.0, 0.0, 0.0)):
        """Host-side forward kinematics in float64, from the joints the table is built from: q [..., n_joints] (numpy or a torch CPU tensor) ->
        (pos [..., 3], rot [..., 3, 3]) of `frame` (0 = the fixed base ... n_joints, the default) in the world; pos is the point `offset` of
        that frame.  T_j = T_{j-1} [R_j | t_j] M_j(q_j) as in include/mpdx.h."""
        is_torch = torch.is_tensor(q)
        qa = np.asarray(q.detach().cpu().numpy() if is_torch else q, np.float64)
        if qa.shape[-1] != self.q_dim:
            raise ValueError(f"q: last axis {qa.shape[-1]}, the chain has {self.q_dim} joints")
        frame = self.q_dim if frame is None else int(frame)
        if not 0 <= frame <= self.q_dim:
            raise ValueError(f"frame {frame} outside 0 ... n_joints ({self.q_dim})")
        lead = qa.shape[:-1]
        R = np.broadcast_to(np.eye(3), lead + (3, 3)).copy()
        T = np.zeros(lead + (3,))
        for j in range(frame):
            A = R @ self.joint_R[j]
            T = T + R @ self.joint_t[j]
            qj = qa[..., j]
            if self.joint_type[j] == _lib.ROBOT_CHAIN_PRISMATIC:
                R, T = A, T + qj[..., None] * A[..., :, 2]
            else:
                c, s = np.cos(qj)[..., None], np.sin(qj)[..., None]
                R = np.stack([A[..., :, 0] * c + A[..., :, 1] * s, A[..., :, 1] * c - A[..., :, 0] * s, A[..., :, 2]], axis=-1)
        pos = T + R @ np.asarray(offset, np.float64).reshape(3)
        return (torch.from_numpy(pos), torch.from_numpy(R)) if is_torch else (pos, R)

    @classmethod
    def from_mdh(cls, alpha, a, d, spheres, self_pairs=(), **kw):
        """A chain of revolute joints from modified-DH rows (Craig): T_i = Rot_x(alpha_{i-1}) Trans_x(a_{i-1}) Rot_z(theta_i) Trans_z(d_i), i.e.
        [R | t] = Rot_x(alpha) Trans_x(a) Trans_z(d) followed by the joint rotation (Rot_z and Trans_z commute)."""
        joints = []
        for al, aa, dd in zip(alpha, a, d):
            ca, sa = math.cos(al), math.sin(al)
            joints.append((np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]]), np.array([aa, -sa * dd, ca * dd]), "revolute"))
        return cls(joints, spheres, self_pairs, **kw)

    @classmethod
    def panda(cls, name="RobotPandaChain"):
        """The package's own Panda (geometry, link spheres, self-collision pairs and joint limits of RobotPanda) expressed as a chain.  RobotPanda
        stays the robot to plan a Panda with: its kernels are specialised (profiles/chain_guide_probe.md)."""
        joints = []
        for al, aa, dd in zip(PANDA_MDH_ALPHA, PANDA_MDH_A, PANDA_MDH_D):
            ca, sa = float(round(math.cos(al))), float(round(math.sin(al)))   # alpha is a multiple of pi / 2: exact entries, as the kernel's tables
            joints.append((np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]]), np.array([aa, -sa * dd, ca * dd]), "revolute"))
        spheres = [(fr, (0.0, 0.0, off), rad) for fr, off, rad in PANDA_LINK_SPHERES]
        return cls(joints, spheres, PANDA_SELF_PAIRS, q_limits=(syn.PANDA_Q_MIN, syn.PANDA_Q_MAX), v_limit=2.5, name=name)


_PANDA_CHAIN = None


def robot_link_spheres(robot, q) -> np.ndarray:
    """The robot's collision spheres in the world at q [q_dim] or [k, q_dim] (numpy or a torch tensor) -> [S, 4] float64 (centre, radius), the k
    configurations' spheres one after the other.  RobotPanda: RobotChain.panda().fk; a RobotChain: its own sphere table; a 3-D RobotPointMass: one
    sphere of link_margin at q.  The depth fusion (GridSDF.from_depth / integrate_depth) masks these, padded, out of the frames."""
    qa = np.asarray(q.detach().cpu().numpy() if torch.is_tensor(q) else q, np.float64)
    if qa.ndim not in (1, 2) or qa.shape[-1] != robot.q_dim:
        raise ValueError(f"robot_link_spheres: q is [{robot.q_dim}] or [k, {robot.q_dim}] for {robot.name}, got {tuple(qa.shape)}")
    if not np.isfinite(qa).all():
        raise ValueError("robot_link_spheres: q must be finite")
    qa = qa.reshape(-1, robot.q_dim)
    if isinstance(robot, RobotPointMass):
        if robot.q_dim != 3:
            raise ValueError(f"robot_link_spheres: a {robot.q_dim}-D point mass (depth fusion is 3-D only)")
        return np.concatenate([qa, np.full((qa.shape[0], 1), float(robot.link_margin))], 1)
    if isinstance(robot, RobotPanda):
        global _PANDA_CHAIN
        if _PANDA_CHAIN is None:
            _PANDA_CHAIN = RobotChain.panda()
        chain = _PANDA_CHAIN
    elif isinstance(robot, RobotChain):
        chain = robot
    else:
        raise ValueError(f"robot_link_spheres: {type(robot).__name__} (RobotPanda, RobotChain or a 3-D RobotPointMass)")
    out = np.zeros((qa.shape[0], chain.n_spheres, 4))
    for k in range(chain.n_spheres):
        out[:, k, :3] = chain.fk(qa, frame=int(chain.sphere_frame[k]), offset=chain.sphere_offset[k])[0]
        out[:, k, 3] = chain.sphere_radius[k]
    return out.reshape(-1, 4)


def make_robot(robot_id: str):
    if robot_id == "RobotPointMass":
        return RobotPointMass(2)
    if robot_id == "RobotPointMass3D":
        return RobotPointMass(3)
    if robot_id == "RobotPanda":
        return RobotPanda()
    raise NotImplementedError(robot_id)


# ------------------------------------------------------------------------------------------------ collision fields / task


@dataclass
class CollisionField:
    kind: int                       # _lib.FIELD_*
    objects: Optional[ObjectSet] = None
    ws_min: Optional[np.ndarray] = None
    ws_max: Optional[np.ndarray] = None
    name: str = ""
    grid: Optional[GridSDF] = None  # _lib.FIELD_GRID


class PlanningTask:
    """The attribute / method surface inference.py reads from `task` (inference.py:161,191-193,288-297)."""

    def __init__(self, env: Env, robot, obstacle_cutoff_margin=0.05, use_extra_objects=True, tensor_args=None, sdf_grid=None, moving_objects=None, **kw):
        """moving_objects (extension; None = as before): an ObjectSet with a `track` (ObjectSet.with_linear_motion, or a [H, dim] array of its own) -
        a further OBJECTS field named 'moving_objects' whose primitives translate along the track during the plan; the guide and the metrics test
        every trajectory point against the obstacle's position at that point's own time (include/mpdx.h, the track members).  The fixed and the
        extra set may carry a track as well (not a fixed set that becomes a grid).  At most MPDX_MAX_FIELDS fields: a Panda task with fixed, extra,
        workspace and self fields is full - build it with use_extra_objects=False and the moving set takes the extras' place.  Not for a RobotChain,
        PlanningScenes or the baseline planners.  random_coll_free_q / ik_coll_free_q, whose configurations have no time, test against the
        fields that do not move.
        sdf_grid (extension; None = the primitive tables, as before): dict(cell_size=..., mode='linear' | 'nearest', padding=0.3) - the FIXED
        objects become a signed-distance grid (baked from the primitives on the device on first use, mpdx_sdf_grid_bake) and
        get_collision_fields() returns a FIELD_GRID field in their place; extra objects, workspace and self fields stay as they are (as
        torch_robotics does, as recalled: the precomputed grid is for the fixed objects only).  An environment that already carries a grid
        (env.grid_fixed, set by task_from_torch_robotics) uses it as it is.  A `GridSDF` instance (GridSDF.from_occupancy / from_points / from_mesh, or node
        values of the caller's own) is used as the objects field as it is, the way env.grid_fixed is."""
        self.env, self.robot, self.obstacle_cutoff_margin = env, robot, obstacle_cutoff_margin
        if isinstance(robot, RobotChain):
            if env.dim != 3:
                raise ValueError("a RobotChain lives in a 3-D workspace (a planar arm is a chain whose axes are all z, among 3-D primitives)")
            if sdf_grid is not None or getattr(env, "grid_fixed", None) is not None:
                raise ValueError("a RobotChain takes primitive, workspace and self fields: no signed-distance grid")
            if moving_objects is not None or any(getattr(o, "track", None) is not None for o in (env.obj_fixed, env.obj_extra if use_extra_objects else None)):
                raise ValueError("a RobotChain takes no moving obstacles: tracks are for the point mass and the Panda (the chain kernels have no MOVING instantiation)")
        self.tensor_args = tensor_args or {"device": "cpu", "dtype": torch.float32}
        self.ws_min, self.ws_max = env.limits
        if moving_objects is not None:
            _check_object_set(moving_objects, env.dim, "moving_objects")
            if moving_objects.track is None:
                raise ValueError("moving_objects: the set has no track (ObjectSet.with_linear_motion, or set .track to a [H, dim] array)")
        given = sdf_grid if isinstance(sdf_grid, GridSDF) else None
        self.sdf_grid = given if given is not None else dict(sdf_grid) if sdf_grid is not None else None
        if given is not None:
            if given.dim != env.dim:
                raise ValueError(f"sdf_grid: a {given.dim}-D GridSDF for the {env.dim}-D workspace of {getattr(env, 'name', 'the environment')}")
            self.df_collision_objects = CollisionField(_lib.FIELD_GRID, grid=given, name="objects")
        elif getattr(env, "grid_fixed", None) is not None:
            self.df_collision_objects = CollisionField(_lib.FIELD_GRID, grid=env.grid_fixed, name="objects")
        elif self.sdf_grid is not None:
            unknown = set(self.sdf_grid) - {"cell_size", "mode", "padding"}
            if unknown or "cell_size" not in self.sdf_grid:
                raise ValueError(f"sdf_grid takes cell_size, mode, padding (got {sorted(self.sdf_grid)})")
            grid = GridSDF.for_primitives(env.obj_fixed, self.ws_min, self.ws_max, self.sdf_grid["cell_size"], self.sdf_grid.get("mode", "linear"),
                                          float(self.sdf_grid.get("padding", 0.3)))
            self.df_collision_objects = CollisionField(_lib.FIELD_GRID, objects=env.obj_fixed, grid=grid, name="objects")
        else:
            self.df_collision_objects = CollisionField(_lib.FIELD_OBJECTS, objects=env.obj_fixed, name="objects")
        self.df_collision_extra_objects = CollisionField(_lib.FIELD_OBJECTS, objects=env.obj_extra, name="extra_objects") if use_extra_objects else None
        self.df_collision_ws_boundaries = CollisionField(_lib.FIELD_WORKSPACE, ws_min=self.ws_min, ws_max=self.ws_max, name="workspace")
        has_self = robot.name == "RobotPanda" or (isinstance(robot, RobotChain) and robot.n_pairs > 0)
        self.df_collision_self = CollisionField(_lib.FIELD_SELF, name="self") if has_self else None
        self.df_collision_moving_objects = CollisionField(_lib.FIELD_OBJECTS, objects=moving_objects, name="moving_objects") if moving_objects is not None else None
        fields = self.get_collision_fields()
        if len(fields) > _lib.MAX_FIELDS:
            raise ValueError(f"{len(fields)} collision fields ({', '.join(f.name for f in fields)}); the kernels take at most {_lib.MAX_FIELDS} - build the task with "
                             f"use_extra_objects=False and the moving set takes the extras' place")
        self._gp_by_h = {}

    def get_collision_fields(self) -> List[CollisionField]:
        out = [self.df_collision_self, self.df_collision_objects, self.df_collision_ws_boundaries, self.df_collision_extra_objects,
               getattr(self, "df_collision_moving_objects", None)]
        return [f for f in out if f is not None]

    def get_collision_fields_extra_objects(self) -> List[CollisionField]:
        return [self.df_collision_extra_objects]

    def get_collision_fields_moving_objects(self) -> List[CollisionField]:
        return [self.df_collision_moving_objects]

    @property
    def has_tracks(self) -> bool:
        """a field of the task moves (its ObjectSet carries a track): the metrics need the horizon of the trajectories they check"""
        return any(field_track(f) is not None for f in self.get_collision_fields())

    # ---- collision checking / metrics (inference.py:161,288-297); arithmetic in csrc/guide.hpp::traj_metrics_kernel
    def _params(self, device, n_support_points=None, static_only=False):
        """The metrics' parameter block.  A task with a track keeps one block per horizon (a track has one row per support point; ValueError when the
        rows differ from n_support_points) and one of its static fields alone (static_only: configurations without a time).  A block is keyed by
        (device, horizon, the identity of every track array): assigning a new array to `objects.track` builds a new block at the next call;
        writing INTO a track array, or changing the primitives of a set, is not seen - build a new task (the one-block cache of a task without
        tracks has the same limit).  At most 8 blocks are kept (the oldest goes first).  refresh_grids() reaches every one of them."""
        if self.has_tracks:
            if n_support_points is None and not static_only:
                raise ValueError("this task has a moving obstacle (a track): its parameter block belongs to one horizon, and the baseline planners "
                                 "(RRTConnectBatch, GPMP2, edges_free) do not take it")
            from .guides import build_device_params
            tracks = tuple(id(field_track(f)) for f in self.get_collision_fields() if field_track(f) is not None)
            key = (torch.device(device), None if static_only else int(n_support_points), () if static_only else tracks)
            store = self.__dict__.setdefault("_gp_by_h", {})
            if key not in store:
                while len(store) >= 8:
                    del store[next(iter(store))]
                fields = [f for f in self.get_collision_fields() if not (static_only and field_track(f) is not None)]
                costs = [CostCollision(self.robot, key[1] or 64, field=f) for f in fields]
                store[key] = build_device_params(self.robot, self.env.dim, self.obstacle_cutoff_margin, None, None, costs, [1.0] * len(costs), True, 128,
                                                 True, 1.0, device)
            return store[key][0]
        if getattr(self, "_gp", None) is None or self._gp_prims.device != torch.device(device):
            from .guides import build_device_params
            costs = [CostCollision(self.robot, 64, field=f) for f in self.get_collision_fields()]
            self._gp, self._gp_prims = build_device_params(self.robot, self.env.dim, self.obstacle_cutoff_margin, None, None, costs,
                                                           [1.0] * len(costs), True, 128, True, 1.0, device)
            self._gp_grids = self._gp.grids_tensor   # (None without a grid field) kept alive next to the primitive table
        return self._gp

    def refresh_grids(self):
        """after GridSDF.update_occupancy / update_mesh: copy the planes again where the metrics' grid buffer is a concatenation (guides.refresh_grid_planes)"""
        from .guides import refresh_grid_planes
        if getattr(self, "_gp", None) is not None:
            refresh_grid_planes(self._gp)
        for gp, _prims in self.__dict__.get("_gp_by_h", {}).values():   # a task with a track: one block per horizon, each with a grid buffer of its own
            refresh_grid_planes(gp)

    def trajectory_metrics(self, trajs, n_check=None, return_mask=False, static_only=False):
        """trajs: UNNORMALISED [B,H,D] on the GPU -> float tensor [B,4]: (#colliding waypoints, path length, smoothness,
        #waypoints checked); with return_mask also the per-waypoint collision flags [B, n_check] (bool) the count is made of.
        A task with a moving obstacle checks every point against the obstacle's position at the point's own time (H must be the track's length:
        ValueError otherwise, before any device work); static_only leaves the moving fields out."""
        import ctypes as C
        if self.has_tracks and not static_only:   # (before any device work)
            for f in self.get_collision_fields():
                if field_track(f) is not None:
                    f.objects.track_rows(trajs.shape[1])
        trajs = trajs.to(torch.float32).contiguous()
        if not trajs.is_cuda:
            raise RuntimeError("trajectory metrics run on the GPU (libmpdx); there is no CPU fallback")
        B, H, D = trajs.shape
        n_check = int(n_check or 4 * H)
        out = torch.empty((B, 4), dtype=torch.float32, device=trajs.device)
        mask = torch.empty((B, n_check), dtype=torch.uint8, device=trajs.device) if return_mask else None
        gp = self._params(trajs.device, H, static_only) if self.has_tracks else self._params(trajs.device)
        _lib.check(_lib.load().mpdx_traj_metrics_mask(C.byref(gp), trajs.data_ptr(), out.data_ptr(), mask.data_ptr() if return_mask else None,
                                                      n_check, B, H, D, _lib.current_stream()), "mpdx_traj_metrics_mask")
        return (out, mask.bool()) if return_mask else out

    def tool_axis_metrics(self, trajs, cost, n_check=None, return_mask=False):
        """trajs: UNNORMALISED [B,H,D] on the GPU, cost: a CostToolAxis of this task's robot -> (max_tilt [B] in radians = acos(clamp(min_i d_i)),
        n_violating [B] = checked points tilted by more than cost.max_tilt) over n_check interpolated points (default 4 H); with return_mask also
        the per-point flags [B, n_check] (bool).  mpdx_traj_tool_metrics (csrc/chain.hpp::traj_tool_chain_kernel)."""
        import ctypes as C
        if not isinstance(cost, CostToolAxis):
            raise TypeError("cost: a CostToolAxis is expected")
        if cost.robot is not self.robot:
            raise ValueError("the CostToolAxis was built for another robot than this task's")
        trajs = trajs.to(torch.float32).contiguous()
        if not trajs.is_cuda:
            raise RuntimeError("tool-axis metrics run on the GPU (libmpdx); there is no CPU fallback")
        B, H, D = trajs.shape
        n_check = int(n_check or 4 * H)
        from .guides import build_device_params
        gp, _keep = build_device_params(self.robot, self.env.dim, self.obstacle_cutoff_margin, None, None, [cost], [1.0], True, 128, True, 1.0, trajs.device)
        out = torch.empty((B, 2), dtype=torch.float32, device=trajs.device)
        mask = torch.empty((B, n_check), dtype=torch.uint8, device=trajs.device) if return_mask else None
        _lib.check(_lib.load().mpdx_traj_tool_metrics(C.byref(gp), trajs.data_ptr(), out.data_ptr(), mask.data_ptr() if return_mask else None,
                                                      n_check, B, H, D, _lib.current_stream()), "mpdx_traj_tool_metrics")
        tilt, n_bad = torch.acos(out[:, 0].clamp(-1.0, 1.0)), out[:, 1]
        return (tilt, n_bad, mask.bool()) if return_mask else (tilt, n_bad)

    def trajectory_costs(self, trajs, cost, n_points=None, return_clearance=False, return_point_costs=False):
        """trajs: UNNORMALISED [B,H,D] on the GPU; cost: a CostComposite of this task's robot, or one of its terms (wrapped with weight 1) -> a
        TrajectoryCosts: the unweighted value of every term in the order of cost.cost_l, their weighted total and - on request - the clearance per
        collision field and the factor sums per evaluated point.  The collision and tool terms are evaluated on n_points points of the guide's linear
        interpolation (default 4 H; H gives the supports), the GP prior on the supports.  mpdx_traj_costs (csrc/costs.hpp::traj_costs_kernel).
        A task with a moving obstacle needs H to be the track's length (ValueError before any device work)."""
        trajs, comp = _costs_arguments(self, trajs, cost)
        H = trajs.shape[1]
        n_points = int(n_points or 4 * H)
        from .guides import build_device_params
        gp, _keep = build_device_params(self.robot, self.env.dim, self.obstacle_cutoff_margin, None, None, comp.cost_l, comp.weight_cost_l, True, 128, True,
                                        1.0, trajs.device)
        return TrajectoryCosts.from_slots(comp, *launch_traj_costs(gp, trajs, n_points, return_clearance, return_point_costs))

    def get_trajs_collision_and_free(self, trajs, return_indices=False, **kw):
        m = self.trajectory_metrics(trajs)
        coll = m[:, 0] > 0
        idx_c, idx_f = torch.nonzero(coll).flatten(), torch.nonzero(~coll).flatten()
        tc = trajs[idx_c] if idx_c.numel() else None
        tf = trajs[idx_f] if idx_f.numel() else None
        if return_indices:
            return tc, idx_c, tf, idx_f, None
        return tc, tf

    def compute_fraction_free_trajs(self, trajs, **kw):
        m = self.trajectory_metrics(trajs)
        return float((m[:, 0] == 0).float().mean())

    def compute_collision_intensity_trajs(self, trajs, **kw):
        m = self.trajectory_metrics(trajs)
        return float((m[:, 0] / m[:, 3]).mean())

    def compute_success_free_trajs(self, trajs, **kw):
        return int(self.compute_fraction_free_trajs(trajs) > 0)

    def random_coll_free_q(self, n_samples=1, max_tries=1000, device="cuda", generator=None):
        """uniform collision-free configurations (inference.py:161)."""
        lo, hi = self.q_limits(device)
        got = []
        for _ in range(max_tries):
            q = lo + (hi - lo) * torch.rand((4 * n_samples, self.robot.q_dim), device=device, generator=generator)
            traj = torch.cat([q, torch.zeros_like(q)], -1)[:, None, :].expand(-1, 2, -1).contiguous()
            free = self.trajectory_metrics(traj, n_check=2, static_only=True)[:, 0] == 0
            got.append(q[free])
            if sum(g.shape[0] for g in got) >= n_samples:
                return torch.cat(got)[:n_samples]
        raise ValueError("No collision free configuration was found")

    def ik_coll_free_q(self, target_pos, target_rot=None, n_samples=1, dedup_distance=0.05, device="cuda", **ik_kwargs):
        """Collision-free configurations that place the robot's frame at an end-effector target (an extension; ik.solve_ik, whose keyword
        arguments pass through: frame, offset, n_restarts, seed, ...).  The converged restarts are filtered as random_coll_free_q filters
        (metrics kernel, n_check=2), sorted by position error and thinned so that no two returned configurations lie within `dedup_distance`
        (joint-space L2); at most n_samples rows [k, q_dim] come back.  target_pos [3], target_rot None or [3, 3]."""
        from .ik import solve_ik
        if torch.as_tensor(target_pos).numel() != 3:
            raise ValueError("ik_coll_free_q takes one target: target_pos [3]")
        res = solve_ik(self.robot, torch.as_tensor(target_pos).reshape(3), None if target_rot is None else torch.as_tensor(target_rot).reshape(3, 3),
                       device=device, **ik_kwargs)
        q, perr = res.q[res.converged], res.pos_err[res.converged]
        if q.shape[0]:
            traj = torch.cat([q, torch.zeros_like(q)], -1)[:, None, :].expand(-1, 2, -1).contiguous()
            free = self.trajectory_metrics(traj, n_check=2, static_only=True)[:, 0] == 0
            q, perr = q[free], perr[free]
        if not q.shape[0]:
            raise ValueError("No collision free configuration reaches the target")
        q = q[torch.argsort(perr)]
        qc, keep = q.cpu(), []
        for i in range(qc.shape[0]):
            if all(float(torch.linalg.norm(qc[i] - qc[k])) > dedup_distance for k in keep):
                keep.append(i)
                if len(keep) >= n_samples:
                    break
        return q[torch.tensor(keep, device=q.device)]

    def q_limits(self, device="cpu"):
        if isinstance(self.robot, RobotChain):
            return torch.tensor(self.robot.q_limits[0], device=device), torch.tensor(self.robot.q_limits[1], device=device)
        lo, hi = syn.limits_for(self.robot.name if self.robot.q_dim != 3 else "RobotPointMass3D")
        qd = self.robot.q_dim
        if self.robot.name == "RobotPointMass":
            lo, hi = np.concatenate([self.ws_min, lo[qd:]]), np.concatenate([self.ws_max, hi[qd:]])
        return torch.tensor(lo[:qd], device=device), torch.tensor(hi[:qd], device=device)


def field_track(f):
    """the track of a collision field's ObjectSet, or None (the field does not move)"""
    return getattr(getattr(f, "objects", None), "track", None) if getattr(f, "kind", None) == _lib.FIELD_OBJECTS else None


def _check_object_set(o, dim, what):
    """An ObjectSet as the primitive tables need it: [n, 3] centres (unused axes zero), [n] positive radii, [n, 3] positive half extents."""
    if not isinstance(o, ObjectSet):
        raise TypeError(f"{what}: an ObjectSet is expected, got {type(o).__name__}")
    sc, sr, bc, bh = (np.asarray(a, np.float32) for a in (o.sphere_centers, o.sphere_radii, o.box_centers, o.box_half))
    if sc.ndim != 2 or sc.shape[1] != 3 or bc.ndim != 2 or bc.shape[1] != 3 or bh.shape != bc.shape or sr.shape != (sc.shape[0],):
        raise ValueError(f"{what}: sphere_centers [n, 3], sphere_radii [n], box_centers / box_half [m, 3] (rows padded to 3-D) are expected, got "
                         f"{sc.shape}, {sr.shape}, {bc.shape}, {bh.shape}")
    if not (np.isfinite(sc).all() and np.isfinite(sr).all() and np.isfinite(bc).all() and np.isfinite(bh).all()):
        raise ValueError(f"{what}: non-finite primitive")
    if (sr <= 0).any() or (bh <= 0).any():
        raise ValueError(f"{what}: radii and half extents must be positive")
    if dim < 3 and (np.abs(sc[:, dim:]).max(initial=0.0) > 0 or np.abs(bc[:, dim:]).max(initial=0.0) > 0):
        raise ValueError(f"{what}: a primitive of a {dim}-D workspace has a centre off the unused axes (wrong dimension)")


class PlanningScenes:
    """Several obstacle scenes of ONE task, for contexts that are planned and evaluated in one batch (an extension: the reference builds one
    PlanningTask per run_inference call, inference.py:107-123).  Scene s is `task` with its extra-objects field replaced by `extra_objects[s]`
    (an empty ObjectSet is a scene without extra obstacles) and, if `fixed_objects` is given, its fixed-objects field by `fixed_objects[s]`.
    Workspace limits, the robot, the self-collision field and a signed-distance grid are the same in every scene (a grid stands for the fixed
    environment: `fixed_objects` with a grid task raises ValueError).

    The guide takes scenes through `GuideManagerTrajectoriesWithVelocity.with_scenes(scenes, scene_of_context, n_per_context)`, the metrics through
    the methods below, which take the assignment per call: `scene_of_context[c]` is the scene of the c-th group of `n_per_context` consecutive
    trajectories.  Both run the MULTI_SCENE instantiations of the HIP guide / metrics kernels on one blocked primitive table
    (guides.build_device_params(scenes=...), layout in include/mpdx.h)."""

    def __init__(self, task: PlanningTask, extra_objects, fixed_objects=None):
        if task.df_collision_extra_objects is None:
            raise ValueError("PlanningScenes replaces the task's extra-objects field: build the task with use_extra_objects=True")
        if task.has_tracks:
            raise ValueError("the task has a moving obstacle (a track): scene batches and tracks do not combine (the kernels have no instantiation for both)")
        extra_objects = list(extra_objects)
        if not extra_objects:
            raise ValueError("at least one scene")
        dim = task.env.dim
        for s, o in enumerate(extra_objects):
            _check_object_set(o, dim, f"extra_objects[{s}]")
            if o.track is not None:
                raise ValueError(f"extra_objects[{s}] carries a track: scene batches and tracks do not combine")
        if fixed_objects is not None:
            if task.df_collision_objects.kind == _lib.FIELD_GRID:
                raise ValueError("the task's fixed field is a signed-distance grid, which every scene shares: fixed_objects cannot replace it")
            fixed_objects = list(fixed_objects)
            if len(fixed_objects) != len(extra_objects):
                raise ValueError(f"{len(fixed_objects)} fixed object sets for {len(extra_objects)} scenes")
            for s, o in enumerate(fixed_objects):
                _check_object_set(o, dim, f"fixed_objects[{s}]")
                if o.track is not None:
                    raise ValueError(f"fixed_objects[{s}] carries a track: scene batches and tracks do not combine")
        self.task, self.extra_objects, self.fixed_objects = task, extra_objects, fixed_objects
        self._gp = None
        # sizes: what a workgroup stages must fit the kernels' table budget (the same rule the launchers apply)
        staged = _lib.SCENE_HEADER_WORDS
        for sets in (extra_objects, fixed_objects):
            if sets is not None:
                staged += 4 * max(len(o.sphere_radii) for o in sets) + 6 * max(len(o.box_centers) for o in sets)
        if fixed_objects is None and task.df_collision_objects.kind == _lib.FIELD_OBJECTS:
            o = task.df_collision_objects.objects
            staged += 4 * len(o.sphere_radii) + 6 * len(o.box_centers)
        if staged + 3 > _lib.SCENE_MAX_STAGED_FLOATS:
            raise ValueError(f"a scene needs {staged} table floats; the kernels stage at most {_lib.SCENE_MAX_STAGED_FLOATS}")

    @property
    def n_scenes(self) -> int:
        return len(self.extra_objects)

    def objects_for(self, field):
        """The per-scene ObjectSets that stand for `field` of the task (None: the field is the same in every scene)."""
        if field is self.task.df_collision_extra_objects:
            return self.extra_objects
        if self.fixed_objects is not None and field is self.task.df_collision_objects:
            return self.fixed_objects
        return None

    def scene_task(self, s: int) -> PlanningTask:
        """Scene s as a single-scene PlanningTask (what one call per scene would use; the tests' reference)."""
        import copy
        t = copy.copy(self.task)
        t._gp = None
        t.df_collision_extra_objects = CollisionField(_lib.FIELD_OBJECTS, objects=self.extra_objects[s], name="extra_objects")
        if self.fixed_objects is not None:
            t.df_collision_objects = CollisionField(_lib.FIELD_OBJECTS, objects=self.fixed_objects[s], name="objects")
        return t

    def check_assignment(self, scene_of_context, n_trajs, n_per_context):
        """scene_of_context as a host int list, validated against the scenes and the batch: one entry per context, each in [0, n_scenes)."""
        npc = int(n_per_context)
        if npc <= 0:
            raise ValueError(f"n_per_context={n_per_context}")
        soc = [int(v) for v in (scene_of_context.tolist() if hasattr(scene_of_context, "tolist") else scene_of_context)]
        if n_trajs is not None:
            if n_trajs % npc:
                raise ValueError(f"{n_trajs} trajectories are not a multiple of n_per_context={npc}")
            if len(soc) != n_trajs // npc:
                raise ValueError(f"scene_of_context has {len(soc)} entries for {n_trajs // npc} contexts of {npc} trajectories")
        bad = [v for v in soc if not 0 <= v < self.n_scenes]
        if bad:
            raise ValueError(f"scene_of_context entries {bad} outside [0, {self.n_scenes})")
        return soc

    @staticmethod
    def bind(gp, scene_of_context, n_per_context, device):
        """A copy of the parameter block `gp` bound to one assignment: (params, device index table - keep it alive as long as the params)."""
        table = torch.tensor(scene_of_context, dtype=torch.int32, device=device)
        out = type(gp).from_buffer_copy(gp)
        out.scene_of_ctx, out.scene_n_per_ctx = table.data_ptr(), int(n_per_context)
        return out, table

    def _params(self, device):
        if self._gp is None or self._gp_prims.device != torch.device(device):
            from .guides import build_device_params
            costs = [CostCollision(self.task.robot, 64, field=f) for f in self.task.get_collision_fields()]
            self._gp, self._gp_prims = build_device_params(self.task.robot, self.task.env.dim, self.task.obstacle_cutoff_margin, None, None, costs,
                                                           [1.0] * len(costs), True, 128, True, 1.0, device, scenes=self)
            self._gp_grids = self._gp.grids_tensor
        return self._gp

    # ---- the metrics of PlanningTask with a scene per context; arithmetic in csrc/guide.hpp::traj_metrics_kernel<..., MULTI_SCENE>
    def trajectory_metrics(self, trajs, scene_of_context, n_per_context, n_check=None, return_mask=False):
        """PlanningTask.trajectory_metrics where the c-th group of n_per_context trajectories is checked against scene scene_of_context[c]."""
        import ctypes as C
        trajs = trajs.to(torch.float32).contiguous()
        if not trajs.is_cuda:
            raise RuntimeError("trajectory metrics run on the GPU (libmpdx); there is no CPU fallback")
        B, H, D = trajs.shape
        soc = self.check_assignment(scene_of_context, B, n_per_context)
        n_check = int(n_check or 4 * H)
        out = torch.empty((B, 4), dtype=torch.float32, device=trajs.device)
        mask = torch.empty((B, n_check), dtype=torch.uint8, device=trajs.device) if return_mask else None
        gp, table = self.bind(self._params(trajs.device), soc, n_per_context, trajs.device)
        _lib.check(_lib.load().mpdx_traj_metrics_mask(C.byref(gp), trajs.data_ptr(), out.data_ptr(), mask.data_ptr() if return_mask else None,
                                                      n_check, B, H, D, _lib.current_stream()), "mpdx_traj_metrics_mask")
        table.record_stream(torch.cuda.current_stream())   # (the launch is asynchronous: the allocator must not hand the table out before it ran)
        return (out, mask.bool()) if return_mask else out

    def trajectory_costs(self, trajs, cost, scene_of_context, n_per_context, n_points=None, return_clearance=False, return_point_costs=False):
        """PlanningTask.trajectory_costs where the c-th group of n_per_context trajectories is evaluated against scene scene_of_context[c] (the
        collision terms of `cost` name the task's fields, as the guide's do)."""
        trajs, comp = _costs_arguments(self.task, trajs, cost)
        B, H, _ = trajs.shape
        soc = self.check_assignment(scene_of_context, B, n_per_context)
        n_points = int(n_points or 4 * H)
        from .guides import build_device_params
        gp0, _keep = build_device_params(self.task.robot, self.task.env.dim, self.task.obstacle_cutoff_margin, None, None, comp.cost_l, comp.weight_cost_l,
                                         True, 128, True, 1.0, trajs.device, scenes=self)
        gp, table = self.bind(gp0, soc, n_per_context, trajs.device)
        raw = launch_traj_costs(gp, trajs, n_points, return_clearance, return_point_costs)
        table.record_stream(torch.cuda.current_stream())   # (the launch is asynchronous: the allocator must not hand the table out before it ran)
        return TrajectoryCosts.from_slots(comp, *raw)

    def get_trajs_collision_and_free(self, trajs, scene_of_context, n_per_context, return_indices=False, **kw):
        m = self.trajectory_metrics(trajs, scene_of_context, n_per_context)
        coll = m[:, 0] > 0
        idx_c, idx_f = torch.nonzero(coll).flatten(), torch.nonzero(~coll).flatten()
        tc = trajs[idx_c] if idx_c.numel() else None
        tf = trajs[idx_f] if idx_f.numel() else None
        if return_indices:
            return tc, idx_c, tf, idx_f, None
        return tc, tf

    def compute_fraction_free_trajs(self, trajs, scene_of_context, n_per_context, **kw):
        m = self.trajectory_metrics(trajs, scene_of_context, n_per_context)
        return float((m[:, 0] == 0).float().mean())

    def compute_collision_intensity_trajs(self, trajs, scene_of_context, n_per_context, **kw):
        m = self.trajectory_metrics(trajs, scene_of_context, n_per_context)
        return float((m[:, 0] / m[:, 3]).mean())


def task_from_torch_robotics(tr_task, tensor_args=None, use_extra_objects=True) -> PlanningTask:
    """Adapter: a REAL `torch_robotics.tasks.tasks.PlanningTask` (what `inference.py:161,181,191-201` builds) -> this package's `PlanningTask`, i.e. the
    primitive tables the guide / metrics kernels read.  torch_robotics is an empty submodule in the reference checkout (`deps/torch_robotics`,
    `.gitmodules:7-9`), so the attribute names below are the published package's AS RECALLED and cannot be exercised here against the real classes
    (tests/test_adapter_cpu.py drives it with stand-in objects of the same shape); every attribute read is listed, and a missing one raises
    AttributeError naming it instead of guessing:

      tr_task.env                      EnvBase:  .name (str, optional), .dim (2 | 3), .limits ([2, dim] tensor: workspace min / max)
      tr_task.env.obj_fixed_list       [ObjectField]  - the environment's own obstacles
      tr_task.env.obj_extra_list       [ObjectField] or None - `use_extra_objects=True` obstacles (inference.py:109)
        ObjectField.fields             [primitive fields]; ObjectField.pos (optional [dim] offset added to every centre; rotations are NOT supported: a
                                       non-identity ObjectField.ori raises)
          MultiSphereField             .centers [n, dim], .radii [n]
          MultiBoxField                .centers [n, dim], .sizes [n, dim] (FULL edge lengths; halved here) - or .half_sizes [n, dim]
      tr_task.robot                    .name ('RobotPointMass' | 'RobotPanda' | ...), .q_dim; RobotPointMass: .link_margins_for_object_collision_checking
                                       ([margin]) or .link_margin
      tr_task.obstacle_cutoff_margin   float (inference.py:110)

          GridMapSDF                       .sdf_tensor ([nx, ny(, nz)] node values, indexed as sdf_tensor[ix, iy(, iz)]), .grad_sdf_tensor (the same
                                           shape + [dim]), .limits ([2, dim]: the position of node 0 and of the last node), .cell_size (float or [dim]
                                           with equal entries) - AS RECALLED, all four needed: it becomes a `GridSDF` in 'nearest' mode (the recalled
                                           lookup: value and stored gradient of the node round((p - limits[0]) / cell_size)) with origin = limits[0].
                                           One grid per objects list, and not next to primitives in the same list (NotImplementedError).

    A field that is neither (a mesh, a grid object without that full surface) has no primitive form: it raises NotImplementedError.
    The arithmetic on the tables (hinge on the SDF, FK, interpolation) is this package's restatement (parity unpinned)."""
    def need(obj, *names):
        for n in names:
            if hasattr(obj, n) and getattr(obj, n) is not None:
                return getattr(obj, n)
        raise AttributeError(f"{type(obj).__name__} has none of the attributes {names} the adapter reads (see task_from_torch_robotics.__doc__)")

    def arr(v, cols=None):
        a = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, np.float32)
        return a.reshape(-1, cols) if cols else a.reshape(-1)

    env_t = need(tr_task, "env")
    dim = int(need(env_t, "dim"))
    if dim not in (2, 3):
        raise NotImplementedError(f"workspace dimension {dim}")

    GRID_ATTRS = ("sdf_tensor", "grad_sdf_tensor", "limits", "cell_size")

    def grid_of(f):
        sdf, grad = need(f, "sdf_tensor"), need(f, "grad_sdf_tensor")
        sdf, grad = torch.as_tensor(sdf).detach().cpu().float(), torch.as_tensor(grad).detach().cpu().float()
        if sdf.dim() != dim or tuple(grad.shape) != tuple(sdf.shape) + (dim,):
            raise NotImplementedError(f"GridMapSDF: sdf_tensor {tuple(sdf.shape)} / grad_sdf_tensor {tuple(grad.shape)} for a {dim}-D workspace")
        cs = np.unique(arr(need(f, "cell_size")))
        if cs.size != 1:
            raise NotImplementedError("GridMapSDF with per-axis cell sizes: the grid field has one cubic cell")
        lim = arr(need(f, "limits"), dim)
        perm = tuple(reversed(range(dim)))    # [ix, iy(, iz)] -> [(iz,) iy, ix]: x fastest
        return GridSDF(sdf.permute(*perm).contiguous(), lim[0].copy(), float(cs[0]), mode="nearest", grad=grad.permute(*perm, dim).contiguous())

    grids = {}

    def object_set(obj_list, which="fixed"):
        sc, sr, bc, bh = [], [], [], []
        n_grid = sum(all(hasattr(f, a) for a in GRID_ATTRS) for obj in (obj_list or []) for f in need(obj, "fields"))
        n_all = sum(len(need(obj, "fields")) for obj in (obj_list or []))
        if n_grid:
            if n_grid != 1 or n_all != 1:
                raise NotImplementedError("one GridMapSDF per objects list, not mixed with primitive fields in the same list")
            obj = [o for o in obj_list if len(o.fields)][0]
            if getattr(obj, "pos", None) is not None and np.abs(arr(obj.pos)).max() > 0:
                raise NotImplementedError("a GridMapSDF under a shifted ObjectField")
            grids[which] = grid_of(obj.fields[0])
            return ObjectSet.empty()
        for obj in (obj_list or []):
            ori = getattr(obj, "ori", None)
            if ori is not None:
                o = arr(ori)
                ident = (o.size == 4 and abs(abs(o[0]) - 1.0) < 1e-6 and np.abs(o[1:]).max() < 1e-6) or (o.size == 9 and np.abs(o.reshape(3, 3) - np.eye(3)).max() < 1e-6) \
                    or np.abs(o).max() < 1e-12
                if not ident:
                    raise NotImplementedError("rotated ObjectField: the primitive tables hold axis-aligned boxes")
            off = arr(obj.pos)[:dim] if getattr(obj, "pos", None) is not None else np.zeros(dim, np.float32)
            for f in need(obj, "fields"):
                kind = type(f).__name__
                if hasattr(f, "radii"):
                    c = arr(need(f, "centers"), dim) + off
                    sc.append(_pad3(c, dim)); sr.append(arr(f.radii))
                elif hasattr(f, "sizes") or hasattr(f, "half_sizes"):
                    c = arr(need(f, "centers"), dim) + off
                    h = arr(f.half_sizes, dim) if getattr(f, "half_sizes", None) is not None else 0.5 * arr(f.sizes, dim)
                    hp = np.concatenate([h, np.full((h.shape[0], 3 - dim), 1.0, np.float32)], 1)   # 2-D boxes are unbounded along the unused axis
                    bc.append(_pad3(c, dim)); bh.append(hp)
                else:
                    raise NotImplementedError(f"{kind}: only sphere (.centers, .radii) and box (.centers, .sizes) primitive fields have a table form")
        z = ObjectSet.empty()
        return ObjectSet(np.concatenate(sc) if sc else z.sphere_centers, np.concatenate(sr) if sr else z.sphere_radii,
                         np.concatenate(bc) if bc else z.box_centers, np.concatenate(bh) if bh else z.box_half)

    env = Env(str(getattr(env_t, "name", type(env_t).__name__)), dim, object_set(need(env_t, "obj_fixed_list")),
              object_set(getattr(env_t, "obj_extra_list", None), "extra"))
    if "extra" in grids:
        raise NotImplementedError("a GridMapSDF among the EXTRA objects: the grid field stands for the fixed objects")
    env.grid_fixed = grids.get("fixed")
    lim = arr(need(env_t, "limits"), dim)
    env.limits = (lim[0].copy(), lim[1].copy())
    rob_t = need(tr_task, "robot")
    rname = str(getattr(rob_t, "name", type(rob_t).__name__))
    if "Panda" in rname:
        robot = RobotPanda()
    elif "PointMass" in rname:
        margin = getattr(rob_t, "link_margins_for_object_collision_checking", None)
        margin = float(arr(margin)[0]) if margin is not None else float(getattr(rob_t, "link_margin", 0.01))
        robot = RobotPointMass(int(need(rob_t, "q_dim")), margin)
    else:
        raise NotImplementedError(f"robot {rname!r}: the kernels know the point mass (2-D / 3-D) and the Panda")
    return PlanningTask(env, robot, obstacle_cutoff_margin=float(need(tr_task, "obstacle_cutoff_margin")), use_extra_objects=use_extra_objects,
                        tensor_args=tensor_args)


def compute_smoothness(trajs, robot, task=None):
    """sum_h |v_{h+1} - v_h| per trajectory (torch_robotics.trajectory.metrics.compute_smoothness, restated)."""
    v = robot.get_velocity(trajs)
    return torch.linalg.norm(torch.diff(v, dim=-2), dim=-1).sum(-1)


def compute_path_length(trajs, robot):
    q = robot.get_position(trajs)
    return torch.linalg.norm(torch.diff(q, dim=-2), dim=-1).sum(-1)


def compute_variance_waypoints(trajs, robot, definition="position_variance"):
    """Diversity of a batch of trajectories, summed over the waypoints (torch_robotics.trajectory.metrics.compute_variance_waypoints,
    un-vendored: restated; the definition is undecidable from the reference tree, so both plausible ones are offered):
      'position_variance' (default): sum_h sum_j Var_b[q_{b,h,j}]  (unbiased variance of each coordinate across the batch)
      'pairwise_distance'          : sum_h Var over unordered trajectory pairs of |q_{a,h} - q_{b,h}|  (SURVEY.md A20's recollection)"""
    q = robot.get_position(trajs)
    if q.shape[0] < 2:
        return 0.0
    if definition == "position_variance":
        return float(q.var(dim=0).sum(-1).sum())
    if definition == "pairwise_distance":
        B = q.shape[0]
        ia, ib = torch.triu_indices(B, B, offset=1, device=q.device)
        d = torch.linalg.norm(q[ia] - q[ib], dim=-1)     # [pairs, H]
        return float(d.var(dim=0).sum()) if d.shape[0] > 1 else 0.0
    raise ValueError(definition)


# ------------------------------------------------------------------------------------------------ cost descriptors


class CostCollision:
    def __init__(self, robot, n_support_points, field=None, sigma_coll=1.0, tensor_args=None, **kw):
        if sigma_coll != 1.0:
            raise NotImplementedError("sigma_coll != 1 (inference.py:201 always passes 1.0)")
        self.robot, self.n_support_points, self.field = robot, n_support_points, field


class CostGPTrajectory:
    """half_factor (extension, default False): whether the GP cost carries GPMP2's 1/2 (1/2 sum e^T Qinv e).  The reference's
    implementation lives in an empty submodule, so the convention is undecidable here; it only matters where the per-waypoint
    gradient norm is below max_grad_norm."""

    def __init__(self, robot, n_support_points, dt, sigma_gp=1.0, tensor_args=None, half_factor=False, **kw):
        self.robot, self.n_support_points, self.dt, self.sigma_gp = robot, n_support_points, float(dt), float(sigma_gp)
        self.half_factor = bool(half_factor)


class CostToolAxis:
    """Tool-axis constraint of a chain robot along the whole trajectory ("carry it upright"; an extension: the reference has no task-space
    cost).  On every interpolated point the unit axis `axis` of frame `frame` (1 ... n_joints, default the last), rotated into the world, is held
    within `max_tilt` radians of the unit world axis `world_axis`:  cost = sum_i relu(cos(max_tilt) - world_axis . Rot_frame(q_i) axis).
    The arithmetic and its gradient are stated in include/mpdx.h (the tool members of mpdx_guide_params).  Both axes are normalised here, in float64.
    At a tilt of exactly pi the gradient vanishes (the axis points exactly the other way: a saddle); nothing works around it.
    The baseline planners (RRT-Connect, GPMP2) do not honour the constraint; there is no position constraint and no training-time use."""

    def __init__(self, robot, n_support_points, frame=None, axis=(0, 0, 1), world_axis=(0, 0, 1), max_tilt=0.1, tensor_args=None):
        if not isinstance(robot, RobotChain):
            raise ValueError(f"CostToolAxis needs a RobotChain, got {getattr(robot, 'name', type(robot).__name__)}: the Panda takes it as RobotChain.panda()")
        frame = robot.q_dim if frame is None else frame
        if isinstance(frame, (bool, float)) or int(frame) != frame or not 1 <= int(frame) <= robot.q_dim:
            raise ValueError(f"frame {frame!r} outside 1 ... n_joints ({robot.q_dim})")
        unit = []
        for what, v in (("axis", axis), ("world_axis", world_axis)):
            a = np.asarray(v, np.float64).reshape(-1)
            if a.shape != (3,) or not np.isfinite(a).all() or not np.linalg.norm(a) > 0:
                raise ValueError(f"{what} must be a finite non-zero 3-vector, got {v!r}")
            unit.append(a / np.linalg.norm(a))
        max_tilt = float(max_tilt)
        if not 0.0 <= max_tilt <= math.pi:
            raise ValueError(f"max_tilt {max_tilt!r} outside [0, pi] radians")
        self.robot, self.n_support_points, self.frame = robot, n_support_points, int(frame)
        self.axis, self.world_axis, self.max_tilt = unit[0], unit[1], max_tilt

    @property
    def cos_min(self) -> float:
        return math.cos(self.max_tilt)


class CostComposite:
    def __init__(self, robot, n_support_points, cost_list, weights_cost_l=None, tensor_args=None, **kw):
        self.robot, self.n_support_points = robot, n_support_points
        self.cost_l = list(cost_list)
        self.weight_cost_l = list(weights_cost_l) if weights_cost_l is not None else [1.0] * len(self.cost_l)
        if len(self.cost_l) != len(self.weight_cost_l):
            raise ValueError("one weight per cost term")


# ------------------------------------------------------------------------------------------------ cost values (mpdx_traj_costs)


def as_cost_composite(cost) -> CostComposite:
    """`cost` itself if it is a CostComposite; a single term wrapped with weight 1; TypeError for anything else"""
    if isinstance(cost, CostComposite):
        return cost
    if isinstance(cost, (CostCollision, CostGPTrajectory, CostToolAxis)):
        return CostComposite(cost.robot, cost.n_support_points, [cost], weights_cost_l=[1.0])
    raise TypeError(f"cost: a CostComposite or one of its terms is expected, got {type(cost).__name__}")


def cost_term_slots(cost_l):
    """(names, slots) of the terms of a composite in the order of cost_l: a collision term is named after its field and takes the next of the slots
    0 ... MPDX_MAX_FIELDS - 1 (the order build_device_params fills fields[] in), the GP prior 'gp' slot MPDX_MAX_FIELDS, the tool-axis term 'tool_axis'
    the slot behind it (the layout of mpdx_traj_costs' cost_out)."""
    names, slots, nf = [], [], 0
    for c in cost_l:
        if isinstance(c, CostCollision):
            names.append(getattr(c.field, "name", "") or f"field{nf}")
            slots.append(nf)
            nf += 1
        elif isinstance(c, CostGPTrajectory):
            names.append("gp")
            slots.append(_lib.MAX_FIELDS)
        elif isinstance(c, CostToolAxis):
            names.append("tool_axis")
            slots.append(_lib.MAX_FIELDS + 1)
        else:
            raise NotImplementedError(type(c))
    if nf > _lib.MAX_FIELDS:
        raise NotImplementedError(f"at most {_lib.MAX_FIELDS} collision fields")
    return names, slots


@dataclass
class TrajectoryCosts:
    """The values of a cost composite on a batch of trajectories (PlanningTask.trajectory_costs, GuideManagerTrajectoriesWithVelocity.costs): what the
    reference's cost(x, x_interpolated=..., return_invidual_costs_and_weights=True) returns, plus how close each trajectory comes to each field."""
    names: List[str]                               # the terms in the order of cost.cost_l: field names, 'gp', 'tool_axis'
    weights: torch.Tensor                          # [n_terms] the composite's weights
    terms: torch.Tensor                            # [B, n_terms] UNWEIGHTED term values
    total: torch.Tensor                            # [B] = terms @ weights
    clearance: Optional[torch.Tensor] = None       # [B, n_collision_terms]: smallest distance less the link radius per field (negative: it collides)
    point_costs: Optional[torch.Tensor] = None     # [B, n_points, n_collision_terms (+ 1 with a tool term)]: the unweighted factor sum per evaluated point

    @property
    def min_clearance(self):
        """[B] the smallest clearance over the collision terms (None without return_clearance, or without a collision term)"""
        if self.clearance is None or self.clearance.shape[-1] == 0:
            return None
        return self.clearance.amin(-1)

    @classmethod
    def from_slots(cls, comp: CostComposite, cost_raw, clearance_raw=None, point_raw=None):
        """From the raw outputs of mpdx_traj_costs: cost_raw [B, MPDX_COST_SLOTS], clearance_raw [B, MPDX_MAX_FIELDS] or None, point_raw
        [B, n_points, MPDX_MAX_FIELDS + 1] or None - the slots picked and ordered as comp.cost_l lists the terms."""
        names, slots = cost_term_slots(comp.cost_l)
        idx = torch.tensor(slots, dtype=torch.long, device=cost_raw.device)
        terms = cost_raw.index_select(-1, idx)
        weights = torch.tensor([float(w) for w in comp.weight_cost_l], dtype=terms.dtype, device=terms.device)
        coll = [s for s in slots if s < _lib.MAX_FIELDS]     # (ascending: the collision terms take the slots in their order)
        cols = coll + ([_lib.MAX_FIELDS] if _lib.MAX_FIELDS + 1 in slots else [])
        clearance = clearance_raw[:, :len(coll)].contiguous() if clearance_raw is not None else None
        points = point_raw.index_select(-1, torch.tensor(cols, dtype=torch.long, device=point_raw.device)) if point_raw is not None else None
        return cls(names, weights, terms, terms @ weights, clearance, points)


def launch_traj_costs(gp, trajs, n_points, return_clearance=False, return_point_costs=False):
    """mpdx_traj_costs on UNNORMALISED float32 [B,H,D] GPU trajectories with the block gp; n_points = 0: the block's own points.  Returns the raw
    (cost [B, COST_SLOTS], clearance [B, MAX_FIELDS] or None, point costs [B, n_points, MAX_FIELDS + 1] or None)."""
    import ctypes as C
    B, H, D = trajs.shape
    n_eval = int(n_points) if n_points else (int(gp.n_interp) if gp.interpolate else H)
    cost = torch.empty((B, _lib.COST_SLOTS), dtype=torch.float32, device=trajs.device)
    clr = torch.empty((B, _lib.MAX_FIELDS), dtype=torch.float32, device=trajs.device) if return_clearance else None
    pts = torch.empty((B, max(n_eval, 0), _lib.MAX_FIELDS + 1), dtype=torch.float32, device=trajs.device) if return_point_costs else None
    _lib.check(_lib.load().mpdx_traj_costs(C.byref(gp), trajs.data_ptr(), cost.data_ptr(), _lib.ptr(clr), _lib.ptr(pts), int(n_points or 0), B, H, D,
                                           _lib.current_stream()), "mpdx_traj_costs")
    return cost, clr, pts


def _costs_arguments(task, trajs, cost):
    """the checks PlanningTask.trajectory_costs and PlanningScenes.trajectory_costs make before any device work; returns (trajs float32, composite)"""
    comp = as_cost_composite(cost)
    robot = task.robot
    for c in comp.cost_l:
        if not isinstance(c, (CostCollision, CostGPTrajectory, CostToolAxis)):
            raise TypeError(f"cost term {type(c).__name__}: CostCollision, CostGPTrajectory or CostToolAxis is expected")
        same_chain = isinstance(robot, RobotChain) and isinstance(c.robot, RobotChain) and c.robot.q_dim == robot.q_dim
        if c.robot is not robot and not same_chain:
            raise ValueError(f"the {type(c).__name__} term was built for another robot than this task's")
    cost_term_slots(comp.cost_l)
    if trajs.dim() != 3:
        raise ValueError(f"trajs: [B, H, D] is expected, got {tuple(trajs.shape)}")
    if task.has_tracks:   # (before any device work, as trajectory_metrics)
        for f in task.get_collision_fields():
            if field_track(f) is not None:
                f.objects.track_rows(trajs.shape[1])
    if not trajs.is_cuda:
        raise RuntimeError("trajectory costs run on the GPU (libmpdx); there is no CPU fallback")
    return trajs.to(torch.float32).contiguous(), comp
