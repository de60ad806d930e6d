"""GuideManagerTrajectoriesWithVelocity - drop-in for mpd/models/diffusion_models/guides.py:149-236.

Same constructor (incl. the `**kwargs` that swallows inference.py:234's misspelt `num_interpolated_points`, so the
effective number of interpolated points stays the class default 128) and the same call protocol
``guide(x_normalized[B,H,D]) -> increment[B,H,D]`` (already negated and weighted).  The cost composite is compiled
once into `mpdx_guide_params`; every call is one launch of the HIP guide kernel (csrc/guide.hpp).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .planning import CostCollision, CostComposite, CostGPTrajectory, CostToolAxis, GRID_MODES


def build_device_params(robot, ws_dim, cutoff_margin, mins, maxs, cost_l, weight_l, interpolate, n_interp, clip_grad, max_grad_norm, device,
                        clip_grad_rule="norm", max_grad_value=0.1, identity_normalizer=False, scenes=None):
    """Compile cost descriptors into the `mpdx_guide_params` block the HIP kernels take.  Returns (params, primitive
    table tensor) - the caller keeps the tensor alive (params holds its raw device pointer).  The planes of FIELD_GRID fields travel in a second
    buffer (global memory, not part of the primitive table the kernels stage in LDS): `params.grids_tensor` (None without a grid) holds it and
    lives as long as the params object; callers keep it next to the primitive table.
    scenes (a planning.PlanningScenes, or None = one scene, the table as before): the OBJECTS fields it varies get one table per scene - the blocked
    layout of include/mpdx.h (per-scene header + tables at the same offsets in every scene block, capacity = the largest scene, the other OBJECTS
    fields once in the shared tail).  n_scenes / scene_stride are set; the caller binds scene_of_ctx / scene_n_per_ctx per call
    (`params.table_host`: the host copy of the table, for tests).
    Moving obstacles: an OBJECTS field whose ObjectSet carries a `track` gets its [H, 4] rows packed behind the primitive tables (offset rounded up to
    a multiple of 4) and track_len / track_off of the field set; H is the cost's n_support_points (ValueError when the track has another number of
    rows, for a RobotChain and with scenes)."""
    gp = _lib.GuideParams()
    gp.robot, gp.q_dim, gp.ws_dim = robot.robot_id, robot.q_dim, ws_dim
    gp.interpolate, gp.n_interp = int(bool(interpolate)), int(n_interp)
    gp.clip_grad, gp.max_grad_norm = int(bool(clip_grad)), float(max_grad_norm)
    if clip_grad_rule not in ("norm", "value"):
        raise NotImplementedError(f"clip_grad_rule={clip_grad_rule!r}")   # as guides.py:219-220
    gp.clip_rule, gp.max_grad_value = (1 if clip_grad_rule == "value" else 0), float(max_grad_value)
    gp.identity_normalizer = int(identity_normalizer)   # 0 limits, 1 Identity, 2 GaussianNormalizer (means in `mins`, stds in `maxs`)
    D = 2 * robot.q_dim
    if mins is not None:
        mins, maxs = torch.as_tensor(mins).cpu().numpy(), torch.as_tensor(maxs).cpu().numpy()
        for d in range(D):
            gp.mins[d], gp.maxs[d] = float(mins[d]), float(maxs[d])
    gp.cutoff_margin, gp.link_margin = float(cutoff_margin), float(robot.link_margin)
    prims, nf, off = [], 0, 0
    tracks = []    # (field index, [H, 4] rows) of the OBJECTS fields that move
    varied = []    # scenes: (field index, [ObjectSet per scene]) of the fields that differ per scene
    shared = []    # scenes: (field index, sphere floats, box floats) of the OBJECTS fields every scene sees
    planes, goff = [], 0     # grid planes, each padded to a multiple of 4 floats (16-byte aligned gradient planes)
    placed = []              # (float offset in the grid buffer, plane) of the planes proper (refresh_grid_planes)
    gp.use_gp = 0
    for c, w in zip(cost_l, weight_l):
        if isinstance(c, CostCollision):
            if nf >= _lib.MAX_FIELDS:
                raise NotImplementedError(f"at most {_lib.MAX_FIELDS} collision fields")
            f, fld = gp.fields[nf], c.field
            f.kind, f.weight = fld.kind, float(w)
            per_scene = scenes.objects_for(fld) if scenes is not None else None
            if fld.kind == _lib.FIELD_OBJECTS and scenes is not None and getattr(fld.objects, "track", None) is not None:
                raise ValueError(f"field {fld.name!r} carries a track: scene batches and tracks do not combine")
            if fld.kind == _lib.FIELD_OBJECTS and scenes is not None:
                if per_scene is not None:
                    varied.append((nf, per_scene))
                else:
                    shared.append((nf,) + tuple(fld.objects.prim_floats()))
            elif fld.kind == _lib.FIELD_OBJECTS:
                if getattr(fld.objects, "track", None) is not None:
                    if robot.robot_id == _lib.ROBOT_CHAIN:
                        raise ValueError(f"field {fld.name!r} carries a track: a RobotChain takes no moving obstacles")
                    tracks.append((nf, fld.objects.track_rows(c.n_support_points)))
                sp, bx = fld.objects.prim_floats()
                f.sphere_off, f.n_spheres = off, sp.size // 4
                off += sp.size
                f.box_off, f.n_boxes = off, bx.size // 6
                off += bx.size
                prims += [sp, bx]
            elif fld.kind == _lib.FIELD_WORKSPACE:
                for j in range(ws_dim):
                    f.ws_min[j], f.ws_max[j] = float(fld.ws_min[j]), float(fld.ws_max[j])
            elif fld.kind == _lib.FIELD_GRID:
                g = fld.grid
                if g is None or g.dim != ws_dim:
                    raise ValueError(f"FIELD_GRID needs a GridSDF of the workspace dimension {ws_dim}")
                sdf_p, grad_p = g.planes(device)
                if g.mode == "nearest" and grad_p is None:
                    raise ValueError("GridSDF mode 'nearest' needs the gradient plane")
                f.mode, f.cell = GRID_MODES[g.mode], g.cell
                for j in range(3):
                    f.n[j] = g.shape[j] if j < ws_dim else 1
                    f.origin[j] = float(g.origin[j]) if j < ws_dim else 0.0
                f.grid_sdf_off, f.grid_grad_off = goff, -1
                for pl in (sdf_p, grad_p if g.mode == "nearest" else None):
                    if pl is None:
                        continue
                    if pl is grad_p:
                        f.grid_grad_off = goff
                    placed.append((goff, pl))
                    planes.append(pl)
                    goff += pl.numel()
                    if goff % 4:
                        planes.append(torch.zeros(4 - goff % 4, dtype=torch.float32, device=pl.device))
                        goff += planes[-1].numel()
            nf += 1
        elif isinstance(c, CostGPTrajectory):
            if gp.use_gp:
                raise NotImplementedError("one CostGPTrajectory term")
            gp.use_gp, gp.gp_weight, gp.dt, gp.sigma_gp = 1, float(w), float(c.dt), float(c.sigma_gp)
            gp.gp_half_factor = int(bool(getattr(c, "half_factor", False)))
        elif isinstance(c, CostToolAxis):   # the tool members at the end of the block (no entry of fields[]): frame, unit axes, cos(max_tilt), weight
            if gp.tool_frame:
                raise NotImplementedError("one CostToolAxis term")
            if c.robot is not robot and (robot.robot_id != _lib.ROBOT_CHAIN or c.robot.q_dim != robot.q_dim):
                raise ValueError("the CostToolAxis was built for another robot than the guide's")
            gp.tool_frame, gp.tool_cos_min, gp.tool_weight = c.frame, c.cos_min, float(w)
            for j in range(3):
                gp.tool_axis[j], gp.tool_world[j] = float(c.axis[j]), float(c.world_axis[j])
        else:
            raise NotImplementedError(type(c))
    gp.n_fields = nf
    if scenes is not None:
        table, n_floats = _scene_table(gp, scenes.n_scenes, varied, shared)
    else:
        for fi, rows in tracks:   # behind the tables, each at a multiple of 4 floats
            if off % 4:
                prims.append(np.zeros(4 - off % 4, np.float32))
                off += prims[-1].size
            gp.fields[fi].track_off, gp.fields[fi].track_len = off, rows.shape[0]
            prims.append(rows.reshape(-1))
            off += rows.size
        n_floats = int(sum(p.size for p in prims))
        table = np.concatenate(prims).astype(np.float32) if n_floats else np.zeros(4, np.float32)
    gp.table_host = table
    prim_t = torch.from_numpy(table).to(device)
    gp.prims, gp.n_prim_floats = prim_t.data_ptr(), n_floats
    grid_t = None
    if planes:
        grid_t = planes[0] if len(planes) == 1 else torch.cat(planes)   # (a single plane is used in place: no second copy of a 7.8-MB grid)
        gp.grids, gp.n_grid_floats = grid_t.data_ptr(), goff
    gp.grids_tensor = grid_t   # a Python attribute of the ctypes object: the buffer lives as long as the params that point into it
    gp.grid_planes = placed
    gp.chain_tensor = None
    if robot.robot_id == _lib.ROBOT_CHAIN:   # the kinematic table of a planning.RobotChain (layout in include/mpdx.h), kept alive the same way
        if planes:
            raise ValueError("a RobotChain takes primitive, workspace and self fields: no FIELD_GRID field")
        gp.chain_tensor = torch.from_numpy(robot.table()).to(device)
        gp.chain, gp.n_chain_floats = gp.chain_tensor.data_ptr(), gp.chain_tensor.numel()
    return gp, prim_t


def refresh_grid_planes(gp):
    """The planes of a GridSDF were rewritten in place (GridSDF.update_occupancy): copy them again into the grid buffer of `gp` where that buffer is
    a concatenation; nothing to do where the single plane is the buffer."""
    buf = gp.grids_tensor
    if buf is None:
        return
    for off, pl in gp.grid_planes:
        if buf.data_ptr() + 4 * off != pl.data_ptr():
            buf[off: off + pl.numel()].copy_(pl)


def _scene_table(gp, n_scenes, varied, shared):
    """The blocked primitive table of include/mpdx.h: n_scenes blocks of gp.scene_stride floats ([header: n_spheres per field, n_boxes per field,
    int32 | the per-scene tables at fixed offsets, capacity = the largest scene, unused rows zero]) followed by the shared tail (the OBJECTS
    fields that are the same in every scene, stored once).  Sets the fields' offsets / capacities and gp.n_scenes / gp.scene_stride; returns
    (table, floats in it)."""
    off = _lib.SCENE_HEADER_WORDS
    slots = []
    for fi, sets in varied:
        tabs = [o.prim_floats() for o in sets]
        f = gp.fields[fi]
        f.n_spheres, f.n_boxes = max(sp.size // 4 for sp, _ in tabs), max(bx.size // 6 for _, bx in tabs)
        f.sphere_off = off
        f.box_off = off + 4 * f.n_spheres
        off = f.box_off + 6 * f.n_boxes
        slots.append((fi, tabs))
    stride = (off + 3) & ~3
    off = stride
    for fi, sp, bx in shared:     # offsets into the staged image [scene block | shared tail]
        f = gp.fields[fi]
        f.sphere_off, f.n_spheres = off, sp.size // 4
        off += sp.size
        f.box_off, f.n_boxes = off, bx.size // 6
        off += bx.size
    tail = off - stride
    if stride + tail > _lib.SCENE_MAX_STAGED_FLOATS:
        raise ValueError(f"a scene block of {stride} floats + {tail} shared floats exceeds the kernels' table budget of {_lib.SCENE_MAX_STAGED_FLOATS} floats")
    table = np.zeros(n_scenes * stride + tail + 4, np.float32)   # (+4: never an empty allocation; not part of n_prim_floats)
    hdr = table.view(np.int32)
    for s in range(n_scenes):
        b0 = s * stride
        for fi, tabs in slots:
            sp, bx = tabs[s]
            f = gp.fields[fi]
            hdr[b0 + fi], hdr[b0 + _lib.MAX_FIELDS + fi] = sp.size // 4, bx.size // 6
            table[b0 + f.sphere_off: b0 + f.sphere_off + sp.size] = sp
            table[b0 + f.box_off: b0 + f.box_off + bx.size] = bx
        for fi, sp, bx in shared:   # a shared field has its capacity in every scene
            hdr[b0 + fi], hdr[b0 + _lib.MAX_FIELDS + fi] = sp.size // 4, bx.size // 6
    for fi, sp, bx in shared:
        f = gp.fields[fi]
        g0 = n_scenes * stride - stride   # image offset -> table offset of the tail
        table[g0 + f.sphere_off: g0 + f.sphere_off + sp.size] = sp
        table[g0 + f.box_off: g0 + f.box_off + bx.size] = bx
    gp.n_scenes, gp.scene_stride = n_scenes, stride
    return table, n_scenes * stride + tail


class GuideManagerTrajectoriesWithVelocity(nn.Module):
    def __init__(self, dataset, cost, clip_grad=False, clip_grad_rule="norm", max_grad_norm=1.0, max_grad_value=0.1,
                 interpolate_trajectories_for_collision=False, num_interpolated_points_for_collision=128,
                 start_state_pos=None, goal_state_pos=None, num_steps=100, robot=None, n_samples=1, tensor_args=None, **kwargs):
        super().__init__()
        # A CostComposite of the reference's cost terms is compiled into the HIP guide kernel (hand-derived gradients).
        # Any other callable with the call-site contract of guides.py:190,
        #     cost(x, x_interpolated=..., return_invidual_costs_and_weights=True) -> ([B] tensors, [weights]),
        # is differentiated with torch autograd ON THE GPU exactly as the reference's manager does (guides.py:173-211);
        # such a guide runs on the step-by-step protocol loop, not inside mpdx_plan.
        self.is_native = isinstance(cost, CostComposite)
        if not self.is_native and not callable(cost):
            raise TypeError("cost must be a CostComposite or a callable with the contract of guides.py:190")
        if clip_grad_rule not in ("norm", "value"):
            raise NotImplementedError(f"clip_grad_rule={clip_grad_rule!r}")   # as guides.py:219-220
        self.cost, self.dataset = cost, dataset
        self.interpolate_trajectories_for_collision = interpolate_trajectories_for_collision
        self.num_interpolated_points_for_collision = num_interpolated_points_for_collision
        self.clip_grad, self.clip_grad_rule = clip_grad, clip_grad_rule
        self.max_grad_norm, self.max_grad_value = max_grad_norm, max_grad_value
        self._params = None
        self._prims = None
        self._grids = None
        self._flag = None
        # a guide bound to obstacle scenes (with_scenes): the scenes, the host assignment, trajectories per context, the device index table
        self._scenes = None
        self._scene_of_context = None
        self._n_per_context = None
        self._scene_table = None

    def with_scenes(self, scenes, scene_of_context, n_per_context):
        """A guide with the same cost terms and options whose trajectories see different obstacle scenes (an extension, planning.PlanningScenes):
        the c-th group of `n_per_context` consecutive trajectories uses scene `scene_of_context[c]`.  The returned guide owns the device index
        table; it is what `guide=` of GaussianDiffusionModel.plan / the step-by-step loop takes, for batches of len(scene_of_context) *
        n_per_context trajectories.  Its whole-tensor range test (LimitsNormalizer.unnormalize) is evaluated per context, as one call per context
        would.  The reference's constructor signature is untouched: the binding is this method."""
        if not self.is_native:
            raise NotImplementedError("scenes need the HIP guide (a CostComposite of the reference's cost terms); a guide that differentiates a Python cost "
                                      "with autograd has one set of obstacles, inside that cost")
        if scenes.task is not self.dataset.task:
            raise ValueError("the scenes were built for another task than this guide's dataset.task")
        soc = scenes.check_assignment(scene_of_context, None, n_per_context)
        g = GuideManagerTrajectoriesWithVelocity(self.dataset, self.cost, clip_grad=self.clip_grad, clip_grad_rule=self.clip_grad_rule,
                                                 max_grad_norm=self.max_grad_norm, max_grad_value=self.max_grad_value,
                                                 interpolate_trajectories_for_collision=self.interpolate_trajectories_for_collision,
                                                 num_interpolated_points_for_collision=self.num_interpolated_points_for_collision)
        g._scenes, g._scene_of_context, g._n_per_context = scenes, soc, int(n_per_context)
        return g

    def check_batch(self, B, n_per_context=None):
        """A scene-bound guide serves batches of exactly the shape it was bound to."""
        if self._scenes is None:
            return
        if B != len(self._scene_of_context) * self._n_per_context:
            raise ValueError(f"this guide is bound to {len(self._scene_of_context)} contexts of {self._n_per_context} trajectories, not to a batch of {B}")
        if n_per_context is not None and int(n_per_context) != self._n_per_context:
            raise ValueError(f"n_per_context={n_per_context} differs from the {self._n_per_context} the guide's scenes were bound with")

    # ------------------------------------------------------------------------------------------- compile to device params
    def device_params(self, device) -> "_lib.GuideParams":
        if self._params is not None and self._prims.device == torch.device(device):
            return self._params
        ds = self.dataset
        if ds.state_dim != 2 * ds.robot.q_dim:
            raise NotImplementedError("the velocity guide needs include_velocity=True (state = pos + vel)")
        kind = getattr(ds.normalizer, "kind", "limits")
        if kind not in ("limits", "identity", "gaussian"):
            raise NotImplementedError(f"the HIP guide un-normalises with limits (LimitsNormalizer and its subclasses), mean / std (GaussianNormalizer) or not at "
                                      f"all (Identity); {type(ds.normalizer).__name__} is not supported under a guide")
        # the kernel's un-normalisation: 0 = limits with the whole-tensor range test (normalization.py:156-167), 1 = none (:111-116),
        # 2 = x * stds + means (:140-141; the two vectors travel in the `mins` / `maxs` slots, no range test)
        mode = {"limits": 0, "identity": 1, "gaussian": 2}[kind]
        lo = None if mode == 1 else ds.normalizer.means if mode == 2 else ds.normalizer.mins
        hi = None if mode == 1 else ds.normalizer.stds if mode == 2 else ds.normalizer.maxs
        self._params, self._prims = build_device_params(
            ds.robot, ds.env.dim, ds.task.obstacle_cutoff_margin, lo, hi,
            self.cost.cost_l, self.cost.weight_cost_l, self.interpolate_trajectories_for_collision, self.num_interpolated_points_for_collision,
            self.clip_grad, self.max_grad_norm, device, clip_grad_rule=self.clip_grad_rule, max_grad_value=self.max_grad_value,
            identity_normalizer=mode, scenes=self._scenes)
        self._grids = self._params.grids_tensor
        if self._scenes is not None:
            self._scene_table = torch.tensor(self._scene_of_context, dtype=torch.int32, device=device)
            self._params.scene_of_ctx, self._params.scene_n_per_ctx = self._scene_table.data_ptr(), self._n_per_context
        return self._params

    def refresh_grids(self):
        """After GridSDF.update_occupancy on a grid of this guide's fields: copy the planes again where the guide's grid buffer is a concatenation
        (several planes: nearest mode, or more than one grid); a no-op where the single plane is used in place."""
        if self._params is not None:
            refresh_grid_planes(self._params)

    # ------------------------------------------------------------------------------------------- the values of what the guide differentiates
    @torch.no_grad()
    def costs(self, x_normalized, return_clearance=False, return_point_costs=False):
        """The VALUES of this guide's cost terms on normalised trajectories [B,H,D] (GPU): a planning.TrajectoryCosts - the unweighted terms in the
        order of cost.cost_l, the composite's weights, their total and, on request, the clearance per collision field and the factor sums per point.
        Un-normalises with dataset.unnormalize_trajectories and evaluates the guide's own parameter block (mpdx_traj_costs): its interpolate /
        num_interpolated_points_for_collision, its scene binding, its grids (refresh_grids reaches the block as it does for forward) - the cost the
        guide differentiates, on the points where it differentiates it.  The reference's contract cost(x, x_interpolated=...,
        return_invidual_costs_and_weights=True) -> (terms, weights) is (list(c.terms.T), list(c.weights))."""
        if not self.is_native:
            raise NotImplementedError("costs() evaluates a CostComposite of the reference's terms on the HIP kernel; this guide differentiates a Python cost "
                                      "callable - call it directly, cost(x, x_interpolated=..., return_invidual_costs_and_weights=True), as the reference does")
        if not x_normalized.is_cuda:
            raise RuntimeError("the guide's costs run on the GPU (libmpdx); there is no CPU fallback")
        from .planning import TrajectoryCosts, launch_traj_costs
        x = x_normalized.to(torch.float32)
        self.check_batch(x.shape[0])
        xu = self.dataset.unnormalize_trajectories(x).to(torch.float32).contiguous()
        gp = self.device_params(x.device)
        return TrajectoryCosts.from_slots(self.cost, *launch_traj_costs(gp, xu, 0, return_clearance, return_point_costs))

    # ------------------------------------------------------------------------------------------- guide protocol
    def _forward_autograd(self, x_normalized):
        """guides.py:173-211 verbatim in behaviour, for a Python cost callable: torch autograd on the device."""
        if not x_normalized.is_cuda:
            raise RuntimeError("the guide runs on the GPU; there is no CPU fallback")
        x = x_normalized.detach().clone()
        with torch.enable_grad():
            x.requires_grad_(True)
            x = self.dataset.unnormalize_trajectories(x)
            if self.interpolate_trajectories_for_collision:
                xi = torch.nn.functional.interpolate(x.transpose(-2, -1), self.num_interpolated_points_for_collision, mode="linear",
                                                     align_corners=True).transpose(-2, -1)
            else:
                xi = x
            cost_l, w_l = self.cost(x, x_interpolated=xi, return_invidual_costs_and_weights=True)
            grad = 0
            for c, w in zip(cost_l, w_l):
                if torch.is_tensor(c):
                    g = torch.autograd.grad([c.sum()], [x], retain_graph=True)[0]
                    if self.clip_grad:
                        if self.clip_grad_rule == "norm":
                            n = torch.linalg.norm(g + 1e-6, dim=-1, keepdims=True)
                            g = torch.clip(n, 0.0, self.max_grad_norm) / n * g
                        else:
                            g = torch.clip(g, -self.max_grad_value, self.max_grad_value)
                    g[..., 0, :] = 0.0
                    g[..., -1, :] = 0.0
                    grad = grad + w * g
        return (-1.0 * grad).detach()

    @torch.no_grad()
    def forward(self, x_normalized):
        if not self.is_native:
            return self._forward_autograd(x_normalized)
        x = x_normalized.to(torch.float32).contiguous()
        B, H, D = x.shape
        self.check_batch(B)
        gp = self.device_params(x.device)
        lib, st = _lib.load(), _lib.current_stream()
        npc = self._n_per_context if self._scenes is not None else B   # scenes: the range test per context, as one call per context would
        flag = torch.zeros(B // npc, dtype=torch.int32, device=x.device)
        _lib.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), npc, B, H, D, st), "mpdx_absmax")
        out = torch.empty_like(x)
        _lib.check(lib.mpdx_guide_step(C.byref(gp), x.data_ptr(), out.data_ptr(), None, None, flag.data_ptr(), None, npc, B, H, D, st),
                   "mpdx_guide_step")
        return out
