"""The grid-box edge cases of tests/test_gpu_grid_edges.py and tests/test_grid_edges_cpu.py - test infrastructure, nothing here touches the GPU.

Every grid is an occupancy grid of the FIXED objects (occupied = the primitive sdf at the node <= 0), transformed with inflate 0.003
(tests/test_gpu_occupancy.py::FIELD_INFLATE: off the lattice of the hinge margins), on a box of its own that cuts through obstacles, with a different
node count along every used axis (a lookup that took a row or plane stride from the wrong count would read other nodes).  The reference planes
come from tests/edt_ref.py (brute force, the arithmetic the device is held to bit for bit); the GPU test downloads the device's planes, asserts
that they equal these, and builds its reference from them.

A case's link points leave its box below and above on some axis: there the lookup clamps the cell coordinate (include/mpdx.h, mpdx_field), a clamped
axis has zero gradient in linear mode, and nearest mode returns the edge node's stored gradient.

The altered references (`mutant`): each stands for a plausible bug of csrc/grid_field.hpp, and tests/test_grid_edges_cpu.py asserts that the GPU
test's yardstick would reject it on the case's own inputs:
  'row'      the row stride taken from n[1] instead of n[0]
  'plane'    the plane stride taken from n[1] * n[2] instead of n[0] * n[1] (3-D)
  'clamped'  a clamped axis keeps its gradient (linear)
  'offset0'  the second grid field of the two-grid block read at offset 0 of the grid buffer (the first field's planes)
"""
import copy
import functools

import numpy as np
import torch

import edt_ref
from grid_ref import GridField
from helpers import obstacle_hugging_trajs, oracle_guide
from test_gpu_grid_sdf import CAP, _classify, _to_supports

INFLATE = 0.003
WEIGHTS = (1e-2, 1e-7)
B = 7

# name -> env, robot, horizon, trajectories, grid box (nx, ny[, nz]), origin, cell
CASES = {
    "pm2-H64": dict(env_id="EnvSimple2D", robot_id="RobotPointMass", H=64, seed="edge/pm2", shape=(118, 131), origin=(-0.553, -0.947), cell=0.01),
    "pm2-H96": dict(env_id="EnvSimple2D", robot_id="RobotPointMass", H=96, seed="edge/pm2-96", shape=(118, 131), origin=(-0.553, -0.947), cell=0.01),
    "pm2-ny2": dict(env_id="EnvSimple2D", robot_id="RobotPointMass", H=64, seed="edge/pm2-ny2", shape=(163, 2), origin=(-0.817, 0.5013), cell=0.0093),
    "pm3": dict(env_id="EnvSpheres3D", robot_id="RobotPointMass3D", H=64, seed="edge/pm3", shape=(37, 29, 23), origin=(-0.6137, -0.4411, 0.2219),
                cell=0.0331, aim=(1, 3, 4, 11, 14, 0, 6)),
    "panda": dict(env_id="EnvSpheres3D", robot_id="RobotPanda", H=64, seed="edge/panda", shape=(31, 27, 23), origin=(-0.5311, -0.4877, 0.1539),
                  cell=0.0397),
}
# one block with two grid fields: a nearest grid whose node count (59 x 43 = 2537) is no multiple of 4 in the objects slot, the workspace field,
# a linear grid over another box in the extra-objects slot (its planes follow the first grid's in the grid buffer), and the GP prior
TWO = dict(env_id="EnvSimple2D", robot_id="RobotPointMass", H=64, seed="edge/two",
           grids=(dict(shape=(59, 43), origin=(-1.0317, -0.2191), cell=0.0213, mode="nearest"),
                  dict(shape=(97, 71), origin=(-0.4123, -0.8867), cell=0.0109, mode="linear")))


def robot_of(robot_id):
    return "RobotPanda" if robot_id == "RobotPanda" else "RobotPointMass"


# ------------------------------------------------------------------------------------------------------------ planes
def occupancy(env_id, shape, origin, cell):
    """[nz, ny, nx] bool (nz = 1 in 2-D): the primitive sdf of the fixed objects at the node <= 0, in float64 from the environment's tables"""
    import mpd_public_amd as m
    env = m.TrajectoryDataset(env_id, "RobotPanda" if env_id == "EnvSpheres3D" else "RobotPointMass").env
    dim = len(shape)
    ax = [np.float64(np.float32(origin[j])) + np.arange(shape[j]) * cell for j in range(dim)]
    pos = np.stack(np.meshgrid(*reversed(ax), indexing="ij")[::-1], -1)
    o = env.obj_fixed
    sd = np.full(pos.shape[:-1], np.inf)
    for c, r in zip(o.sphere_centers, o.sphere_radii):
        sd = np.minimum(sd, np.linalg.norm(pos - c[:dim], axis=-1) - r)
    for c, h in zip(o.box_centers, o.box_half):
        d = np.abs(pos - c[:dim]) - h[:dim]
        sd = np.minimum(sd, np.minimum(d.max(-1), 0.0) + np.linalg.norm(np.maximum(d, 0.0), axis=-1))
    occ = sd <= 0
    return occ.reshape((1,) + occ.shape) if dim == 2 else occ


@functools.lru_cache(maxsize=None)
def planes(env_id, shape, origin, cell):
    """(occ, sdf, grad) of a grid box, numpy, in the grid's own layout ([ny, nx] / [nz, ny, nx]; grad [..., 4]); computed once, read-only"""
    occ3 = occupancy(env_id, shape, origin, cell)
    sdf3 = edt_ref.sdf_ref(edt_ref.d2_ref(occ3), occ3, cell, INFLATE)
    grad3 = edt_ref.grad_ref(sdf3, cell)
    lead = tuple(reversed(shape))
    out = (occ3.reshape(lead), sdf3.reshape(lead), grad3.reshape(lead + (4,)))
    for a in out:
        a.setflags(write=False)
    return out


def spec_planes(spec, env_id):
    return planes(env_id, tuple(spec["shape"]), tuple(spec["origin"]), spec["cell"])


def field_of(spec, mode, sdf, grad):
    return GridField(torch.from_numpy(np.array(sdf)), spec["origin"], spec["cell"], mode, torch.from_numpy(np.array(grad)) if mode == "nearest" else None)


# ------------------------------------------------------------------------------------------------------------ datasets and inputs
def base_dataset(case, device="cpu"):
    import mpd_public_amd as m
    c = CASES[case] if isinstance(case, str) else case
    return m.TrajectoryDataset(c["env_id"], c["robot_id"], n_support_points=c["H"], tensor_args={"device": device, "dtype": torch.float32})


def with_grids(ds, grids):
    """ds with its task's fixed objects replaced by grids[0] (a grid_sdf.GridSDF) and - two grids - its extra objects by grids[1]"""
    from mpd_public_amd import _lib
    from mpd_public_amd.planning import CollisionField, PlanningTask
    d = copy.copy(ds)
    d.task = PlanningTask(ds.env, ds.robot, obstacle_cutoff_margin=ds.task.obstacle_cutoff_margin, tensor_args=ds.tensor_args, sdf_grid=grids[0])
    if len(grids) > 1:
        d.task.df_collision_extra_objects = CollisionField(_lib.FIELD_GRID, grid=grids[1], name="extra_objects")
    return d


def aimed_trajs(ds, seed, aim, centres=None):
    """normalised fp32 [len(aim), 64, D]: straight lines through the centres of the listed fixed spheres (or through `centres` [n, >= q_dim]) at
    mid-time, on to the mirror image of their start (clamped to +-0.95), plus a little noise; velocities inside +-0.9 (the normaliser's range test
    does not fire)"""
    from helpers import t
    from oracle.normalizer import LimitsNormalizer
    qd = ds.robot.q_dim
    nrm = LimitsNormalizer(ds.normalizer.mins.cpu(), ds.normalizer.maxs.cpu())
    src = ds.env.obj_fixed.sphere_centers[list(aim)] if centres is None else np.asarray(centres)
    ctr = torch.tensor(src[:, :qd], dtype=torch.float32)
    n = ctr.shape[0]
    b = nrm.normalize(torch.cat([ctr, ctr], -1))[:, :qd].unsqueeze(1)
    a = t(f"{seed}/a", (n, 1, qd), "uniform", 0.9)
    s = torch.linspace(0, 1, 64).reshape(1, 64, 1)
    pos = (a + 2 * (b - a) * s).clamp(-0.95, 0.95) + 0.01 * t(f"{seed}/n", (n, 64, qd))
    return torch.cat([pos, (0.3 * t(f"{seed}/v", (n, 64, qd))).clamp(-0.9, 0.9)], -1).contiguous()


@functools.lru_cache(maxsize=None)
def trajs(case):
    """normalised fp32 [B, H, D] (read-only)"""
    c = CASES[case] if case in CASES else TWO
    ds = base_dataset(c)
    if "aim" in c:
        x = aimed_trajs(ds, c["seed"], c["aim"])
    else:
        x = obstacle_hugging_trajs(ds, B, seed=c["seed"], scale=0.9)
    if c["H"] != 64:
        x = torch.nn.functional.interpolate(x.transpose(1, 2), c["H"], mode="linear", align_corners=True).transpose(1, 2).contiguous()
    x.requires_grad_(False)
    return x


# ------------------------------------------------------------------------------------------------------------ the reference
def grid_terms(comp):
    return [k for k, term in enumerate(comp.cost_l) if isinstance(getattr(term, "field", None), GridField)]


def oracle(ds_prim, fields, two=False):
    """(og, comp, [grid term indices]) of the unchanged fp64 oracle with the fixed objects' field - and, two grids, the extra objects' - replaced by
    `fields` (GridField)"""
    og, comp = oracle_guide(ds_prim, *WEIGHTS, dtype=torch.float64)
    names = [f.name for f in ds_prim.task.get_collision_fields()]
    ks = [names.index("objects")] + ([names.index("extra_objects")] if two else [])
    for k, gf in zip(ks, fields):
        comp.cost_l[k].field = gf
    return og, comp, ks


def classify(comp, xi, cutoff):
    """[B, N] bool: tests/test_gpu_grid_sdf.py::_classify over every grid term"""
    cut = {i: cutoff for i in range(len(comp.cost_l))}
    amb = None
    for k in grid_terms(comp):
        a = _classify(comp, comp.cost_l[k].field, xi, cut)
        amb = a if amb is None else amb | a
    return amb


def hits(comp, xi):
    """[B, N] bool: the metrics flags in fp64 (margin = link radius, no cutoff)"""
    from oracle import costs as oc
    hit = torch.zeros(xi.shape[:2], dtype=torch.bool)
    for term in comp.cost_l:
        if isinstance(term, oc.CostCollision):
            keep, term.cutoff = term.cutoff, 0.0
            hit |= (term.factors(xi) > 0).any(-1)
            term.cutoff = keep
    return hit


def clamped_points(gf, pts):
    """[..., K, dim] bool: the link point lies outside the grid box along that axis (its coordinate is clamped)"""
    u = (pts - gf.origin.to(pts.dtype)) * gf.inv
    hi = torch.tensor([v - 1 for v in gf.n], dtype=pts.dtype)
    return (u < 0) | (u > hi)


def n_check_of(H):
    return 4 * H


def reference(case, fields):
    """everything the fp64 reference says about a case ('two': the two-grid block) with its grid terms over `fields` (GridField): og, comp, grid term
    indices, x, xi (guide), amb [B, H] (support waypoints), ref (increment), xm (the checked points of the metrics), hit, amb_m [B, n_check]"""
    from oracle.guide import interpolate_points_v1
    two = case == "two"
    c = TWO if two else CASES[case]
    ds = base_dataset(c)
    og, comp, ks = oracle(ds, fields, two)
    x = trajs(case)
    xu = og.normalizer.unnormalize(x.double())
    xi = interpolate_points_v1(xu, 128)
    amb = _to_supports(classify(comp, xi, ds.task.obstacle_cutoff_margin), c["H"]).numpy()
    ref = og(x.double()).numpy()
    xm = interpolate_points_v1(xu.float().double(), n_check_of(c["H"]))
    return dict(ds=ds, og=og, comp=comp, ks=ks, x=x, xi=xi, amb=amb, ref=ref, xm=xm, hit=hits(comp, xm).numpy(), amb_m=classify(comp, xm, 0.0).numpy())


@functools.lru_cache(maxsize=None)
def cpu_reference(case, mode):
    """reference() over the edt_ref planes; case 'two' is the two-grid block (mode ignored)"""
    if case == "two":
        fields = [field_of(g, g["mode"], *spec_planes(g, TWO["env_id"])[1:]) for g in TWO["grids"]]
        return reference(case, fields)
    c = CASES[case]
    _, sdf, grad = spec_planes(c, c["env_id"])
    return reference(case, [field_of(c, mode, sdf, grad)])


# ------------------------------------------------------------------------------------------------------------ the yardstick and the altered copies
def atol_of(w_coll=WEIGHTS[0]):
    return 2e-6 * max(w_coll, 1e-2) / 1e-2         # tests/test_gpu_grid_sdf.py: the rtol=1e-3 / atol line


def outside(got, ref, factor=1.0):
    """[B, H] bool: a waypoint with an element farther than factor x (atol + 1e-3 |ref|) from the reference"""
    return (np.abs(got - ref) > factor * (atol_of() + 1e-3 * np.abs(ref))).any(-1)


class _Mutant(GridField):
    """a GridField whose lookups form the flat index with other strides (the node arrays padded so that every index stays inside), or whose clamped
    axes keep their gradient"""

    def __init__(self, gf, strides=None, keep_clamped_grad=False):
        self.__dict__.update(gf.__dict__)
        if strides is not None:
            self.strides = list(strides)
            reach = sum((v - 1) * s for v, s in zip(self.n, self.strides)) + sum(self.strides) + 1
            extra = max(0, reach - self.sdf_flat.numel())
            self.sdf_flat = torch.cat([self.sdf_flat, torch.zeros(extra)])
            if self.grad_flat is not None:
                self.grad_flat = torch.cat([self.grad_flat, torch.zeros(extra, self.grad_flat.shape[1])])
        self.keep_clamped_grad = keep_clamped_grad

    def coords(self, p):
        c = GridField.coords(self, p)
        if not self.keep_clamped_grad:
            return c
        u = (p - self.origin.to(p.dtype)) * self.inv
        return u + (c - u).detach()                  # the clamped value, the unclamped derivative


def mutant(gf, kind, first=None):
    n = gf.n
    if kind == "row":
        return _Mutant(gf, [1, n[1], n[0] * n[1]][:gf.dim])
    if kind == "plane":
        return _Mutant(gf, [1, n[0], n[1] * n[2]])
    if kind == "clamped":
        return _Mutant(gf, keep_clamped_grad=True)
    if kind == "offset0":   # the grid buffer of guides.build_device_params: [first sdf | pad to 4 | first grad (nearest)] then this field's plane
        buf = [first.sdf_flat]
        if first.sdf_flat.numel() % 4:
            buf.append(torch.zeros(4 - first.sdf_flat.numel() % 4))
        if first.mode == "nearest":
            g4 = torch.zeros(first.grad_flat.shape[0], 4)
            g4[:, :first.dim] = first.grad_flat
            buf.append(g4.reshape(-1))
        buf.append(gf.sdf_flat)
        m = _Mutant(gf)
        m.sdf_flat = torch.cat(buf)[: gf.sdf_flat.numel()].clone()
        return m
    raise ValueError(kind)


def mutant_increment(case, mode, kind):
    """the increment of the oracle with the case's (last) grid field replaced by its altered copy"""
    r = cpu_reference(case, mode)
    comp = r["comp"]
    k = r["ks"][-1]
    keep = comp.cost_l[k].field
    comp.cost_l[k].field = mutant(keep, kind, first=comp.cost_l[r["ks"][0]].field if kind == "offset0" else None)
    try:
        return r["og"](r["x"].double()).numpy()
    finally:
        comp.cost_l[k].field = keep
