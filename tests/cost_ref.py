"""Reference side of the cost-value tests (tests/test_cost_cpu.py, tests/test_gpu_costs.py; mpdx_traj_costs, csrc/costs.hpp) - test infrastructure,
nothing here touches the GPU.

The per-term costs are those of the existing oracle composites (guide_ref.oracle_of / helpers.oracle_guide, chain_ref.oracle_guide_chain,
grid_ref.GridField, moving_ref.oracle, tool_ref.ToolAxisRef, scene_ref.scene_dataset), called as the reference's guide calls its cost,
    comp(xu, x_interpolated=xi, return_invidual_costs_and_weights=True),  xi = interpolate_points_v1(xu, n_points).
The clearance per field is restated in the manner of helpers.oracle_config_slack (which gives -(clearance) over all fields); the factor sums per
point come from CostCollision.factors(...).sum(-1).

The yardstick (the allowance a kernel value gets) is computed from two evaluations of the SAME composite on the SAME float32 inputs, one in float64
and one in torch float32 on the CPU - never from the kernel's output:
    allowance = 8 x |fp32 oracle - fp64 oracle| (the largest over the batch, per term) + n_factors_active x 2^-22 x max(1, largest |coordinate|)
(the kernel sums in another order and has its own sin / cos and square roots); a clearance has n_factors_active = 1.
"""
import torch

FACTOR = 8.0
ULP_FLOOR = 2.0 ** -22


def is_collision(term):
    from oracle import costs as oc
    return isinstance(term, oc.CostCollision)


def is_tool(term):
    return hasattr(term, "cos_min") and hasattr(term, "d")      # tool_ref.ToolAxisRef


def term_slack(term, xi):
    """[B, N, n_factors]: radius-margin minus distance of every factor of a collision term (no cutoff margin, no relu) - per link sphere (objects,
    grid and moving fields: anything with .sdf), per sphere and face (workspace), per pair (self).  helpers.oracle_config_slack, one term at a time."""
    rob, f = term.robot, term.field
    dtype = xi.dtype
    pts = rob.link_points(xi[..., : rob.q_dim])
    radii = rob.radii.to(dtype)
    if f.kind == "objects":
        return radii - f.sdf(pts)
    if f.kind == "workspace":
        m = radii.unsqueeze(-1)
        return torch.cat([m - (pts - f.ws_min.to(dtype)), m - (f.ws_max.to(dtype) - pts)], dim=-1).flatten(-2)
    if f.kind == "self":
        a, b = pts[..., f.pairs[:, 0], :], pts[..., f.pairs[:, 1], :]
        return radii[f.pairs[:, 0]] + radii[f.pairs[:, 1]] - torch.linalg.norm(a - b, dim=-1)
    raise NotImplementedError(f.kind)


def clearance(comp, xi):
    """[B, n_collision_terms]: per collision term of the composite, the minimum over points and factors of (distance - radius margin)"""
    return torch.stack([-term_slack(t, xi).amax((-1, -2)) for t in comp.cost_l if is_collision(t)], -1)


def point_costs(comp, xi):
    """[B, N, n_collision_terms (+ 1 with a tool term)]: the unweighted factor sum of every collision term at every point, then the tool hinge"""
    cols = [t.factors(xi).sum(-1) for t in comp.cost_l if is_collision(t)]
    cols += [torch.relu(t.cos_min.to(xi.dtype) - t.d(xi)) for t in comp.cost_l if is_tool(t)]
    return torch.stack(cols, -1)


def active_factors(comp, xi):
    """([B, n_terms], [B, N, n point columns]) numbers of factors with a non-zero value: per term and trajectory (the GP prior: its H - 1 segments
    are not counted here - 0), and per point column"""
    per_term, per_point = [], []
    for t in comp.cost_l:
        if is_collision(t):
            a = (t.factors(xi) > 0).sum(-1)
            per_term.append(a.sum(-1))
            per_point.append(a)
        elif is_tool(t):
            a = (t.cos_min.to(xi.dtype) - t.d(xi) > 0).long()
            per_term.append(a.sum(-1))
        else:
            per_term.append(torch.zeros(xi.shape[0], dtype=torch.long))
    per_point += [(t.cos_min.to(xi.dtype) - t.d(xi) > 0).long() for t in comp.cost_l if is_tool(t)]
    return torch.stack(per_term, -1), torch.stack(per_point, -1) if per_point else None


def largest_coordinate(comp, xu, xi):
    """max(1, largest |coordinate|) over the state and the link points of every collision term"""
    big = float(xu.abs().max())
    for t in comp.cost_l:
        if is_collision(t):
            big = max(big, float(t.robot.link_points(xi[..., : t.robot.q_dim]).abs().max()))
    return max(1.0, big)


def evaluate(comp, xu, n_points, dtype=torch.float64):
    """The reference's values of a composite on UNNORMALISED trajectories xu [B, H, D] (any dtype; evaluated in `dtype`; comp must have been built in
    `dtype`): dict(terms [B, n_terms] unweighted, in the order of comp.cost_l; weights; total; clearance; point_costs; xi)."""
    from oracle.guide import interpolate_points_v1
    xu = xu.to(dtype)
    xi = interpolate_points_v1(xu, n_points)
    with torch.no_grad():
        cost_l, w_l = comp(xu, x_interpolated=xi, return_invidual_costs_and_weights=True)
        terms = torch.stack([c.to(dtype) for c in cost_l], -1)
        w = torch.tensor([float(v) for v in w_l], dtype=dtype)
        has_coll = any(is_collision(t) for t in comp.cost_l)
        out = dict(terms=terms, weights=w, total=terms @ w, xi=xi, xu=xu,
                   clearance=clearance(comp, xi) if has_coll else torch.zeros((xu.shape[0], 0), dtype=dtype),
                   point_costs=point_costs(comp, xi) if has_coll or any(is_tool(t) for t in comp.cost_l) else None)
    return out


def yardstick(comp64, comp32, xu32, n_points):
    """(ref: evaluate() in fp64, allow: dict of absolute allowances with the shapes terms [B, n_terms] (total [B], clearance [B, n_coll], point_costs
    [B, N, cols]) - from the fp64 and the torch-fp32 oracle alone, err32: the fp32 oracle's largest error per term [n_terms])."""
    assert xu32.dtype == torch.float32
    r64 = evaluate(comp64, xu32, n_points, torch.float64)
    r32 = evaluate(comp32, xu32, n_points, torch.float32)
    n_term, n_point = active_factors(comp64, r64["xi"])
    big = largest_coordinate(comp64, r64["xu"], r64["xi"])
    H = xu32.shape[1]
    gp_cols = torch.tensor([0 if (is_collision(t) or is_tool(t)) else H - 1 for t in comp64.cost_l])
    err_terms = (r32["terms"].double() - r64["terms"]).abs().amax(0)                                    # [n_terms]
    allow_terms = FACTOR * err_terms + (n_term + gp_cols).double() * ULP_FLOOR * big                    # [B, n_terms]
    w = r64["weights"].abs()
    allow = dict(terms=allow_terms, total=allow_terms @ w)
    err_clr = (r32["clearance"].double() - r64["clearance"]).abs().amax(0) if r64["clearance"].shape[-1] else torch.zeros(0, dtype=torch.float64)
    allow["clearance"] = (FACTOR * err_clr + ULP_FLOOR * big).expand_as(r64["clearance"])
    if r64["point_costs"] is not None:
        err_pt = (r32["point_costs"].double() - r64["point_costs"]).abs().amax((0, 1))
        allow["point_costs"] = FACTOR * err_pt + n_point.double() * ULP_FLOOR * big
    return r64, allow, err_terms


def compare(got, ref, allow, what, names=None):
    """got: a planning.TrajectoryCosts (or a dict with its members) on the device or the host.  Prints the largest error beside the allowance for every
    member and term, then asserts |got - ref| <= allowance everywhere (NaN fails).  Returns the figures [(member, term, max err, allowance there)]."""
    figs, bad = [], []
    for key in ("terms", "total", "clearance", "point_costs"):
        g = got[key] if isinstance(got, dict) else getattr(got, key)
        if g is None:
            continue
        g = torch.as_tensor(g).detach().cpu().double()
        r, a = ref[key].double(), allow[key].double()
        assert g.shape == r.shape, (what, key, tuple(g.shape), tuple(r.shape))
        err = (g - r).abs()
        cols = range(g.shape[-1]) if g.dim() > 1 else [None]
        for k in cols:
            e, al, rr = (err, a, r) if k is None else (err[..., k], a[..., k], r[..., k])
            i = int(torch.nan_to_num(e, nan=float("inf")).argmax())
            name = "" if k is None else (names[k] if names and key == "terms" and k < len(names) else str(k))
            figs.append((key, name, float(e.reshape(-1)[i]), float(al.reshape(-1)[i])))
            print(f"{what}: {key} {name}: max err {float(e.reshape(-1)[i]):.3e} (allowance there {float(al.reshape(-1)[i]):.3e}, smallest allowance "
                  f"{float(al.min()):.3e}; |ref| up to {float(rr.abs().max()):.4g})")
            if not bool((e <= al).all()):
                bad.append((key, name, int((~(e <= al)).sum())))
    assert not bad, f"{what}: outside the allowance: {bad}"
    return figs


def unnormalised32(og, x):
    """the float32 un-normalised trajectories a kernel is given: the oracle normaliser's float64 result, rounded once"""
    return og.normalizer.unnormalize(x.double()).float().contiguous()


# ------------------------------------------------------------------------------------------------------------ the cases of the tests
# (robot, H, n_points) of the term comparisons: the coverage cases of guide_ref at their own interpolation, the Panda again with two waves of
# supports and a point count that is no multiple of 64 (257 = four strides + 1), and at H = 8 with 70 points (one stride + 6) - and each of the
# H = 64 cases once more at n_points == H (the supports themselves) inside the test
TERM_CASES = [("RobotPointMass", 64, 128), ("RobotPointMass3D", 24, 128), ("RobotPanda", 64, 128), ("chain:R1", 64, 128), ("chain:R3", 64, 128),
              ("chain:R8", 64, 128), ("chain:Panda", 64, 128), ("RobotPanda", 128, 257), ("RobotPanda", 8, 70)]
TERM_IDS = [f"{r.replace('chain:', '')}-H{h}-N{n}" for r, h, n in TERM_CASES]
# the cases whose every slot must be non-zero on some trajectory (tests/test_cost_cpu.py), but for guide_ref.ZERO_RUNS
SLOT_CASES = [("RobotPointMass", 64), ("RobotPointMass3D", 24), ("RobotPanda", 64), ("chain:R3", 64), ("chain:R8", 64), ("chain:R1", 64)]
WEIGHTS = (1e-2, 1e-7)


def oracle_pair(ds, n_interp=128, **kw):
    """(og, comp64, comp32): the oracle composite of a coverage dataset in float64 and in float32 (the yardstick's two evaluations)"""
    import guide_ref as gr
    og, c64 = gr.oracle_of(ds, *WEIGHTS, dtype=torch.float64, n_interp=n_interp, **kw)
    _, c32 = gr.oracle_of(ds, *WEIGHTS, dtype=torch.float32, n_interp=n_interp, **kw)
    return og, c64, c32


def product_composite(ds, weights=WEIGHTS, half_factor=False, sigma_gp=1.0, shuffle=None):
    """The product's CostComposite of a dataset as inference.py builds it (the collision fields, then the GP prior); shuffle: a permutation of the terms"""
    import mpd_public_amd as m
    H = ds.n_support_points
    costs = [m.CostCollision(ds.robot, H, field=f, sigma_coll=1.0) for f in ds.task.get_collision_fields()]
    w = [weights[0]] * len(costs)
    costs.append(m.CostGPTrajectory(ds.robot, H, 5.0 / H, sigma_gp=sigma_gp, half_factor=half_factor))
    w.append(weights[1])
    if shuffle is not None:
        costs, w = [costs[i] for i in shuffle], [w[i] for i in shuffle]
    return m.CostComposite(ds.robot, H, costs, weights_cost_l=w)


def term_case(robot_id, H):
    """(case of guide_ref, og, comp64, comp32, xu32) of a coverage case"""
    import guide_ref as gr
    c = gr.case(robot_id, H)
    og, c64, c32 = oracle_pair(c["ds"], c["n_interp"])
    return c, og, c64, c32, unnormalised32(og, c["x"])


# ---- the flag cross-check's batches: colliding and free trajectories, chosen by the reference
N_FLAG = 128            # n_points = n_check of the cross-check
FLAG_BAND = 1e-5
FLAG_CASES = ("RobotPointMass", "RobotPanda", "chain:R3")


def _segments(ds, n, tag, spread=0.9, reach=0.25):
    """normalised fp32 [n, 64, D]: straight joint-space segments from hash-uniform configurations to hash-uniform neighbours within `reach` (of the
    normalised range) per joint, zero noise, small hash-normal velocities"""
    from mpd_public_amd import synthetic as syn
    qd = ds.robot.q_dim
    a = torch.from_numpy(syn.hash_uniform(f"cost_flags/{tag}/a", n * qd, -spread, spread).reshape(n, 1, qd)).float()
    b = (a + reach * torch.from_numpy(syn.hash_uniform(f"cost_flags/{tag}/b", n * qd, -1.0, 1.0).reshape(n, 1, qd)).float()).clamp(-spread, spread)
    s = torch.linspace(0, 1, 64).reshape(1, 64, 1)
    vel = 0.1 * torch.from_numpy(syn.hash_normal(f"cost_flags/{tag}/v", n * 64 * qd).reshape(n, 64, qd)).float()
    return torch.cat([a + (b - a) * s, vel], -1).contiguous()


def flag_slack(robot_id, ds, xu32, n_check=N_FLAG):
    """[B, n_check] fp64 slack (max over every collision hinge at margin = link radius) of un-normalised float32 trajectories"""
    import guide_ref as gr
    from oracle.guide import interpolate_points_v1
    if gr.is_chain(robot_id):
        import chain_ref
        _, comp = gr.oracle_of(ds, dtype=torch.float64)
        return chain_ref.hinge_slack(comp, interpolate_points_v1(xu32.double(), n_check))
    from helpers import oracle_hinge_slack
    return oracle_hinge_slack(ds, xu32.double(), n_check)


_FLAG = {}


def flag_batch(robot_id):
    """(ds (CPU), xu32 [B, 64, D], slack [B, N_FLAG] fp64) of the flag cross-check: 16 obstacle-hugging trajectories (the point mass at scale 0.25, so
    that some are free) and, for the Panda and a chain, up to 6 short straight segments of a scan of 256 whose largest slack is below -1e-3 (free by the
    reference), in each robot's OWN environment (EnvSimple2D / EnvSpheres3D)."""
    if robot_id in _FLAG:
        return _FLAG[robot_id]
    import guide_ref as gr
    import mpd_public_amd as m
    from helpers import obstacle_hugging_trajs
    from oracle.normalizer import LimitsNormalizer
    if gr.is_chain(robot_id):
        ds = gr.metrics_dataset(robot_id, "own")
    else:
        env_id, _ = gr.ROBOTS[robot_id]
        ds = m.TrajectoryDataset(env_id, robot_id, n_support_points=64)
    nrm = LimitsNormalizer(ds.normalizer.mins.cpu().double(), ds.normalizer.maxs.cpu().double())
    un = lambda x: nrm.unnormalize(x.double()).float().contiguous()
    if robot_id == "RobotPointMass":
        xu = un(obstacle_hugging_trajs(ds, 16, seed="cost_flags/pm", scale=0.25))
    else:
        if gr.is_chain(robot_id):
            import chain_ref
            hug = chain_ref.chain_trajs(ds.robot.q_dim, 16, 64, f"cost_flags/{gr.hash_tag(robot_id)}")
        else:
            hug = obstacle_hugging_trajs(ds, 16, seed="cost_flags/panda")
        scan = un(_segments(ds, 256, gr.hash_tag(robot_id)))
        free = flag_slack(robot_id, ds, scan).amax(-1) < -1e-3
        xu = torch.cat([un(hug), scan[free][:6]]).contiguous()
    _FLAG[robot_id] = (ds, xu, flag_slack(robot_id, ds, xu))
    return _FLAG[robot_id]


def flag_classes(slack, band=FLAG_BAND):
    """(collides [B] bool by the reference, decided [B] bool: no checked point within the band of a decision)"""
    return slack.amax(-1) > 0, ~(slack.abs() <= band).any(-1)


# ---- grid fields: a small grid (cell 0.1) over a box SMALLER than the workspace (padding < 0), so that link points leave the box and are clamped
GRID_CELL, GRID_PADDING = 0.1, -0.35
GRID_CASES = [("pm2-H64", "linear"), ("pm2-H64", "nearest"), ("panda", "linear"), ("panda", "nearest")]


def grid_dataset(case, mode, device="cpu"):
    """(primitive dataset, the same with the fixed objects as a grid) of a case of tests/grid_edges_ref.py"""
    import copy
    import grid_edges_ref as ge
    from mpd_public_amd.planning import PlanningTask
    prim = ge.base_dataset(case, device)
    d = copy.copy(prim)
    d.task = PlanningTask(prim.env, prim.robot, obstacle_cutoff_margin=prim.task.obstacle_cutoff_margin, tensor_args=prim.tensor_args,
                          sdf_grid=dict(cell_size=GRID_CELL, mode=mode, padding=GRID_PADDING))
    return prim, d


def grid_oracles(prim, field):
    """(og, comp64, comp32) of the primitive dataset's oracle with the fixed objects' field replaced by `field` (a grid_ref.GridField)"""
    from helpers import oracle_guide
    out = []
    for dtype in (torch.float64, torch.float32):
        og, comp = oracle_guide(prim, *WEIGHTS, dtype=dtype)
        k = [f.name for f in prim.task.get_collision_fields()].index("objects")
        comp.cost_l[k].field = field
        out.append((og, comp))
    return out[0][0], out[0][1], out[1][1]
