"""CPU checks of the cost values (mpdx_traj_costs, PlanningTask.trajectory_costs, GuideManagerTrajectoriesWithVelocity.costs): the reference's clearance
against hand-computed distances and against helpers.oracle_config_slack, the C ABI's refusals on host buffers (no launch), the Python surface without a
device, and - from the reference alone - the conditions the GPU tests (tests/test_gpu_costs.py) put on their inputs."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import cost_ref as cr
import guide_ref as gr

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------------------- the reference's clearance, by hand
class _TwoSpheres:
    """a 'robot' whose configuration IS its two sphere centres (radii 0.1 and 0.2)"""
    q_dim, name = 6, "TwoSpheres"
    radii = torch.tensor([0.1, 0.2], dtype=torch.float64)

    def link_points(self, q):
        return q.reshape(q.shape[:-1] + (2, 3))


def _pm_term(field, dim=2):
    from oracle import costs as oc
    rob = oc.RobotPointMass(dim, 0.01)
    rob.radii = torch.tensor([0.01], dtype=torch.float64)      # (the class keeps a float32 0.01)
    return oc.CostCollision(rob, 64, field=field, cutoff_margin=0.05)


def _at(*p):
    """one trajectory of one point at position p (velocities zero): xi [1, 1, 2 dim]"""
    return torch.tensor([[list(p) + [0.0] * len(p)]], dtype=torch.float64)


def test_reference_clearance_equals_hand_computed_distances():
    from oracle import costs as oc
    e2 = torch.zeros((0, 2), dtype=torch.float64)
    sphere = oc.ObjectField(torch.tensor([[0.5, 0.0]], dtype=torch.float64), torch.tensor([0.2], dtype=torch.float64), e2, e2)
    box = oc.ObjectField(e2, torch.zeros(0, dtype=torch.float64), torch.tensor([[0.0, 0.0]], dtype=torch.float64), torch.tensor([[0.2, 0.1]], dtype=torch.float64))
    ws = oc.WorkspaceField(torch.tensor([-1.0, -1.0], dtype=torch.float64), torch.tensor([1.0, 1.0], dtype=torch.float64))

    def clr(field, *p):
        comp = oc.CostComposite(None, 64, [_pm_term(field)], weights_cost_l=[1.0])
        return float(cr.clearance(comp, _at(*p))[0, 0])
    assert clr(sphere, 0.0, 0.0) == pytest.approx(0.5 - 0.2 - 0.01, abs=1e-15)            # 0.3 from the surface, less the link margin
    assert clr(box, 0.5, 0.0) == pytest.approx(0.3 - 0.01, abs=1e-15)                      # a face
    assert clr(box, 0.5, 0.5) == pytest.approx(0.5 - 0.01, abs=1e-15)                      # a corner: |(0.3, 0.4)|
    assert clr(box, 0.05, 0.0) == pytest.approx(-0.1 - 0.01, abs=1e-15)                    # inside: the nearest face is 0.1 away
    assert clr(ws, 0.7, 0.0) == pytest.approx(0.3 - 0.01, abs=1e-15)                       # the upper x face
    assert clr(ws, 0.0, -1.2) == pytest.approx(-0.2 - 0.01, abs=1e-15)                     # outside the lower y face
    pair = oc.CostCollision(_TwoSpheres(), 64, field=oc.SelfField(torch.tensor([[0, 1]])), cutoff_margin=0.05)
    comp = oc.CostComposite(None, 64, [pair], weights_cost_l=[1.0])
    xi = torch.tensor([[[0.0, 0.0, 0.0, 1.0, 0.0, 0.0] + [0.0] * 6], [[0.0, 0.0, 0.0, 0.0, 0.25, 0.0] + [0.0] * 6]], dtype=torch.float64)
    got = cr.clearance(comp, xi)[:, 0]
    assert float(got[0]) == pytest.approx(1.0 - 0.3, abs=1e-15) and float(got[1]) == pytest.approx(0.25 - 0.3, abs=1e-15)
    # the minimum runs over the points of a trajectory, and the point costs are the hinges at margin = radius + cutoff
    two = torch.cat([_at(0.0, 0.0), _at(0.2, 0.0)], 1)
    comp = oc.CostComposite(None, 64, [_pm_term(sphere)], weights_cost_l=[1.0])
    assert float(cr.clearance(comp, two)[0, 0]) == pytest.approx(0.1 - 0.01, abs=1e-15)
    assert cr.point_costs(comp, two)[0, :, 0].tolist() == [0.0, 0.0]                                   # 0.3 and 0.1 away: beyond the margin 0.06
    assert cr.point_costs(comp, _at(0.28, 0.0))[0, 0, 0] == pytest.approx(0.06 - 0.02, abs=1e-15)


@pytest.mark.parametrize("robot_id,H", [("RobotPointMass", 64), ("RobotPointMass3D", 24), ("RobotPanda", 64)])
def test_reference_clearance_over_the_fields_is_minus_the_config_slack(robot_id, H):
    from helpers import oracle_config_slack
    c, og, c64, _, xu = cr.term_case(robot_id, H)
    ref = cr.evaluate(c64, xu, c["n_interp"])
    qd = c["ds"].robot.q_dim
    slack = oracle_config_slack(c["ds"], ref["xi"][..., :qd]).amax(-1)
    assert torch.allclose(ref["clearance"].amin(-1), -slack, rtol=0, atol=1e-13)
    assert torch.allclose(ref["point_costs"].sum(1), ref["terms"][:, :-1], rtol=1e-12, atol=1e-12)      # the point costs sum to the terms


# ---------------------------------------------------------------------------------------------------------------- the C ABI, no launch
@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbol_and_its_ten_arguments(lib):
    from mpd_public_amd import _lib
    res, args = _lib.SIGNATURES["mpdx_traj_costs"]
    assert res is C.c_int and len(args) == 10 and lib.mpdx_traj_costs.argtypes == args
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mpdx.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+mpdx_traj_costs\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(decl.split(",")) == 10
    slots = [int(n) for name, n in re.findall(r"#define (\w+) \(\w+_MAX_FIELDS \+ (\d+)\)", text) if name.endswith("_COST_SLOTS")]     # the header's slot count
    assert len(slots) == 1 and slots[0] + _lib.MAX_FIELDS == _lib.COST_SLOTS == 6


def _pm_block():
    """a well-formed 2-D point-mass block over HOST memory (the entry point checks it before anything is launched)"""
    from mpd_public_amd import _lib
    gp = _lib.GuideParams()
    gp.robot, gp.q_dim, gp.ws_dim, gp.interpolate, gp.n_interp, gp.n_fields = _lib.ROBOT_POINTMASS, 2, 2, 1, 128, 2
    gp.cutoff_margin, gp.link_margin = 0.05, 0.01
    f = gp.fields[0]
    f.kind, f.weight, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 1.0, 0, 2, 8, 0
    gp.fields[1].kind = _lib.FIELD_WORKSPACE
    keep = [(C.c_float * 2048)(), (C.c_int32 * 4)()]
    gp.prims, gp.n_prim_floats = C.addressof(keep[0]), 8
    gp._keep = keep
    return gp


def _call(lib, gp, x=True, cost=True, n_points=128, B=4, H=64, D=4):
    buf = (C.c_float * (4 * 64 * 16))()
    out = (C.c_float * 64)()
    a = lambda b: C.cast(b, C.c_void_p)
    rc = lib.mpdx_traj_costs(C.byref(gp) if gp is not None else None, a(buf) if x else None, a(out) if cost else None, None, None, n_points, B, H, D, None)
    return rc, (lib.mpdx_last_error() or b"").decode()


def test_refusals_name_the_argument(lib):
    from mpd_public_amd import _lib
    from test_chain_cpu import _valid_block
    cases = []

    def case(what, expect, gp=None, **kw):
        cases.append((what, expect, _pm_block() if gp is None else gp, kw))
    rc, msg = _call(lib, None)
    assert rc == -1 and "gp" in msg, msg
    case("null x", "x_unnormalised", x=False)
    case("null cost_out", "cost_out", cost=False)
    case("B = 0", "B", B=0)
    case("D != 2 q_dim", "D", D=6)
    case("H = 1", "H", H=1)
    for n in (1, -1, 8193):
        case(f"n_points {n}", "n_points", n_points=n)
    gp = _pm_block(); gp.n_interp = 9000
    case("n_points 0 takes a bad n_interp", "n_interp", gp, n_points=0)
    case("LDS", "LDS", H=20000)                                           # 20000 x 4 floats of state: 320 KB
    gp = _pm_block(); gp.n_fields = 5
    case("n_fields", "n_fields", gp)
    gp = _pm_block(); gp.prims = None
    case("no primitive table", "primitive", gp)
    gp = _pm_block(); gp.fields[0].kind = _lib.FIELD_GRID                 # a grid field without a grid buffer
    case("grid descriptor", "grid", gp)
    gp = _pm_block(); gp.n_scenes, gp.scene_stride = 2, 16                # scenes without a scene table
    case("scene members", "scene", gp)
    gp = _pm_block(); gp.fields[0].track_len, gp.fields[0].track_off = 32, 8      # a track of another horizon
    case("track_len != H", "track_len", gp)
    gp = _pm_block(); gp.fields[0].track_len, gp.fields[0].track_off, gp.n_prim_floats = 64, 8, 8 + 4 * 64
    gp.n_scenes, gp.scene_stride = 2, 16
    case("track + scenes", "track_len", gp)
    gp = _pm_block(); gp.tool_frame = 1
    case("tool term on a built-in robot", "tool_frame", gp)
    for what, change in (("bad chain table", lambda g, t: t.view(np.int32).__setitem__(1, 17)), ("chain + grid", lambda g, t: setattr(g.fields[0], "kind", _lib.FIELD_GRID)),
                         ("chain without a table", lambda g, t: setattr(g, "chain", None))):
        gp, tab = _valid_block()
        change(gp, tab)
        case(what, "chain", gp, D=6)
    gp, _ = _valid_block(); gp.fields[0].track_len, gp.fields[0].track_off, gp.n_prim_floats = 64, 20, 20 + 4 * 64
    case("chain + track", "MPDX_ROBOT_CHAIN", gp, D=6)
    gp, _ = _valid_block(); gp.tool_frame = 4
    case("tool_frame beyond the joints", "tool_frame", gp, D=6)
    gp, _ = _valid_block(); gp.tool_frame = 2; gp.tool_axis[2] = 1.0; gp.tool_world[2] = 0.5
    case("tool_world not unit", "tool_world", gp, D=6)
    assert len(cases) == 23
    for what, expect, gp, kw in cases:
        rc, msg = _call(lib, gp, **kw)
        assert rc == -1 and expect in msg, (what, rc, msg)


# ---------------------------------------------------------------------------------------------------------------- the Python surface without a device
def test_term_order_weights_and_slots_of_a_shuffled_composite():
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    from mpd_public_amd.guides import build_device_params
    from mpd_public_amd.planning import TrajectoryCosts, as_cost_composite, cost_term_slots
    ds = gr.cover_dataset("RobotPointMass", 64)
    comp = cr.product_composite(ds, weights=(0.5, 0.25), shuffle=[2, 3, 0, 1])        # extra objects, GP prior, objects, workspace
    names, slots = cost_term_slots(comp.cost_l)
    assert names == ["extra_objects", "gp", "objects", "workspace"] and slots == [0, 4, 1, 2]
    gp, _ = build_device_params(ds.robot, 2, 0.05, None, None, comp.cost_l, comp.weight_cost_l, True, 128, True, 1.0, "cpu")
    assert [gp.fields[k].kind for k in range(3)] == [_lib.FIELD_OBJECTS, _lib.FIELD_OBJECTS, _lib.FIELD_WORKSPACE] and gp.n_fields == 3
    assert gp.fields[0].n_spheres == len(ds.env.obj_extra.sphere_radii) and gp.fields[1].n_spheres == len(ds.env.obj_fixed.sphere_radii)     # slot 0 IS the extras
    B, N = 2, 3
    raw = torch.arange(B * 6, dtype=torch.float32).reshape(B, 6)
    clr = torch.arange(B * 4, dtype=torch.float32).reshape(B, 4) - 2.0
    pts = torch.arange(B * N * 5, dtype=torch.float32).reshape(B, N, 5)
    tc = TrajectoryCosts.from_slots(comp, raw, clr, pts)
    assert tc.names == names and tc.weights.tolist() == [0.5, 0.25, 0.5, 0.5]
    assert torch.equal(tc.terms, raw[:, [0, 4, 1, 2]]) and torch.equal(tc.total, tc.terms @ tc.weights)
    assert torch.equal(tc.clearance, clr[:, :3]) and torch.equal(tc.point_costs, pts[..., :3]) and torch.equal(tc.min_clearance, clr[:, :3].amin(-1))
    bare = TrajectoryCosts.from_slots(comp, raw)
    assert bare.clearance is None and bare.point_costs is None and bare.min_clearance is None
    # a single term is wrapped with weight 1; a tool term adds the last point column
    one = as_cost_composite(comp.cost_l[1])
    assert isinstance(one, m.CostComposite) and one.cost_l == [comp.cost_l[1]] and one.weight_cost_l == [1.0] and as_cost_composite(comp) is comp
    assert cost_term_slots(one.cost_l) == (["gp"], [4])
    rob = m.RobotChain.panda()
    tool = m.CostToolAxis(rob, 64, max_tilt=0.3)
    mixed = m.CostComposite(rob, 64, [tool, m.CostGPTrajectory(rob, 64, 0.1)], weights_cost_l=[2.0, 3.0])
    tm = TrajectoryCosts.from_slots(mixed, raw, clr, pts)
    assert tm.names == ["tool_axis", "gp"] and torch.equal(tm.terms, raw[:, [5, 4]]) and tm.clearance.shape == (B, 0) and tm.min_clearance is None
    assert torch.equal(tm.point_costs, pts[..., 4:5])
    assert "TrajectoryCosts" in m.__all__ and m.TrajectoryCosts is TrajectoryCosts


def test_errors_of_the_python_surface_without_a_device():
    import mpd_public_amd as m
    import moving_ref as mr
    from helpers import toy_cost
    ds = gr.cover_dataset("RobotPointMass", 64)
    comp = cr.product_composite(ds)
    x = torch.zeros((2, 64, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ds.task.trajectory_costs(x, comp)
    with pytest.raises(RuntimeError, match="GPU"):
        ds.task.trajectory_costs(x, comp.cost_l[0])
    other = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass")
    with pytest.raises(ValueError, match="another robot"):
        other.task.trajectory_costs(x, comp)
    with pytest.raises(TypeError):
        ds.task.trajectory_costs(x, toy_cost)
    with pytest.raises(ValueError, match=r"\[B, H, D\]"):
        ds.task.trajectory_costs(x[0], comp)
    moving = mr.dataset("pm2-H64")                                   # a task with a track: H against the track BEFORE the device is asked for
    with pytest.raises(ValueError, match="track"):
        moving.task.trajectory_costs(torch.zeros((2, 32, 4)), mr.product(moving).cost)
    with pytest.raises(RuntimeError, match="GPU"):
        moving.task.trajectory_costs(x, mr.product(moving).cost)
    guide = gr.product_run(ds, dict(weights=cr.WEIGHTS, only=None, clip_grad=True, gp_half_factor=False))
    with pytest.raises(RuntimeError, match="GPU"):
        guide.costs(x)
    with pytest.raises(NotImplementedError, match="callable"):
        m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost).costs(x)
    scenes = m.PlanningScenes(ds.task, [m.ObjectSet.empty(), m.ObjectSet.empty()])
    with pytest.raises(RuntimeError, match="GPU"):
        scenes.trajectory_costs(x, comp, [0, 1], 1)


def test_experiment_reports_costs_only_on_request():
    from mpd_public_amd import inference
    assert inspect.signature(inference.experiment).parameters["report_costs"].default is False
    src = inspect.getsource(inference.experiment)
    body = src[src.index("    if report_costs:"):]
    block = body[:body.index("    if results_dir:")]
    for key in ("cost_guide_trajs_final", "cost_guide_terms_trajs_final", "min_clearance_trajs_final"):
        assert src.count(f'results_data_dict["{key}"]') == 1 and f'results_data_dict["{key}"]' in block, key       # (written under the switch only)
    assert "idx_best_traj = torch.argmin(cost_all).item()" in src                                                # the reference's rule, untouched


# ---------------------------------------------------------------------------------------------------------------- conditions of the GPU tests
FEW = {("RobotPanda", "self"): (5, 22), ("chain:R3", "self"): (2, 13)}       # slots that only a few trajectories reach


@pytest.mark.parametrize("robot_id,H", cr.SLOT_CASES, ids=[f"{r.replace('chain:', '')}-H{h}" for r, h in cr.SLOT_CASES])
def test_every_slot_is_reached_by_the_coverage_trajectories(robot_id, H):
    c, og, c64, c32, xu = cr.term_case(robot_id, H)
    ref, allow, err32 = cr.yardstick(c64, c32, xu, c["n_interp"])
    names = gr.term_names(c["ds"])
    hit = (ref["terms"] != 0).sum(0).tolist()
    print(f"{robot_id} H={H}: B = {xu.shape[0]}; trajectories with a non-zero cost per term: {dict(zip(names, hit))}; fp32-oracle error per term: "
          f"{[f'{e:.2e}' for e in err32.tolist()]}; largest |term|: {[f'{v:.4g}' for v in ref['terms'].abs().amax(0).tolist()]}")
    for k, nm in enumerate(names):
        if nm in gr.ZERO_RUNS.get(robot_id, ()):
            assert hit[k] == 0 and not ref["terms"][:, k].any() and float(allow["terms"][:, k].max()) == 0.0, nm        # exactly zero, and held to it
            assert float(ref["clearance"][:, k].min()) > c["ds"].task.obstacle_cutoff_margin
        else:
            assert hit[k] > 0, nm
        if (robot_id, nm) in FEW:
            assert (hit[k], xu.shape[0]) == FEW[(robot_id, nm)], (nm, hit[k])
    # the yardstick is not a licence: the fp32 oracle is within 2e-5 of the fp64 one on every term, relative to the term's largest value
    big = ref["terms"].abs().amax(0).clamp_min(1e-30)
    assert float((err32 / big).max()) < 2e-5, (err32 / big).tolist()
    assert float(ref["clearance"].min()) < 0 and bool(torch.isfinite(ref["point_costs"]).all())


@pytest.mark.parametrize("robot_id", cr.FLAG_CASES)
def test_flag_batches_hold_both_classes(robot_id):
    ds, xu, slack = cr.flag_batch(robot_id)
    collides, decided = cr.flag_classes(slack)
    n_c, n_f = int((collides & decided).sum()), int((~collides & decided).sum())
    print(f"{robot_id}: {xu.shape[0]} trajectories, {n_c} colliding, {n_f} free, {int((~decided).sum())} within 1e-5 of a decision")
    assert slack.shape == (xu.shape[0], cr.N_FLAG) and n_c >= 3 and n_f >= 3
    assert float((~decided).double().mean()) <= 0.10
