"""CPU self-test of the chain cases of tests/guide_ref.py: the proof that the cases of tests/test_gpu_chain_terms.py can fail.

A chain case is TrajectoryDataset("EnvSpheres3D", RobotChain, H) with the coverage environment (5 + 1 spheres, 3 + 1 boxes, a shrunk workspace) and
the oracle on the reference forward kinematics of tests/chain_ref.py.  Asserted from the reference alone: the reference-only conditions of every
case (every reachable decision class active, the ambiguous share under the Panda's 2 % cap, the float32 oracle inside the yardstick on every
non-ambiguous waypoint of every run, max|x| away from the normaliser's range test), the declared unreachable classes, MUTANTS of the float32 oracle
- each a plausible bug of the table walk of csrc/chain.hpp - that the runs of the GPU module must reject, and mutants of the metrics flags.  For
every increment mutant the table also says whether the OLD rule of tests/test_gpu_chain.py (at most 1 % of the waypoints outside the yardstick, on
that file's inputs: EnvSpheres3D, B = 3, the composite at the default weights) passes it.
"""
import numpy as np
import pytest
import torch

import chain_ref as cr
import guide_ref as gr
from test_guide_ref_cpu import (_term, m_box_second_axis, m_drop_last_box, m_drop_pair, m_face, m_gp_dropped, m_no_cutoff, m_radius)

C = gr.CHAIN


# ---------------------------------------------------------------------------------------------------------------- the robots
@pytest.mark.parametrize("k,n_spheres,n_pairs", [(2, 5, 0), (4, 9, 0), (5, 11, 4), (6, 13, 12)])
def test_truncations_of_R8(k, n_spheres, n_pairs):
    """R8[:k]: the first k joints, the spheres whose frame is at most k, the pairs among them; the product's table holds the same robot (its
    float64 host FK against the reference FK of the description)."""
    full, d = cr.description("R8"), cr.description(f"R8[:{k}]")
    assert len(d["joints"]) == k and len(d["spheres"]) == n_spheres and len(d["pairs"]) == n_pairs
    assert all(sp[0] <= k for sp in d["spheres"]) and max(sp[0] for sp in d["spheres"]) == k
    assert d["spheres"] == full["spheres"][:n_spheres]         # the spheres are ordered by frame: the renumbering is the identity
    assert d["pairs"] == [p for p in full["pairs"] if max(p) < n_spheres]
    rob, ref = cr.product_robot(f"R8[:{k}]"), cr.RobotChainRef(d)
    assert rob.q_dim == k and rob.n_spheres == n_spheres and rob.n_pairs == n_pairs
    q = cr.t(f"trunc/{k}", (5, k), "uniform").double()
    pts = ref.link_points(q)
    for s, (frame, off, _r) in enumerate(d["spheres"]):
        np.testing.assert_allclose(rob.fk(q, frame=frame, offset=off)[0].numpy(), pts[:, s].numpy(), rtol=0, atol=1e-12)


def test_every_joint_count_has_a_case():
    counts = {gr.cover_dataset(r).robot.q_dim for r, _, _ in gr.CHAIN_CASES}
    assert counts == set(range(1, 9)), counts
    assert {r for r, _, _ in gr.CHAIN_CASES} == set(gr.CHAIN_ROBOTS)


@pytest.mark.parametrize("robot_id", gr.CHAIN_ROBOTS)
def test_unreachable_classes_are_the_declared_constant(robot_id):
    labels, q, missing = gr.probe_configs(robot_id)
    print(f"{robot_id}: {len(labels)} reachable classes, unreachable: {missing}")
    assert tuple(missing) == gr.UNREACHABLE[robot_id]
    rob = gr.cover_dataset(robot_id).robot
    assert len(labels) + len(missing) == (8 + 2) + 2 * (rob.n_spheres + 1) + 6 + rob.n_pairs      # primitives, links + inbox per objects field, faces, pairs
    if robot_id == C + "Panda":
        assert gr.UNREACHABLE[robot_id] == gr.UNREACHABLE["RobotPanda"]
    if robot_id == C + "R8":      # 9 of the 24 pairs close; every sphere but the two of the base frame reaches a margin
        assert sum("pair" in k for k in labels) == 9 and sum(k.startswith("f1 link") for k in labels) == 14


# ---------------------------------------------------------------------------------------------------------------- conditions of the GPU cases
@pytest.mark.parametrize("robot_id,H,seed", gr.CHAIN_CASES, ids=gr.CHAIN_IDS)
def test_reference_conditions_of_every_chain_case(robot_id, H, seed):
    """... and the float32 oracle's own figure for every run but the un-clipped GP prior alone: no non-ambiguous waypoint outside the yardstick."""
    c = gr.check_reference_conditions(robot_id, H, seed)
    ds = c["ds"]
    assert c["x"].shape[0] <= 26
    for k, (name, run) in enumerate(gr.runs_of(ds)):
        if gr.is_unclipped_gp(ds, run):
            continue    # (test_fp32_oracle_error_on_the_unclipped_gp_prior_alone)
        ref = gr.case_reference(robot_id, H, k, seed)
        assert (np.abs(ref).max() > 0) != gr.run_is_zero(robot_id, ds, run), name
        got32 = gr.oracle_run(ds, c["x"], run, torch.float32, c["n_interp"])
        fig = gr.judge(got32, ref, gr.run_ambiguity(run, ds, c["amb"]), run["weights"][0], f"{robot_id} H={H} {name}: fp32 oracle")
        assert fig["differ_outside"] == 0


def test_seed_of_R3_H24():
    """R3 H = 24 is the one case that seed "0" leaves over the cap (8 of 312 waypoints, 2.56 %); its seed is the first that meets it."""
    assert float(gr.case(C + "R3", 24, "0")["amb"].mean()) > gr.cap_of(C + "R3")
    assert (C + "R3", 24, "1") in gr.CHAIN_CASES and all(s == "0" for r, h, s in gr.CHAIN_CASES if (r, h) != (C + "R3", 24))


# ---------------------------------------------------------------------------------------------------------------- mutants of the increment
def _set_robot(comp, robot):
    for c in comp.cost_l:
        if hasattr(c, "robot"):
            c.robot = robot


def m_pair_sign(p):
    """pair p pulls its sphere a where it should push it (the sign of the force on a swapped; the value is kept).  Member a, not b: the second
    members of R8's reachable pairs 5 and 21 are base-frame spheres, on which a force moves no joint"""
    def mutate(og, comp):
        term = _term(comp, "self")

        def factors(trajs):
            rob, pr = term.robot, term.field.pairs
            pts, r = rob.link_points(trajs[..., : rob.q_dim]), rob.radii.to(trajs.dtype)
            a, b = pts[..., pr[:, 0], :], pts[..., pr[:, 1], :]
            sel = (torch.arange(len(pr)) == p).unsqueeze(-1)
            a = torch.where(sel, 2 * a.detach() - a, a)
            return torch.relu(r[pr[:, 0]] + r[pr[:, 1]] - torch.linalg.norm(a - b, dim=-1))
        term.factors = factors
    return mutate


def m_sphere_frame_down(s):
    """sphere s rides on the frame below its own"""
    def mutate(og, comp):
        rob = comp.cost_l[0].robot
        desc = dict(rob.desc)
        frame, off, r = desc["spheres"][s]
        assert frame >= 1
        desc["spheres"] = desc["spheres"][:s] + [(frame - 1, off, r)] + desc["spheres"][s + 1:]
        new = cr.RobotChainRef(desc, rob.dtype)
        new.radii = rob.radii
        _set_robot(comp, new)
    return mutate


class _FoldedAsRevolute(cr.RobotChainRef):
    """the forward kinematics of the description with the GRADIENT of prismatic joint j taken as a revolute joint's (a rotation about the joint's z
    by q_j - q_j: the identity in value, d/dq_j of a rotation)"""

    def frames(self, q):
        q = q.to(self.dtype)
        j = self.as_revolute
        assert self.fixed[j][1]
        out = super().frames(torch.cat([q[..., :j], q[..., j:j + 1].detach(), q[..., j + 1:]], -1))
        a = q[..., j] - q[..., j].detach()
        z, o = torch.zeros_like(a), torch.ones_like(a)
        c, s = torch.cos(a), torch.sin(a)
        Rz = torch.stack([torch.stack([c, -s, z, z], -1), torch.stack([s, c, z, z], -1), torch.stack([z, z, o, z], -1), torch.stack([z, z, z, o], -1)], -2)
        # frames above joint j: T_k = T_j Rz (T_j^-1 T_k), T_j the frame of joint j itself (index j + 1; index 0 is the base)
        Tj = out[j + 1]
        return out[: j + 1] + [Tj @ Rz @ torch.linalg.solve(Tj, T) if k > 0 else Tj @ Rz for k, T in enumerate(out[j + 1:])]


def m_prismatic_as_revolute(j):
    def mutate(og, comp):
        rob = comp.cost_l[0].robot
        new = _FoldedAsRevolute(rob.desc, rob.dtype)
        new.as_revolute, new.radii = j, rob.radii
        _set_robot(comp, new)
    return mutate


# per robot: (a sphere on the link of a prismatic joint, a sphere on the link of a revolute joint, the prismatic joint (0-based), a sphere whose
# radius / cutoff margin is changed) - all with reachable hinges
_PICKS = {"R3": dict(on_prismatic=2, on_revolute=3, prismatic=1, radius=3, cutoff=4), "R8": dict(on_prismatic=5, on_revolute=7, prismatic=2, radius=9, cutoff=12)}


def _mutants(name):
    robot_id = C + name
    labels, _, _ = gr.probe_configs(robot_id)
    pk = _PICKS[name]
    desc = cr.description(name)
    assert desc["joints"][desc["spheres"][pk["on_prismatic"]][0] - 1][2] == "prismatic" and desc["joints"][desc["spheres"][pk["on_revolute"]][0] - 1][2] == "revolute"
    assert desc["joints"][pk["prismatic"]][2] == "prismatic"
    pairs = [int(k.split("pair")[1]) for k in labels if "pair" in k]
    out = [(f"self pair {p} dropped", m_drop_pair(p)) for p in pairs]
    out += [(f"self pair {p}: sign of the force on a swapped", m_pair_sign(p)) for p in sorted({pairs[0], pairs[-1]})]
    out += [(f"sphere {pk['on_prismatic']} (on a prismatic joint's link) one frame down", m_sphere_frame_down(pk["on_prismatic"])),
            (f"sphere {pk['on_revolute']} (on a revolute joint's link) one frame down", m_sphere_frame_down(pk["on_revolute"])),
            (f"prismatic joint {pk['prismatic']} folded as a revolute joint", m_prismatic_as_revolute(pk["prismatic"])),
            ("one link radius x 0.9", m_radius(pk["radius"])), ("cutoff margin left off one link sphere", m_no_cutoff(pk["cutoff"])),
            ("last fixed box dropped", m_drop_last_box), ("box interior axis = second-largest d_j", m_box_second_axis)]
    for j in range(3):
        for upper in (False, True):
            if f"f2 face{j}{'+' if upper else '-'}" in labels:
                out.append((f"{'upper' if upper else 'lower'} face of axis {j} moved away", m_face(j, upper)))
    return out + [("GP term dropped", m_gp_dropped)]


OLD_SEED, OLD_W = "0", (1e-2, 1e-7)


def _old_rule_passes(name, H, mutate, cache={}):
    """the rule tests/test_gpu_chain.py used so far, on its inputs (chain_ref.chain_case_inputs: EnvSpheres3D, B = 3, SEED "0"): at most 1 % of the
    waypoints outside the yardstick, float32 mutant against the float64 oracle at the default weights"""
    if (name, H) not in cache:
        ds, desc, x = cr.chain_case_inputs(name, H, OLD_SEED)
        cache[name, H] = (ds, desc, x, cr.oracle_guide_chain(ds, desc, *OLD_W, dtype=torch.float64)[0](x.double()).numpy())
    ds, desc, x, ref = cache[name, H]
    og, comp = cr.oracle_guide_chain(ds, desc, *OLD_W, dtype=torch.float32)
    mutate(og, comp)
    frac, bad = cr.mismatch_fraction(og(x.float()).numpy(), ref, OLD_W[0])
    return bool(frac <= 0.01), int(bad.sum()), bad.size


@pytest.mark.parametrize("name", ["R3", "R8"])
def test_every_mutant_of_the_fp32_oracle_is_rejected(name):
    robot_id, H = C + name, 64
    c = gr.check_reference_conditions(robot_id, H)
    ds, x = c["ds"], c["x"]
    runs = gr.runs_of(ds)
    table, survivors, old_passes = [], [], {}
    for mname, mutate in _mutants(name):
        by = None
        for k, (run_name, run) in enumerate(runs):
            if gr.is_unclipped_gp(ds, run):
                continue    # (the float32 oracle itself misses the yardstick there: that run would "reject" every mutant)
            got = gr.oracle_run(ds, x, run, torch.float32, c["n_interp"], mutate=mutate)
            if gr.rejected(got, gr.case_reference(robot_id, H, k), gr.run_ambiguity(run, ds, c["amb"]), run["weights"][0]):
                by = run_name
                break
        ok, n_bad, n_all = _old_rule_passes(name, H, mutate)
        old_passes[mname] = (ok, n_bad)
        table.append(f"  {mname:62s} rejected by: {by or 'NOTHING':34s} old rule on the old inputs: {'PASSES' if ok else 'rejects'} ({n_bad} of {n_all} waypoints)")
        if by is None:
            survivors.append(mname)
    print(f"mutants of the float32 oracle, {name} H={H}:\n" + "\n".join(table))
    assert not survivors, survivors
    # what the old rule could not see on its own inputs: the boxes (EnvSpheres3D has none) and the GP term change no waypoint
    for mname in ("last fixed box dropped", "box interior axis = second-largest d_j", "GP term dropped"):
        assert old_passes[mname] == (True, 0), (mname, old_passes[mname])
    print(f"  the old rule passes {sum(ok for ok, _ in old_passes.values())} of {len(old_passes)} mutants")


def test_mutants_are_the_same_function_in_value():
    """the sign swap and the revolute fold change the gradient alone: the cost of the mutated oracle equals the oracle's"""
    c = gr.case(C + "R3", 64)
    from oracle.guide import interpolate_points_v1
    for mutate in (m_pair_sign(1), m_prismatic_as_revolute(1)):
        og, comp = gr.oracle_of(c["ds"], dtype=torch.float64, n_interp=c["n_interp"])
        og2, comp2 = gr.oracle_of(c["ds"], dtype=torch.float64, n_interp=c["n_interp"])
        mutate(og2, comp2)
        xu = og.normalizer.unnormalize(c["x"].double())
        xi = interpolate_points_v1(xu, c["n_interp"])
        a, b = comp(xu, x_interpolated=xi), comp2(xu, x_interpolated=xi)
        assert float(a.abs().max()) > 0
        np.testing.assert_allclose(b.detach().numpy(), a.numpy(), rtol=1e-12)
        assert not np.array_equal(og2(c["x"].double()).numpy(), og(c["x"].double()).numpy())


# ---------------------------------------------------------------------------------------------------------------- metrics
# metrics mutants that change no decided flag of the reference, by name, with the reason (asserted equal to what the reference finds)
_R8_COVER = ("every checked point collides twice over, whatever the joints do (guide_ref.METRICS_ALL_COLLIDE): the base-frame spheres 0 and 1 lie 0.07 and "
             "0.064 under the lower z face, and sphere 2, almost on joint 0's axis, 0.003 inside fixed sphere 0")
_R8_PAIRS = tuple(f"self pair {p} dropped" for p in (5, 6, 8, 9, 10, 11, 12, 16, 21))
METRICS_BLIND = {
    (C + "R8", "cover"): (_R8_COVER, ("objects fields dropped", "workspace dropped", "self field dropped") + _R8_PAIRS),
    (C + "R8[:4]", "cover"): (_R8_COVER, ("objects fields dropped", "workspace dropped")),
    (C + "Panda", "cover"): ("the hand's spheres 8, 9 and 10 lie within 0.17 of each other: wherever one of their pairs closes alone in its field, another "
                             "pair closes with it (the self field as a whole decides 221 flags)", tuple(f"self pair {p} dropped" for p in (0, 1, 3, 4, 7, 8, 9))),
    (C + "R8", "own"): ("the pairs of the tip spheres 10 ... 15 against the base spheres close together; pair 10 alone decides flags (41), the field 118",
                        tuple(p for p in _R8_PAIRS if p != "self pair 10 dropped")),
    (C + "R8[:4]", "own"): ("four joints do not reach the faces at +-1: no workspace hinge is active", ("workspace dropped",)),
}


def _flag_mutants(robot_id, slacks):
    """(slack [B, n_check], [(name, slack of a metrics evaluation with one piece missing)])"""
    kinds = [k for k, _ in slacks]
    each = [s.amax(-1) for _, s in slacks]

    def without(drop):
        return torch.stack([e for i, e in enumerate(each) if i not in drop]).amax(0)
    out = [("objects fields dropped", without({i for i, k in enumerate(kinds) if k == "objects"})),
           ("workspace dropped", without({kinds.index("workspace")}))]
    if "self" in kinds:
        i = kinds.index("self")
        out.append(("self field dropped", without({i})))
        labels, _, _ = gr.probe_configs(robot_id)
        for p in [int(k.split("pair")[1]) for k in labels if "pair" in k]:
            s = slacks[i][1]
            keep = torch.arange(s.shape[-1]) != p
            out.append((f"self pair {p} dropped", torch.maximum(without({i}), s[..., keep].amax(-1))))
    full = without(set())
    last = full.clone()
    last[:, -1] = -float("inf")
    return full, out + [("last checked point skipped", last)]


@pytest.mark.parametrize("robot_id,env", gr.METRICS_CASES, ids=[f"{r[len(C):]}-{e}" for r, e in gr.METRICS_CASES])
def test_metrics_flags_can_see_each_field(robot_id, env):
    """The reference conditions of the metrics comparison (tests/test_gpu_chain_terms.py), and: a metrics evaluation without the self field, the
    objects fields, the workspace, one reachable pair or the last checked point changes at least one DECIDED flag of the reference - or is listed
    in METRICS_BLIND."""
    _, slacks = gr.chain_metrics_reference(robot_id, env)
    full, mutants = _flag_mutants(robot_id, slacks)
    assert torch.equal(full, cr.hinge_slack(*_comp_and_xi(robot_id, env)))
    gr.check_metrics_conditions(full, (robot_id, env) in gr.METRICS_ALL_COLLIDE, f"{robot_id} {env}")
    decided = full.abs() > gr.DELTA
    blind = []
    for name, s in mutants:
        n = int((((s > 0) != (full > 0)) & decided).sum())
        print(f"  {robot_id} {env}: {name}: changes {n} decided flags")
        if n == 0:
            blind.append(name)
    assert tuple(blind) == METRICS_BLIND.get((robot_id, env), ("", ()))[1], blind


def _comp_and_xi(robot_id, env, n_check=256):
    from oracle.guide import interpolate_points_v1
    xu32, _ = gr.chain_metrics_reference(robot_id, env)
    return gr.oracle_of(gr.metrics_dataset(robot_id, env), dtype=torch.float64)[1], interpolate_points_v1(xu32.double(), n_check)
