"""GPU parity of the primitive-field guide and metrics kernels (csrc/guide.hpp: guide_step_kernel, guide_step_panda_kernel, traj_metrics_kernel) against
the fp64 oracle, term by term, on inputs that reach every decision of every collision term (tests/guide_ref.py; the CPU proof that these cases can
fail is tests/test_guide_ref_cpu.py).

Rule: every support waypoint that is not AMBIGUOUS - decided from the fp64 reference alone: an interpolated point that contributes to it lies within
1e-5 of a hinge, an arg-min tie, a box-interior axis tie or centre plane, or a sphere centre - must agree under the yardstick of DESIGN.md section 6
(1e-3 relative, 2e-6 * max(w, 1e-2) / 1e-2 absolute); none is left out.  The share of ambiguous waypoints is capped (1 % point mass, 2 % Panda), and
the reference-only conditions are asserted before the kernel's output is looked at.

Runs of a case: the composite at the weights (1e-2, 1e-7) and (1.0, 1e-4), then a product guide with ONE cost term at weight 1.0 - each collision
field alone, the GP prior alone (gp_half_factor both ways) - with the norm clip on and off.  Every run prints its figures next to the float32
oracle's own error for the same run (the lines that profiles/guide_terms.md tabulates).
"""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import guide_ref as gr
from helpers import oracle_guide, oracle_hinge_slack, t

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

IDS = [f"{r}-H{h}" for r, h in gr.GPU_CASES]


@functools.lru_cache(maxsize=None)
def _gpu_dataset(robot_id, H):
    return gr.cover_dataset(robot_id, H, "cuda")


def _increment(robot_id, H, run):
    c = gr.case(robot_id, H)
    pg = gr.product_run(_gpu_dataset(robot_id, H), run, c["n_interp"]).cuda()
    return pg(c["x"].cuda()).cpu().numpy()


def _oracle32_error(robot_id, H, k, run):
    c = gr.case(robot_id, H)
    return float(np.abs(gr.oracle_run(c["ds"], c["x"], run, torch.float32, c["n_interp"]) - gr.case_reference(robot_id, H, k)).max())


def _judge_run(robot_id, H, k, name, run, got, tag=""):
    c = gr.case(robot_id, H)
    ref = gr.case_reference(robot_id, H, k)
    assert got.shape == ref.shape == tuple(c["x"].shape) and np.abs(ref).max() > 0
    e32 = _oracle32_error(robot_id, H, k, run)
    try:
        fig = gr.judge(got, ref, gr.run_ambiguity(run, c["ds"], c["amb"]), run["weights"][0], f"{robot_id} H={H}{tag} {name}")
    finally:
        d = np.abs(got - ref)
        print(f"GUIDE-TERMS | {robot_id} H={H}{tag} | {name} | max|diff| all waypoints {d.max():.3e} | float32 oracle max|diff| {e32:.3e}")
    return fig


# ---------------------------------------------------------------------------------------------------------------- 1. increments
@pytest.mark.parametrize("robot_id,H", gr.GPU_CASES, ids=IDS)
def test_increment_composite_and_every_term_alone_vs_oracle(robot_id, H):
    """Gradient-only mode: the composite at both weight pairs and every cost term alone (clip on / off), every non-ambiguous waypoint inside the
    yardstick.  (The GP prior alone with the clip off: test_unclipped_gp_alone_vs_oracle.)"""
    c = gr.check_reference_conditions(robot_id, H)
    for k, (name, run) in enumerate(gr.runs_of(c["ds"])):
        if gr.is_unclipped_gp(c["ds"], run):
            continue
        _judge_run(robot_id, H, k, name, run, _increment(robot_id, H, run))


def test_unclipped_gp_alone_vs_oracle():
    """The GP prior alone at weight 1.0 with the norm clip OFF, every case, gp_half_factor both ways, under the yardstick at that weight (1e-3 rel / 2e-4
    abs) on every waypoint; and, exactly, half factor on = 0.5 x half factor off.

    The float32 ORACLE does not meet this bound (tests/test_guide_ref_cpu.py::test_fp32_oracle_error_on_the_unclipped_gp_prior_alone: the rounding
    of the un-normalised state times 24 / dt^3 is an absolute error of 1e-2 ... 3e-1 in every element of an increment of 1e3 ... 1e5 whose elements
    cancel; 0 - 27 waypoints per case outside the yardstick), and neither did the kernels while they evaluated the term in float32 from the float32
    un-normalised state: they missed on exactly as many waypoints (Panda H = 96: 27 of 2112, max|diff| 2.31e-1).  guide_gp_apply now evaluates the term
    in float64 from the float32 normalised state.  Measured on an MI355X (no half factor: kernel waypoints outside of B x H, max|diff|; float32 oracle:
    waypoints outside, max|diff|; max|ref|):
      RobotPointMass   H = 64: 0 of 576, 2.66e-4; 2, 1.24e-2; 9.0e3     H = 128: 0 of 1152, 3.05e-3; 1, 9.70e-2; 7.5e4
                       H = 96: 0 of 864, 2.55e-3; 3, 4.14e-2; 3.1e4     H = 48: 0 of 432, 3.32e-4; 0, 5.21e-3; 4.0e3
      RobotPointMass3D H = 64: 0 of 640, 4.66e-4; 3, 1.27e-2; 1.0e4     H = 96: 0 of 960, 2.72e-3; 3, 4.18e-2; 3.0e4     H = 9: 0 of 90, 1.1e-5; 0, 3.3e-5; 8.0e1
      RobotPanda       H = 64: 0 of 1408, 9.71e-4; 9, 6.60e-2; 3.1e4    H = 96: 0 of 2112, 1.04e-2; 27, 2.27e-1; 9.3e4
    What is left is the float32 rounding of the result and, at H = 96 and 48, of dt = 5 / H (exact at H = 64, 128).  profiles/guide_terms.md has the
    half-factor rows."""
    total, lines = 0, []
    for robot_id, H in gr.GPU_CASES:
        c = gr.case(robot_id, H)
        got = {}
        for k, (name, run) in enumerate(gr.runs_of(c["ds"])):
            if not gr.is_unclipped_gp(c["ds"], run):
                continue
            ref = gr.case_reference(robot_id, H, k)
            got[run["gp_half_factor"]] = g = _increment(robot_id, H, run)
            assert np.isfinite(g).all() and not g[:, 0].any() and not g[:, -1].any()
            bad = gr.outside(g, ref, 1.0)
            o32 = gr.oracle_run(c["ds"], c["x"], run, torch.float32, c["n_interp"])
            bad32 = gr.outside(o32, ref, 1.0)
            lines.append(f"GUIDE-TERMS | {robot_id} H={H} | {name} | kernel: {int(bad.sum())} of {bad.size} waypoints outside, max|diff| {np.abs(g - ref).max():.3e} | "
                         f"float32 oracle: {int(bad32.sum())} outside, max|diff| {np.abs(o32 - ref).max():.3e} | max|ref| {np.abs(ref).max():.3e}")
            total += int(bad.sum())
        np.testing.assert_allclose(got[True], 0.5 * got[False], rtol=1e-6, atol=1e-12)
    print("\n".join(lines))
    assert total == 0, f"{total} waypoints of the un-clipped GP increments are outside 1e-3 rel / 2e-4 abs"


# ---------------------------------------------------------------------------------------------------------------- 2. the Panda's dense variant
_CHILD_CODE = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import guide_ref as gr
import test_gpu_guide_terms as M
out = {{}}
for H in M.DENSE_H:
    c = gr.case("RobotPanda", H)
    for k, (name, run) in enumerate(gr.runs_of(c["ds"])):
        out[f"{{H}}/{{k}}"] = M._increment("RobotPanda", H, run)
    out[f"{{H}}/variant"] = np.array(M._variant("RobotPanda", H))
np.savez({out!r}, **out)
"""
DENSE_H = (64, 96)
# mpdx_guide_variant with MPDX_GUIDE_DENSE=1: at H = 96 with 128 interpolated points the dense layout needs more than its 80-KB budget and the
# launcher keeps the table variant whatever the switch says (the case then repeats the table variant in a process of its own)
DENSE_TAKEN = {64: 1, 96: 0}
_CHILD = {}


def _variant(robot_id, H):
    """mpdx_guide_variant for the case's composite guide at its batch: the launcher's own rule (1 = the Panda's dense variant)"""
    from mpd_public_amd import _lib
    c = gr.case(robot_id, H)
    pg = gr.product_run(_gpu_dataset(robot_id, H), gr.runs_of(c["ds"])[0][1], c["n_interp"]).cuda()
    gp = pg.device_params(torch.device("cuda"))
    return int(_lib.load().mpdx_guide_variant(C.byref(gp), c["x"].shape[0], H, c["x"].shape[2]))


def _dense_results(tmp_path_factory):
    """MPDX_GUIDE_DENSE is read once per process: ONE child runs the Panda cases with the dense variant forced on, the parent judges what it saved"""
    if "dense" not in _CHILD:
        out = tmp_path_factory.mktemp("guide_dense") / "increments.npz"
        code = _CHILD_CODE.format(root=str(ROOT), tests=str(ROOT / "tests"), out=str(out))
        r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env={**os.environ, "MPDX_GUIDE_DENSE": "1"}, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(out) as z:
            _CHILD["dense"] = {k: z[k] for k in z.files}
    return _CHILD["dense"]


@pytest.mark.parametrize("H", DENSE_H)
def test_panda_dense_variant_vs_oracle(H, tmp_path_factory):
    """guide_step_panda_kernel<DENSE> (the variant large batches take), forced on at this small batch: the same runs, the same rule - the GP prior alone
    with the clip off included, every waypoint inside 1e-3 rel / 2e-4 abs.  The variant each process took is asked of the launcher's own rule
    (mpdx_guide_variant): dense in the child at H = 64, the table variant in this process; H = 96 see DENSE_TAKEN."""
    c = gr.check_reference_conditions("RobotPanda", H)
    res = _dense_results(tmp_path_factory)
    assert int(res[f"{H}/variant"]) == DENSE_TAKEN[H] and _variant("RobotPanda", H) == 0
    for k, (name, run) in enumerate(gr.runs_of(c["ds"])):
        got = res[f"{H}/{k}"]
        if not gr.is_unclipped_gp(c["ds"], run):
            _judge_run("RobotPanda", H, k, name, run, got, tag=" dense")
            continue
        ref = gr.case_reference("RobotPanda", H, k)
        assert got.shape == ref.shape and np.isfinite(got).all() and not got[:, 0].any() and not got[:, -1].any()
        bad = gr.outside(got, ref, 1.0)
        bad32 = gr.outside(gr.oracle_run(c["ds"], c["x"], run, torch.float32, c["n_interp"]), ref, 1.0)
        print(f"GUIDE-TERMS | RobotPanda H={H} dense | {name} | kernel: {int(bad.sum())} of {bad.size} waypoints outside, max|diff| {np.abs(got - ref).max():.3e} | "
              f"float32 oracle: {int(bad32.sum())} outside | max|ref| {np.abs(ref).max():.3e}")
        assert not bad.any(), f"dense H={H} {name}: {int(bad.sum())} waypoints outside 1e-3 rel / 2e-4 abs"


# ---------------------------------------------------------------------------------------------------------------- 3. apply mode
@pytest.mark.parametrize("robot_id,H", [("RobotPointMass", 64), ("RobotPointMass3D", 9), ("RobotPanda", 64)])
def test_apply_mode_equals_x_plus_increment(robot_id, H):
    """mpdx_guide_step in place == x + increment with the hard conditions written, bit for bit, and max|x_new| flagged for the next range test
    (as tests/test_gpu_chain.py does for the chain kernel).  H = 9, D = 6: H * D is no multiple of 4."""
    from mpd_public_amd import _lib
    c = gr.case(robot_id, H)
    ds = _gpu_dataset(robot_id, H)
    run = gr.runs_of(ds)[0][1]
    pg = gr.product_run(ds, run, c["n_interp"]).cuda()
    xg = c["x"].cuda()
    B, _, D = xg.shape
    inc = pg(xg)
    hs, hg = t(f"terms_hs/{robot_id}", (B, D), "uniform").cuda(), t(f"terms_hg/{robot_id}", (B, D), "uniform").cuda()
    want = xg + inc
    want[:, 0], want[:, -1] = hs, hg
    lib, gp, st = _lib.load(), pg.device_params(xg.device), _lib.current_stream()
    flag_in = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.mpdx_absmax(xg.data_ptr(), flag_in.data_ptr(), B, B, H, D, st))
    assert torch.equal(flag_in.view(torch.float32), xg.abs().reshape(1, -1).max(1)[0])
    flag_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    y = xg.clone()
    _lib.check(lib.mpdx_guide_step(C.byref(gp), y.data_ptr(), None, hs.data_ptr(), hg.data_ptr(), flag_in.data_ptr(), flag_out.data_ptr(), B, B, H, D, st))
    assert float(inc.abs().max()) > 0
    assert torch.equal(y, want)
    assert torch.equal(flag_out.view(torch.float32), want.abs().reshape(1, -1).max(1)[0])


# ---------------------------------------------------------------------------------------------------------------- 4. metrics
@pytest.mark.parametrize("robot_id", list(gr.ROBOTS))
def test_metrics_flags_vs_fp64_reference(robot_id):
    """trajectory_metrics(..., return_mask=True), 256 checked points, on the coverage trajectories: the flags equal slack > 0 of the fp64 reference
    wherever |slack| > 1e-5; at most 1 % of the points lie in that band; both flag values occur; the count column is the mask's sum."""
    n_check = 256
    c = gr.case(robot_id, 64)
    ds = _gpu_dataset(robot_id, 64)
    og, _ = oracle_guide(c["ds"], dtype=torch.float64)
    xu32 = og.normalizer.unnormalize(c["x"].double()).float()          # what the kernel is given
    slack = oracle_hinge_slack(c["ds"], xu32, n_check)
    band = slack.abs() <= gr.DELTA
    print(f"{robot_id}: {int(band.sum())} of {band.numel()} checked points within 1e-5 of a margin; {int((slack > 0).sum())} collide")
    assert float(band.double().mean()) <= 0.01 and bool((slack > gr.DELTA).any()) and bool((slack < -gr.DELTA).any())
    out, mask = ds.task.trajectory_metrics(xu32.cuda(), n_check=n_check, return_mask=True)
    out, mask = out.cpu(), mask.cpu()
    assert mask.shape == slack.shape
    print(f"  flags differing outside the band: {int((mask != (slack > 0))[~band].sum())}; inside: {int((mask != (slack > 0))[band].sum())}")
    assert torch.equal(mask[~band], (slack > 0)[~band])
    assert bool(mask.any()) and not bool(mask.all())
    assert torch.equal(out[:, 0], mask.sum(1).float()) and bool((out[:, 3] == n_check).all())
