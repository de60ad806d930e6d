"""GPU tests of mpdx_gpmp_step (csrc/planner.hpp gpmp_lm_kernel) against the float64 oracle (oracle/gpmp.py; PARITY UNPINNED - the
reference's GPMP2 is un-vendored): the proposal over the shapes of the block-cyclic-reduction tree, held to the NORMWISE BACKWARD ERROR
against the oracle's system (tests/gpmp_ref.py: a wrong block shows there, not in the forward error), and the Levenberg-Marquardt
accept / reject machine driven branch by branch."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import gpmp_ref as R
from oracle import gpmp as ogpmp

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def _dataset(env_id, robot_id):
    import mpd_public_amd as m
    return m.TrajectoryDataset(env_id, robot_id, tensor_args={"device": "cuda", "dtype": torch.float32})


def _planner(ds, H, n_interp, lam=1e-2, **kw):
    from mpd_public_amd.generate_trajectories import GPMP2
    ds.n_support_points = H
    opt = GPMP2(ds, R.DT, sigma_gp=R.SIGMA_GP, sigma_obs=R.SIGMA_OBS, n_interp=n_interp or H, lambda_init=lam, device="cuda", **kw)
    if not n_interp:
        opt.gp.interpolate = 0       # collision factors on the supports (N = H)
    return opt


def _fresh(x0, lam):
    x = x0.cuda().contiguous().clone()
    state = torch.zeros((x.shape[0], 4), device="cuda")
    state[:, 0], state[:, 1] = 3.0e38, lam
    return x, torch.zeros_like(x), state


def _step(opt, x, delta, state, solve=1):
    from mpd_public_amd import _lib
    B, H, D = x.shape
    _lib.check(_lib.load().mpdx_gpmp_step(C.byref(opt.gp), C.byref(opt.opts), x.data_ptr(), delta.data_ptr(), state.data_ptr(), B, H, D, solve,
                                          _lib.current_stream()), "mpdx_gpmp_step")
    torch.cuda.synchronize()


def _snap(*ts):
    return [t.detach().cpu().clone() for t in ts]


def _objective(ds, theta, n_interp):
    robot, coll = R.oracle_terms(ds)
    return float(ogpmp.objective(theta.double(), robot, coll, R.DT, R.SIGMA_GP, R.SIGMA_OBS, n_interp or 0))


def _proposal_problems(ds, theta, delta, F_gpu, n_interp, lam, tag, forward=True, step=1.0):
    """the checks of ONE trajectory's proposal `delta` (CPU, [H, D]) at the float32 point `theta` with damping `lam`; prints the figures,
    returns (figures, list of violated checks).  A trajectory the oracle calls ambiguous is measured, not judged (F and the end rows are)."""
    rec = R.oracle_record(ds, theta, n_interp, lam)
    got = delta.double() / step
    eta = R.backward_error(rec["A"], rec["g"], got[1:-1])
    scale = float(rec["want"].abs().max())
    fwd = float((got - rec["want"]).abs().max()) / scale
    fig = dict(eta_gpu=eta, eta_ref32=rec["eta_ref32"], fwd=fwd, ambiguous=rec["ambiguous"])
    print(f"GPMP_STEP {tag} eta_gpu={eta:.2e} eta_ref32={rec['eta_ref32']:.2e} ratio={eta / rec['eta_ref32']:.1f} fwd={fwd:.2e} "
          f"F_rel={abs(F_gpu - rec['F']) / rec['F']:.1e} ambiguous={int(rec['ambiguous'])}")
    bad = []
    if not (rec["F"] > 0 and abs(F_gpu - rec["F"]) <= 2e-4 * rec["F"]):
        bad.append(f"{tag}: F {F_gpu} vs {rec['F']}")
    if delta[0].any() or delta[-1].any():
        bad.append(f"{tag}: end rows of delta are not zero")
    if not bool(torch.isfinite(delta).all()):
        bad.append(f"{tag}: proposal not finite")
    if rec["ambiguous"]:
        return fig, bad
    if not eta <= min(R.ETA_FACTOR * rec["eta_ref32"], R.ETA_CEIL):
        bad.append(f"{tag}: eta {eta:.3e} > min({R.ETA_FACTOR:g} x {rec['eta_ref32']:.3e}, {R.ETA_CEIL:g})")
    if forward and not (scale > 1e-4 and fwd <= 2e-2):
        bad.append(f"{tag}: forward error {fwd:.3e} of scale {scale:.3e}")
    return fig, bad


# ---------------------------------------------------------------------------------------------------------------- the first proposal over the tree shapes
@pytest.mark.parametrize("env_id,robot_id,H,n_interp,lam", R.STEP_CASES)
def test_first_step_vs_oracle_over_the_tree_shapes(env_id, robot_id, H, n_interp, lam):
    """The first call's proposal at every level-size pattern of the solver (n = H - 2 = 2, 3, 2^k, 2^k - 1, even levels at stride > 1,
    nl == 2), with uneven interpolation segments, N = H with and without interpolation, and linearisation mappings with N < 64:
    F to 2e-4, zero end rows, x bit-unchanged, forward error <= 2e-2 of the step's scale (lambda = 1e-2), and the backward error
    against the oracle's float64 system  eta <= 32 eta(all-fp32 oracle), never above 2e-6  (smallest defect measured: 9.1e-6).
    Per-case figures measured on an MI355X: profiles/gpmp_step_edges.md."""
    ds = _dataset(env_id, robot_id)
    x0 = R.gpmp_case(ds, H)
    opt = _planner(ds, H, n_interp, lam)
    x, delta, state = _fresh(x0, lam)
    _step(opt, x, delta, state)
    xc, dc, sc = _snap(x, delta, state)
    assert torch.equal(xc, x0)                         # the first call accepts the (zero) proposal: the point is unchanged
    assert torch.equal(sc[:, 1], torch.full((R.B_CASE,), lam).float()) and not sc[:, 2].any()
    tag = f"{robot_id} H={H} N={n_interp} lam={lam:g} levels={R.level_sizes(H)} parts={R.linearisation_parts(robot_id, H, n_interp or H)}"
    bad, skipped = [], 0
    for b in range(R.B_CASE):
        fig, pb = _proposal_problems(ds, x0[b], dc[b], float(sc[b, 0]), n_interp, lam, f"{tag} b={b}", forward=lam >= 1e-3)
        bad += pb
        skipped += fig["ambiguous"]
    assert skipped <= 1, f"{skipped} of {R.B_CASE} trajectories ambiguous"
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------- the accept / reject machine
LM_CASES = [R.PM + (24, 128), R.PANDA + (24, 48)]
LAM0 = 1e-2


def _after_first_call(env_id, robot_id, H, n_interp, lam=LAM0, **kw):
    ds = _dataset(env_id, robot_id)
    opt = _planner(ds, H, n_interp, lam, **kw)
    x, delta, state = _fresh(R.gpmp_case(ds, H), lam)
    _step(opt, x, delta, state)
    return ds, opt, x, delta, state


def _check_judged_call(ds, opt, n_interp, before, after, solve=1, tag="", check_proposal=True):
    """One call that judged the candidates x + delta of `before` = (x, delta, state) and left `after`: every trajectory against the
    oracle's objective and gpmp_ref.lm_expect.  Returns the per-trajectory expectations."""
    (x0, d0, s0), (x1, d1, s1) = before, after
    out, bad = [], []
    for b in range(x0.shape[0]):
        cand = x0[b].clone()
        cand[1:-1] += d0[b, 1:-1]                       # float32 sum, as the kernel forms it
        F_cur = _objective(ds, x0[b], n_interp)
        F_cand = _objective(ds, cand, n_interp) if bool(torch.isfinite(cand).all()) else float("nan")
        if F_cand == F_cand:                            # decidable in float32
            assert abs(F_cand - F_cur) > 1e-3 * F_cur, (tag, b, F_cand, F_cur)
        e = R.lm_expect(F_cur, float(s0[b, 1]), float(s0[b, 2]), F_cand, opt.opts, False, solve)
        out.append(e)
        assert torch.equal(x1[b], cand if e["accept"] else x0[b]), (tag, b, "x")
        assert float(s1[b, 1]) == float(np.float32(e["lam"])), (tag, b, "lambda", float(s1[b, 1]), e["lam"])
        assert float(s1[b, 2]) == e["n_acc"], (tag, b, "n_acc", float(s1[b, 2]))
        if F_cand == F_cand:
            assert abs(float(s1[b, 3]) - F_cand) <= 2e-4 * F_cand, (tag, b, "F_cand", float(s1[b, 3]), F_cand)
        else:
            assert bool(torch.isnan(s1[b, 3])), (tag, b)
        assert abs(float(s1[b, 0]) - e["F"]) <= 2e-4 * e["F"], (tag, b, "F", float(s1[b, 0]), e["F"])
        if e["accept"]:
            assert float(s1[b, 3]) == float(s1[b, 0]), (tag, b)
        else:
            assert float(s1[b, 0]) == float(s0[b, 0]), (tag, b, "F of the kept point: same input, same code, same bits")
        assert bool(torch.isfinite(x1[b]).all()) and bool(torch.isfinite(d1[b]).all()), (tag, b)
        if e["proposes"] and not check_proposal:
            assert d1[b, 1:-1].any() and not d1[b, 0].any() and not d1[b, -1].any(), (tag, b)
        elif e["proposes"]:
            _, pb = _proposal_problems(ds, x1[b], d1[b], float(s1[b, 0]), n_interp, abs(e["lam"]), f"{tag} b={b}", step=float(opt.opts.step))
            bad += pb
        else:
            assert not d1[b].any(), (tag, b, "delta is zeroed")
    assert not bad, "\n".join(bad)
    return out


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
def test_lm_accepts_a_descending_candidate(env_id, robot_id, H, n_interp):
    ds, opt, x, delta, state = _after_first_call(env_id, robot_id, H, n_interp)
    before = _snap(x, delta, state)
    assert not before[2][:, 2].any()                   # after call 1: (F, lambda, 0, .)
    _step(opt, x, delta, state)
    exp = _check_judged_call(ds, opt, n_interp, before, _snap(x, delta, state), tag=f"accept {robot_id}")
    assert all(e["accept"] and e["n_acc"] == 1 and abs(e["lam"] - LAM0 * 0.2) < 1e-9 for e in exp), exp   # the full step lowers F on all four


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
def test_lm_rejects_an_ascending_candidate_and_relinearises(env_id, robot_id, H, n_interp):
    ds, opt, x, delta, state = _after_first_call(env_id, robot_id, H, n_interp)
    delta *= -40.0
    before = _snap(x, delta, state)
    _step(opt, x, delta, state)
    exp = _check_judged_call(ds, opt, n_interp, before, _snap(x, delta, state), tag=f"reject {robot_id}")
    assert all(not e["accept"] and e["n_acc"] == 0 and abs(e["lam"] - LAM0 * 10) < 1e-8 and e["proposes"] for e in exp), exp


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
def test_lm_rejects_a_nan_candidate(env_id, robot_id, H, n_interp):
    ds, opt, x, delta, state = _after_first_call(env_id, robot_id, H, n_interp)
    delta[:, H // 2, 1] = float("nan")
    before = _snap(x, delta, state)
    _step(opt, x, delta, state)
    exp = _check_judged_call(ds, opt, n_interp, before, _snap(x, delta, state), tag=f"nan {robot_id}")
    assert all(not e["accept"] and e["lam"] > LAM0 and e["proposes"] for e in exp), exp


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
def test_lm_marks_convergence_at_the_lambda_ceiling_and_then_returns_at_once(env_id, robot_id, H, n_interp):
    ds, opt, x, delta, state = _after_first_call(env_id, robot_id, H, n_interp, lambda_max=LAM0)
    delta *= -40.0
    before = _snap(x, delta, state)
    _step(opt, x, delta, state)
    after = _snap(x, delta, state)
    exp = _check_judged_call(ds, opt, n_interp, before, after, tag=f"ceiling {robot_id}")
    assert all(not e["accept"] and not e["proposes"] for e in exp), exp
    assert torch.equal(after[2][:, 1], -before[2][:, 1]) and not after[1].any() and torch.equal(after[0], before[0])
    delta.copy_(torch.full_like(delta, 7.5))           # garbage: a converged trajectory's call returns before it reads it
    _step(opt, x, delta, state)
    again = _snap(x, delta, state)
    assert torch.equal(again[0], after[0]) and torch.equal(again[2], after[2]) and bool((again[1] == 7.5).all())


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
@pytest.mark.parametrize("scale", [1.0, -40.0])
def test_lm_judge_only_call(env_id, robot_id, H, n_interp, scale):
    ds, opt, x, delta, state = _after_first_call(env_id, robot_id, H, n_interp)
    delta *= scale
    before = _snap(x, delta, state)
    _step(opt, x, delta, state, solve=0)
    exp = _check_judged_call(ds, opt, n_interp, before, _snap(x, delta, state), solve=0, tag=f"judge-only {robot_id}")
    assert all(e["accept"] == (scale > 0) and not e["proposes"] for e in exp), exp


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
def test_fixed_damping_accepts_every_candidate(env_id, robot_id, H, n_interp):
    ds, opt, x, delta, state = _after_first_call(env_id, robot_id, H, n_interp, adaptive=False)
    delta *= -40.0
    before = _snap(x, delta, state)
    _step(opt, x, delta, state)
    after = _snap(x, delta, state)
    # (the accepted point is 40 steps uphill - joint angles of ~100 rad: the state is checked there, the proposal is not held to the oracle)
    exp = _check_judged_call(ds, opt, n_interp, before, after, tag=f"fixed {robot_id}", check_proposal=False)
    assert all(e["accept"] and e["n_acc"] == 1 for e in exp) and torch.equal(after[2][:, 1], before[2][:, 1]), exp


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
def test_step_scale_is_applied_to_the_proposal_only(env_id, robot_id, H, n_interp):
    _, _, x1, d1, s1 = _after_first_call(env_id, robot_id, H, n_interp)
    _, _, xq, dq, sq = _after_first_call(env_id, robot_id, H, n_interp, step=0.25)
    assert d1.abs().max() > 1e-4 and torch.equal(dq, 0.25 * d1) and torch.equal(xq, x1) and torch.equal(sq, s1)


@pytest.mark.parametrize("env_id,robot_id,H,n_interp", LM_CASES)
def test_trajectories_of_a_batch_are_independent(env_id, robot_id, H, n_interp):
    """trajectory 0 accepts, 1 rejects, 2 rejects at the lambda ceiling (converges), 3 has a NaN candidate: each one's outputs are those of
    running it alone, bit for bit."""
    ds, opt, x, delta, state = _after_first_call(env_id, robot_id, H, n_interp)
    delta[1:3] *= -40.0
    delta[3, H // 2, 0] = float("nan")
    state[2, 1] = float(opt.opts.lambda_max)
    before = _snap(x, delta, state)
    _step(opt, x, delta, state)
    after = _snap(x, delta, state)
    exp = _check_judged_call(ds, opt, n_interp, before, after, tag=f"batch {robot_id}")
    assert [e["accept"] for e in exp] == [True, False, False, False] and [e["lam"] < 0 for e in exp] == [False, False, True, False], exp
    for b in range(R.B_CASE):
        xb, db, sb = (t[b:b + 1].cuda().contiguous() for t in before)
        _step(opt, xb, db, sb)
        for got, want, name in zip(_snap(xb, db, sb), after, ("x", "delta", "state")):
            same = (got[0] == want[b]) | (torch.isnan(got[0]) & torch.isnan(want[b]))
            assert bool(same.all()), (b, name)
