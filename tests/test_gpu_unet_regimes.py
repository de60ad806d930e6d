"""The U-Net's convolution kernels against the float64 oracle under checkpoint-like weights (tests/regime_ref.py): every forward kernel family and both
backward forms, at the smallest batches that select them.  tests/test_unet_regimes_cpu.py shows that each case here can fail.

Forward families (csrc/): the fused level programs (B = 3, the default), the per-layer kernels conv_block 128 / 256 and conv_pair with MPDX_FUSED=0 (B = 3
on 16-wide, B = 100 on 32-wide tiles), FusedSeqMid3 of the three-level network, the weight-stationary kernels conv_ws / conv_wsn / conv_wsp (B = 513 against
MPDX_WS=0), the general epilogue of other horizons (masked rows at 48 and 24), the run kernel and the joined programs inside a plan.  Backward forms: the
whole-trajectory programs, and gn_mish_bwd_kernel / EPI_GN_BWD per layer with MPDX_TRAIN_BWD_PROG=0, gn_mish_bwd_gen_kernel with the row mask at H = 48.

Bounds: regime_ref.K / K_G times the float32 oracle's own error against float64, plus a floor at the precision of the format (module docstring there).
Every case prints its figures before it asserts; the measured table is profiles/unet_regimes.md."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import regime_ref as rr
from helpers import synth_sd, t, kernel_path, DIM_MULTS
from test_gpu_train_batches import parse_report

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
T_FWD = 37
_NETS, _REFS, _X = {}, {}, {}


def _sd(D, opt, regime):
    return rr.apply_regime(synth_sd(D, opt), regime)


def _net(D, opt, H, regime):
    key = (D, opt, H, regime)
    if key not in _NETS:
        import mpd_public_amd as m
        net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
        net.load_state_dict(_sd(D, opt, regime), strict=True)
        _NETS[key] = net.cuda().eval()
    return _NETS[key]


def _x(D, H, n=100):
    """the first n trajectories of ONE input tensor per (D, H)"""
    if (D, H) not in _X:
        _X[D, H] = t(f"reg_x_D{D}_H{H}", (513, H, D))
    return _X[D, H][:n].contiguous()


def _ref(D, opt, H, regime, idx):
    """the oracle on the trajectories `idx` (a tuple) of _x(D, H), once per module"""
    key = (D, opt, H, regime, idx)
    if key not in _REFS:
        x = _x(D, H, 513)[list(idx)].contiguous()
        _REFS[key] = rr.forward_ref(_sd(D, opt, regime), x, torch.full((len(idx),), T_FWD, dtype=torch.long))
        if regime == "bigaffine":
            rr.assert_bigaffine_shares(_REFS[key]["shares"])
    return _REFS[key]


def _run(net, x):
    return net(x.cuda(), torch.full((x.shape[0],), T_FWD, dtype=torch.long, device="cuda"), None)


def _each_alone(net, x, y):
    """a trajectory's result is bit-equal to its B = 1 run"""
    for i in range(x.shape[0]):
        assert torch.equal(_run(net, x[i:i + 1]), y[i:i + 1]), i


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("regime", rr.REGIMES)
@pytest.mark.parametrize("family,B,fused", [("fused", 3, True), ("layer16", 3, False), ("layer32", 100, False)])
def test_four_level_forward_vs_fp64(regime, family, B, fused):
    D, opt, H = 14, 1, 64
    net, x = _net(D, opt, H, regime), _x(D, H, B)
    ref = _ref(D, opt, H, regime, tuple(range(B)))
    with kernel_path(fused):
        y = _run(net, x)
        if B == 3:
            _each_alone(net, x, y)
    rr.check_forward(y, ref, f"{family} B={B} D={D} H={H} {regime}")


@pytest.mark.parametrize("regime", rr.REGIMES)
def test_three_level_forward_vs_fp64(regime):
    D, opt, H, B = 4, 0, 64, 3
    net, x = _net(D, opt, H, regime), _x(D, H, B)
    y = _run(net, x)
    _each_alone(net, x, y)
    rr.check_forward(y, _ref(D, opt, H, regime, tuple(range(B))), f"fused3 B={B} D={D} H={H} {regime}")


@pytest.mark.parametrize("regime", ["offset100", "constgroup", "bigaffine"])
def test_weight_stationary_forward_is_bit_equal_and_vs_fp64(regime):
    """B = 513: conv_ws, conv_wsn (modes S1 and UPT) and conv_wsp with a ragged last tile == the per-layer kernels, both ends of the batch against the oracle"""
    D, opt, H, B = 14, 1, 64, 513
    net, x = _net(D, opt, H, regime), _x(D, H, B)
    old = os.environ.get("MPDX_WS")
    try:
        os.environ["MPDX_WS"] = "1"
        y_ws = _run(net, x)
        os.environ["MPDX_WS"] = "0"
        y_pl = _run(net, x)
    finally:
        if old is None:
            os.environ.pop("MPDX_WS", None)
        else:
            os.environ["MPDX_WS"] = old
    assert bool(torch.isfinite(y_ws).all()) and float(y_ws.abs().max()) > 1e-3
    assert torch.equal(y_ws, y_pl)
    idx = (0, 1, 2, 3, 509, 510, 511, 512)
    rr.check_forward(y_ws[list(idx)], _ref(D, opt, H, regime, idx), f"ws B={B} D={D} H={H} {regime}")


@pytest.mark.parametrize("regime", ["offset100", "tinyvar", "constgroup", "bigaffine"])
@pytest.mark.parametrize("H,opt", [(128, 1), (32, 0), (48, 1), (24, 1)])
def test_other_horizons_forward_vs_fp64(regime, H, opt):
    """the general epilogue: GroupNorm regions of other sizes, and (48, 24) containers whose rows behind the horizon are masked out of the statistics.
    Everything the pass wrote - the workspace holds every layer's activations, pad rows included - and the result are finite."""
    D, B = 4, 3
    net, x = _net(D, opt, H, regime), _x(D, H, B)
    net.engine(T_FWD + 1, B)
    net._ws.zero_()
    y = _run(net, x)
    assert bool(torch.isfinite(net._ws).all())
    _each_alone(net, x, y)
    rr.check_forward(y, _ref(D, opt, H, regime, tuple(range(B))), f"gen B={B} D={D} H={H} {regime}")


# ---------------------------------------------------------------------------------------------- a plan: the bit-identities
PLAN_T, PLAN_N0 = 3, 1
_DMS, _CHAINS = {}, {}


def _dm(regime):
    if regime not in _DMS:
        import mpd_public_amd as m
        net = m.TemporalUnet(n_support_points=64, state_dim=4, unet_input_dim=32, dim_mults=DIM_MULTS[1])
        net.load_state_dict(_sd(4, 1, regime), strict=True)
        _DMS[regime] = m.GaussianDiffusionModel(model=net.cuda().eval(), variance_schedule="cosine", n_diffusion_steps=PLAN_T, predict_epsilon=True).cuda().eval()
    return _DMS[regime]


def _plan(regime, B, run=True, join=True):
    dm = _dm(regime)
    dm.model.set_inner_run(run)
    dm.model.set_plan_join(join)
    hc = {0: t("reg_plan_hc0", (4,), "uniform", 0.6).cuda(), 63: t("reg_plan_hc1", (4,), "uniform", 0.6).cuda()}
    noise = t("reg_plan_noise", (PLAN_T + PLAN_N0 + 1, 8, 64, 4))[:, :B].contiguous().cuda()
    x, chain = dm.plan(hc, B, 64, n_diffusion_steps_without_noise=PLAN_N0, noise=noise, noise_std_extra_schedule_fn=lambda tt: 0.5)
    torch.cuda.synchronize()
    assert dm.model.status() == 0
    assert bool(torch.isfinite(chain).all()) and torch.equal(x, chain[-1])
    return chain, dm.model.inner_runs(), dm.model.plan_joined(), (hc, noise)


@pytest.mark.parametrize("regime", ["offset100", "bigaffine", "bigtime"])
@pytest.mark.parametrize("B", [5, 8])
def test_plan_identities_hold(regime, B):
    """T = 3 steps and one without noise, injected noise: the run kernel == seven launches, joined == separate programs, fused plan == step-by-step loop,
    and (B = 5) a chain equals the first five trajectories of the B = 8 one.  (No oracle comparison of whole chains: the clamp to [-1, 1] and four steps
    make it uninformative under these regimes.)"""
    import mpd_public_amd as m
    chain, runs, joined, (hc, noise) = _plan(regime, B)
    if regime == "bigaffine":   # (the first pass of the plan, in float64: the regime reaches the three Mish branches on this very input)
        x_T = noise[0].cpu().clone()
        x_T[:, 0], x_T[:, 63] = hc[0].cpu(), hc[63].cpu()
        rr.assert_bigaffine_shares(rr.forward_ref(_sd(4, 1, regime), x_T, torch.full((B,), PLAN_T - 1, dtype=torch.long))["shares"])
    assert runs > 0 and joined > 0, (runs, joined)
    assert not torch.equal(chain[1], chain[2])
    c_norun, runs0, _, _ = _plan(regime, B, run=False)
    assert runs0 == 0 and torch.equal(chain, c_norun)
    c_nojoin, _, joined0, _ = _plan(regime, B, join=False)
    assert joined0 == 0 and torch.equal(chain, c_nojoin)
    dm = _dm(regime)
    dm.model.set_inner_run(True)
    dm.model.set_plan_join(True)
    steps = dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, n_diffusion_steps_without_noise=PLAN_N0,
                             noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise, fused=False)
    assert torch.equal(chain, steps)
    _CHAINS[regime, B] = chain
    other = _CHAINS.get((regime, 8)) if B == 5 else None
    if B == 5:
        if other is None:
            other = _plan(regime, 8)[0]
        assert torch.equal(chain, other[:, :5])


# ---------------------------------------------------------------------------------------------- training
TRAIN_T = 25
TRAIN_REGIMES = ("plain", "offset100", "tinyvar", "constgroup", "gsign", "bigaffine")
# name -> (D, dim_mults option, H, B, backward programs switched on?)
TRAIN_CASES = {"prog4": (14, 1, 64, 4, True), "prog3": (4, 0, 64, 4, True), "layer4": (14, 1, 64, 4, False), "layer3": (4, 0, 64, 4, False),
               "ragged33": (14, 1, 64, 33, True), "masked48": (4, 1, 48, 5, True)}
_GREFS, _CHILD = {}, {}


def _train_batch(D, H, B):
    x0, noise = t(f"reg_tr_x0_{D}_{H}", (33, H, D), "uniform", 0.8)[:B], t(f"reg_tr_noise_{D}_{H}", (33, H, D))[:B]
    hc = {0: t(f"reg_tr_hc0_{D}", (33, D), "uniform", 0.7)[:B], H - 1: t(f"reg_tr_hc1_{D}", (33, D), "uniform", 0.7)[:B]}
    return x0.contiguous(), (torch.arange(B) * 7) % TRAIN_T, hc, noise.contiguous()


def _grad_ref(D, opt, H, B, regime):
    key = (D, opt, H, B, regime)
    if key not in _GREFS:
        x0, tv, hc, noise = _train_batch(D, H, B)
        _GREFS[key] = rr.grads_ref(_sd(D, opt, regime), x0, tv, hc, noise, TRAIN_T)
        if regime == "bigaffine":
            rr.assert_bigaffine_shares(_GREFS[key]["shares"])
    return _GREFS[key]


def train_pass(D, opt, H, B, regime):
    """(loss, {name: gradient on the CPU}) of one TrainStep.loss_backward with supplied t and noise, hard conditions at 0 and H - 1"""
    import mpd_public_amd as m
    from mpd_public_amd.trainer import TrainStep
    net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(_sd(D, opt, regime), strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=TRAIN_T, predict_epsilon=True, loss_type="l2").cuda()
    x0, tv, hc, noise = _train_batch(D, H, B)
    loss, _ = TrainStep(dm).loss_backward(x0.cuda(), {k: v.cuda() for k, v in hc.items()}, t=tv.cuda(), noise=noise.cuda())
    torch.cuda.synchronize()
    return float(loss), {k: p.grad.detach().cpu().clone() for k, p in dm.model.named_parameters()}


def _check_form(rep, case):
    """which backward form ran, from the pass's own report"""
    D, opt, H, B, prog = TRAIN_CASES[case]
    gn_in_epilogue = sum(g for _, g in rep["tiles"].values())
    if prog and H == 64:
        assert rep["up"] == 1 and rep["down"] == 1, rep     # the whole-trajectory programs (their own statistics, v_rcp / v_rsq)
        assert opt == 1 or not rep["tiles"], rep            # three levels: the programs are the whole pass
    else:
        assert rep["up"] == 0 and rep["down"] == 0, rep     # per layer: gn_mish_bwd_kernel (_gen at other horizons) and EPI_GN_BWD
        assert rep["tiles"] and (gn_in_epilogue > 0) == (H == 64), rep


_CHILD_CODE = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import test_gpu_unet_regimes as M
out = {{}}
for regime in M.TRAIN_REGIMES:
    print("REGIME-PASS", regime, file=sys.stderr, flush=True)
    out[regime] = M.train_pass(*M.TRAIN_CASES[{case!r}][:4], regime)
    sys.stderr.flush()
torch.save(out, {out!r})
"""


def _child_results(case, tmp_path_factory):
    """MPDX_TRAIN_BWD_PROG is read once per process: ONE child per case runs all the regimes with the programs switched off"""
    if case not in _CHILD:
        out = tmp_path_factory.mktemp(f"regimes_{case}") / "grads.pt"
        code = _CHILD_CODE.format(root=str(ROOT), tests=str(ROOT / "tests"), case=case, out=str(out))
        r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env={**os.environ, "MPDX_TRAIN_BWD_PROG": "0", "MPDX_DEBUG_TRAIN": "1"},
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        parts = r.stderr.split("REGIME-PASS ")[1:]
        reports = {p.split(None, 1)[0]: parse_report(p) for p in parts}
        _CHILD[case] = (torch.load(out), reports)
    return _CHILD[case]


@pytest.mark.parametrize("regime", TRAIN_REGIMES)
@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_training_pass_vs_fp64_autograd(case, regime, capfd, monkeypatch, tmp_path_factory):
    """the loss and every gradient against float64 autograd of the oracle, on the backward form the case claims"""
    D, opt, H, B, prog = TRAIN_CASES[case]
    ref = _grad_ref(D, opt, H, B, regime)
    if prog:
        capfd.readouterr()
        monkeypatch.setenv("MPDX_DEBUG_TRAIN", "1")
        try:
            loss, grads = train_pass(D, opt, H, B, regime)
        finally:
            monkeypatch.delenv("MPDX_DEBUG_TRAIN")
        rep = parse_report(capfd.readouterr().err)
    else:
        results, reports = _child_results(case, tmp_path_factory)
        (loss, grads), rep = results[regime], reports[regime]
    print(f"REGIME rep {case} {regime}: {rep}")
    rr.check_grads(loss, grads, ref, f"{case} B={B} D={D} H={H} {regime}")
    _check_form(rep, case)
    if regime == "constgroup":
        zeros = sum(1 for g in ref["g64"].values() if float(g.abs().max()) == 0.0)
        assert zeros >= 50, zeros   # everything in front of a zeroed convolution but the residual path
