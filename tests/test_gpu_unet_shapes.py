"""Every U-Net shape of tests/shapes_ref.py - the networks mpdx_unet_create admits besides the two shipped ones - against the float64 oracle: forward
on the default path and with one launch per layer, the weight-stationary kernels at B = 513, the fused plan with its runs / joined / paired launches
switched on and off, and the training step with the backward programs on and off.  The special kernels are selected by layer shape, not by network,
so these rows reach them in places and dataflows the shipped networks do not (the table in shapes_ref.py says which); tests/test_unet_shapes_cpu.py
shows that the cases can fail.

Bounds: regime_ref.K / K_G as they stand (K e_ref + 2^-23 max|y64| forward; per tensor K_G e_ref + 2^-20 max|g64|).  On these rows e_ref is 0.9 - 1.6e-6
under `plain` and 0.6 - 1.2e-4 under `offset100`, the results are near 1.3 - 2.2: bounds of about 4 - 7e-6 and 2 - 5e-4.  Every case prints its figures
(lines starting SHAPES / REGIME) before it asserts; the measured table is profiles/unet_shapes.md."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import regime_ref as rr
import shapes_ref as S
from helpers import t, kernel_path
from test_gpu_train_batches import parse_report

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NAMES = [c[0] for c in S.CASES]
FWD_REGIMES = ("plain", "offset100")
_NETS, _REFS, _SDS = {}, {}, {}


def _sd(name, regime):
    if (name, regime) not in _SDS:
        _SDS[name, regime] = rr.apply_regime(S.state_dict(name), regime)
    return _SDS[name, regime]


def _new_net(name, regime):
    import mpd_public_amd as m
    _, H, W, mults, D = S.ROWS[name]
    net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=W, dim_mults=mults)
    net.load_state_dict(_sd(name, regime), strict=True)
    return net


def _net(name, regime):
    if (name, regime) not in _NETS:
        _NETS[name, regime] = _new_net(name, regime).cuda().eval()
    return _NETS[name, regime]


def _programs(net):
    from mpd_public_amd import _lib
    lib, got = _lib.load(), []
    while lib.mpdx_unet_fused_program(net._handle(), len(got)) != -2:
        got.append(lib.mpdx_unet_fused_program(net._handle(), len(got)))
    return got


def _ref(name, regime, idx):
    """the oracle on the trajectories `idx` (a tuple) of the row's input, once per module"""
    key = (name, regime, idx)
    if key not in _REFS:
        x = S.x_in(name, 513)[list(idx)].contiguous()
        _REFS[key] = rr.forward_ref(_sd(name, regime), x, S.tvec(len(idx)))
    return _REFS[key]


def _run(net, x):
    return net(x.cuda(), S.tvec(x.shape[0]).cuda(), None)


def _fwd_batch(name):
    """B = 3; B = 5 where the coarsest level has 4 positions: a 16-wide tile then holds four trajectories - one full tile and a ragged one"""
    _, H, W, mults, D = S.ROWS[name]
    return 5 if (H >> (len(mults) - 1)) == 4 else 3


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("fused", [True, False], ids=["default", "perlayer"])
@pytest.mark.parametrize("regime", FWD_REGIMES)
@pytest.mark.parametrize("name", NAMES)
def test_forward_vs_fp64_and_each_trajectory_alone(name, regime, fused):
    B = _fwd_batch(name)
    net, x = _net(name, regime), S.x_in(name, B)
    ref = _ref(name, regime, tuple(range(B)))
    with kernel_path(fused):
        y = _run(net, x)
        for i in range(B):   # a trajectory's result is bit-equal to its B = 1 run
            assert torch.equal(_run(net, x[i:i + 1]), y[i:i + 1]), i
    progs = _programs(net)
    assert progs == S.PROGRAMS[name]
    ratio = rr.check_forward(y, ref, f"{name} {'default' if fused else 'perlayer'} B={B} {regime}")
    print(f"SHAPES fwd | {name} | {'default' if fused else 'per layer'} | {regime} | B={B} | programs {progs if fused else '-'} | e_ref {ref['e_ref']:.2e} | ratio {ratio:.3f}")


# ---------------------------------------------------------------------------------------------- large batch: the weight-stationary kernels
@pytest.mark.parametrize("regime", FWD_REGIMES)
@pytest.mark.parametrize("name", ["four-128", "four-256", "five"])
def test_weight_stationary_forward_is_bit_equal_and_vs_fp64(name, regime):
    """B = 513 (a ragged last tile): MPDX_WS=1 == MPDX_WS=0, both ends of the batch against the oracle.  four-128 puts its 128-channel layers on
    conv_wsn, four-256 nine 256 -> 256 layers on conv_ws."""
    B = 513
    net, x = _net(name, regime), S.x_in(name, B)
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
    ref = _ref(name, regime, idx)
    ratio = rr.check_forward(y_ws[list(idx)], ref, f"{name} ws B={B} {regime}")
    print(f"SHAPES ws | {name} | MPDX_WS=1 == 0 | {regime} | B={B} | - | e_ref {ref['e_ref']:.2e} | ratio {ratio:.3f}")


# ---------------------------------------------------------------------------------------------- a plan: the bit-identities
PLAN_T, PLAN_N0 = 3, 1
PLAN_PASSES = PLAN_T + PLAN_N0
PLAN_ROWS = ("four-128", "four-256", "five", "rep-last")
# what the admission rules of mpdx_plan's schedule give (csrc/mpdx.hip PlanSchedule, inner_run_first, tail_run_first), per fused plan of PLAN_PASSES passes:
# (seven-layer run launches, layers inside run launches of either kind, joined launches, of them paired)
#   four-256  four levels on H = 64 and seven consecutive 256 -> 256 layers on 8 positions from downs.3.0.blocks.0 on: the run, every pass; programs 0 + 2: no join
#   four-128  programs 5 + 3: every pass but the last is joined, and paired (B <= 128, D <= 16); ups.0's three 128 -> 128 layers + Upsample1d: the tail run
#   five      programs 5 + 3: joined and paired although n_levels == 5; the runs are for four levels only
#   rep-last  programs 0, -1, 2: neither
PLAN_WANT = {"four-256": (PLAN_PASSES, 7 * PLAN_PASSES, 0, 0), "four-128": (0, 4 * PLAN_PASSES, PLAN_PASSES - 1, PLAN_PASSES - 1),
             "five": (0, 0, PLAN_PASSES - 1, PLAN_PASSES - 1), "rep-last": (0, 0, 0, 0)}
_DMS, _CHAINS = {}, {}


def _dm(name):
    if name not in _DMS:
        import mpd_public_amd as m
        _DMS[name] = m.GaussianDiffusionModel(model=_new_net(name, "plain").cuda().eval(), variance_schedule="cosine", n_diffusion_steps=PLAN_T,
                                              predict_epsilon=True).cuda().eval()
    return _DMS[name]


def _plan_inputs(name, B):
    _, H, W, mults, D = S.ROWS[name]
    hc = {0: t("shapes_plan_hc0", (D,), "uniform", 0.6), H - 1: t("shapes_plan_hc1", (D,), "uniform", 0.6)}
    noise = t(f"shapes_plan_noise_{name}", (PLAN_PASSES + 1, 8, H, D))[:, :B].contiguous()
    return hc, noise


def _plan(name, B, run=True, join=True, split=None):
    """-> (chain, (seven-layer runs, run layers, joined, paired)) of one fused plan; the handle's status is 0 afterwards"""
    dm, (hc, noise) = _dm(name), _plan_inputs(name, B)
    H = S.ROWS[name][1]
    dm.model.set_inner_run(run)
    dm.model.set_plan_join(join)
    dm.model.set_level_split(split)
    x, chain = dm.plan({k: v.cuda() for k, v in hc.items()}, B, H, n_diffusion_steps_without_noise=PLAN_N0, noise=noise.cuda(),
                       noise_std_extra_schedule_fn=lambda tt: 0.5)
    torch.cuda.synchronize()
    assert dm.model.status() == 0
    assert bool(torch.isfinite(chain).all()) and torch.equal(x, chain[-1])
    return chain, (dm.model.inner_runs(), dm.model.inner_run_layers(), dm.model.plan_joined(), dm.model.plan_split())


def _first_step_ref(name, B):
    """the plan's first pass (U-Net at t = T - 1 on the conditioned noise, the DDPM update, the hard conditions) by the oracle in float64 and float32"""
    from oracle import diffusion as odiff, schedules as osched
    hc, noise = _plan_inputs(name, B)
    out = {}
    for key, dt in (("y64", torch.float64), ("y32", torch.float32)):
        buf = {k: v.to(dt) for k, v in osched.make_buffers(PLAN_T, "cosine").items()}
        hcb = {k: v[None, :].expand(B, -1).to(dt).clone() for k, v in hc.items()}
        sd = {k: v.to(dt) for k, v in _sd(name, "plain").items()}
        with rr.one_thread():
            x = odiff.apply_hard_conditioning(noise[0].to(dt).clone(), hcb)
            x = odiff.ddpm_step(buf, sd, x, hcb, PLAN_T - 1, noise[1].to(dt), noise_std=0.5)
            out[key] = odiff.apply_hard_conditioning(x, hcb)
    return out


@pytest.mark.parametrize("B", [5, 8])
@pytest.mark.parametrize("name", PLAN_ROWS)
def test_plan_identities_hold(name, B):
    """T = 3 steps and one without noise, injected noise: runs on == off, joined == separate programs, paired == unpaired, fused plan == step-by-step
    loop, and (B = 5) the chain equals the first five trajectories of the B = 8 one; the first pass against the oracle."""
    import mpd_public_amd as m
    chain, counts = _plan(name, B)
    progs = _programs(_dm(name).model)
    print(f"SHAPES plan | {name} | B={B} | programs {progs} | inner_runs {counts[0]} inner_run_layers {counts[1]} plan_joined {counts[2]} plan_split {counts[3]}")
    assert progs == S.PROGRAMS[name]
    assert not torch.equal(chain[1], chain[2])
    ref = _first_step_ref(name, B)
    ratio = rr.check_forward(chain[1], ref, f"{name} plan first pass B={B}")
    print(f"SHAPES plan1 | {name} | first pass of the plan | plain | B={B} | programs {progs} | e_ref {float((ref['y32'].double() - ref['y64']).abs().max()):.2e} | ratio {ratio:.3f}")
    c_norun, n_norun = _plan(name, B, run=False)
    assert n_norun[:2] == (0, 0) and torch.equal(chain, c_norun)
    c_nojoin, n_nojoin = _plan(name, B, join=False)
    assert n_nojoin[2:] == (0, 0) and torch.equal(chain, c_nojoin)
    c_split, n_split = _plan(name, B, split=True)
    c_nosplit, n_nosplit = _plan(name, B, split=False)
    assert n_nosplit[3] == 0 and n_nosplit[2] == n_split[2] and torch.equal(c_split, c_nosplit) and torch.equal(chain, c_split)
    print(f"SHAPES plan | {name} | B={B} | level split forced on: plan_split {n_split[3]} of plan_joined {n_split[2]}")
    dm = _dm(name)
    dm.model.set_inner_run(True)
    dm.model.set_plan_join(True)
    dm.model.set_level_split(None)
    hc, noise = _plan_inputs(name, B)
    steps = dm.run_inference(None, {k: v.cuda() for k, v in hc.items()}, n_samples=B, horizon=S.ROWS[name][1], return_chain=True, sample_fn=m.ddpm_sample_fn,
                             n_diffusion_steps_without_noise=PLAN_N0, noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise.cuda(), fused=False)
    assert torch.equal(chain, steps)
    _CHAINS[name, B] = chain
    if B == 5:
        other = _CHAINS.get((name, 8))
        if other is None:
            other = _plan(name, 8)[0]
        assert torch.equal(chain, other[:, :5])
    assert counts == PLAN_WANT[name], (name, counts)
    assert n_split[3] == PLAN_WANT[name][3]


# ---------------------------------------------------------------------------------------------- training
TRAIN_T, TRAIN_B = 25, 4
TRAIN_ROWS = ("two", "rep-first", "rep-last", "four-256", "five")
TRAIN_REGIMES = ("plain", "offset100", "constgroup")
_GREFS, _CHILD = {}, {}


def _train_batch(name):
    _, H, W, mults, D = S.ROWS[name]
    B = TRAIN_B
    x0, noise = t(f"shapes_tr_x0_{name}", (B, H, D), "uniform", 0.8), t(f"shapes_tr_noise_{name}", (B, H, D))
    hc = {0: t(f"shapes_tr_hc0_{name}", (B, D), "uniform", 0.7), H - 1: t(f"shapes_tr_hc1_{name}", (B, D), "uniform", 0.7)}
    return x0, (torch.arange(B) * 7) % TRAIN_T, hc, noise


def _grad_ref(name, regime):
    if (name, regime) not in _GREFS:
        x0, tv, hc, noise = _train_batch(name)
        _GREFS[name, regime] = rr.grads_ref(_sd(name, regime), x0, tv, hc, noise, TRAIN_T)
    return _GREFS[name, regime]


def train_pass(name, regime):
    """(loss, {name: gradient on the CPU}) of one TrainStep.loss_backward with supplied t and noise, hard conditions at 0 and H - 1"""
    import mpd_public_amd as m
    from mpd_public_amd.trainer import TrainStep
    dm = m.GaussianDiffusionModel(model=_new_net(name, regime), n_diffusion_steps=TRAIN_T, predict_epsilon=True, loss_type="l2").cuda()
    x0, tv, hc, noise = _train_batch(name)
    loss, _ = TrainStep(dm).loss_backward(x0.cuda(), {k: v.cuda() for k, v in hc.items()}, t=tv.cuda(), noise=noise.cuda())
    torch.cuda.synchronize()
    return float(loss), {k: p.grad.detach().cpu().clone() for k, p in dm.model.named_parameters()}


_CHILD_CODE = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import test_gpu_unet_shapes as M
out = {{}}
for regime in M.TRAIN_REGIMES:
    print("REGIME-PASS", regime, file=sys.stderr, flush=True)
    out[regime] = M.train_pass({name!r}, regime)
    sys.stderr.flush()
torch.save(out, {out!r})
"""


def _child_results(name, tmp_path_factory):
    """MPDX_TRAIN_BWD_PROG is read once per process: ONE child per row runs the regimes with the programs switched off"""
    if name not in _CHILD:
        out = tmp_path_factory.mktemp(f"shapes_{name}") / "grads.pt"
        code = _CHILD_CODE.format(root=str(ROOT), tests=str(ROOT / "tests"), name=name, out=str(out))
        r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env={**os.environ, "MPDX_TRAIN_BWD_PROG": "0", "MPDX_DEBUG_TRAIN": "1"},
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        parts = r.stderr.split("REGIME-PASS ")[1:]
        _CHILD[name] = (torch.load(out), {p.split(None, 1)[0]: parse_report(p) for p in parts})
    return _CHILD[name]


@pytest.mark.parametrize("prog", [True, False], ids=["programs", "perlayer"])
@pytest.mark.parametrize("regime", TRAIN_REGIMES)
@pytest.mark.parametrize("name", TRAIN_ROWS)
def test_training_pass_vs_fp64_autograd(name, regime, prog, capfd, monkeypatch, tmp_path_factory):
    """the loss and every gradient against float64 autograd of the oracle, B = 4 with four different timesteps.  `five` ends like the standard
    network (Upsample1d(128) onto 16 positions, two up levels, final_conv), so the whole-trajectory backward program of the up levels runs in it, behind
    five levels instead of four; the other rows run one launch per layer.  Its time table row is 2944 floats: time_bwd_all_kernel stages rows of up to
    4608 (it took 2560 and the training step refused this network)."""
    ref = _grad_ref(name, regime)
    if prog:
        capfd.readouterr()
        monkeypatch.setenv("MPDX_DEBUG_TRAIN", "1")
        try:
            loss, grads = train_pass(name, regime)
        finally:
            monkeypatch.delenv("MPDX_DEBUG_TRAIN")
        rep = parse_report(capfd.readouterr().err)
    else:
        results, reports = _child_results(name, tmp_path_factory)
        (loss, grads), rep = results[regime], reports[regime]
    worst, lratio = rr.check_grads(loss, grads, ref, f"{name} {'programs' if prog else 'perlayer'} B={TRAIN_B} {regime}")
    print(f"SHAPES train | {name} | {'programs on' if prog else 'MPDX_TRAIN_BWD_PROG=0'} | {regime} | B={TRAIN_B} | up {rep['up']} down {rep['down']} | "
          f"worst gradient ratio {worst:.3f} | loss ratio {lratio:.3f}")
    if prog and name == "five":   # (the down program is applicable too, but declines at run time - it ran in none of the measured passes; not asserted)
        assert rep["up"] == 1, rep
    else:
        assert (rep["up"], rep["down"]) == (0, 0), rep
