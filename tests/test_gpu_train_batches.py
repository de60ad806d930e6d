"""The training step above batch 128: the large input-gradient tiles, the saturated weight-gradient splits and the per-layer path behind the backward
programs' batch limit.  mpdx_train_loss_backward (csrc/train_host.hpp, train.hpp, fused_bwd.hpp) picks its kernels and work splits from the batch size;
the other training tests stop at 128, bench.py measures 512.  What changes above 128 (read from the MPDX_DEBUG_TRAIN report of every case, asserted):

  * choose_tile (csrc/mpdx.hip) gives an input-gradient convolution the largest tile that still yields 160 workgroups and fits 96 KiB of LDS: the MT x NT mix
    of the four-level network's inner layers changes at batch 73, 77, 153, 157 and 313 (TILES below); from 313 on a 32 x 64 tile holds the GroupNorm regions
    of four trajectories (EPI_GN_BWD, 128 channels on 16 positions) and the paired second 1x1 convolution; with NT = 64 the last tile is partial when the
    batch is no multiple of 8 (L = 8) / 4 (L = 16): 129, 155, 203, 313, 513;
  * the weight gradients behind the chain use the split divisor 8 up to 128 and 4 beyond (129), the split count grows with sqrt(B / 128) up to 2 (512);
  * up to batch 512 (MPDX_TRAIN_BWD_PROG_MAX_B) the outer levels run as the two whole-trajectory programs, from 513 on per layer on the large tiles.
    On the three-level network (dim_mults option 0) the two programs cover ALL 34 layers: up to 512 it launches no input-gradient convolution of its own
    (the report's tile line reads `none`), so its large tiles are met at 513 only - the case (513, 4, 0) was added to the issue's list for that;
  * MPDX_TRAIN_DEFERRED=0 (the fallback train_ws takes by itself when the partial sums pass 96 M floats): no programs, no pairing, no late launch.

Reference: float64 autograd of the oracle (oracle/train.py).  Bounds, the project's own: |loss - ref| < 5e-6 max(1, |ref|); per tensor
max|g - g_ref| <= 2e-4 max|g_ref| (l1: 2e-3, sign(e) flips where |e| ~ 1e-7).  The fp32 oracle alone stays 2.3e-6 (batch 128) ... 5.0e-6 (577) from the fp64 one
over all tensors, so 2e-4 is 40 x what fp32 rounding needs at these batches.

Measured worst relative gradient error per case (B, D, dim_mults option; MI355X) - 30 ... 170 x below the bound:
  (129, 4, 1) 3.5e-6   (155, 4, 1) 6.6e-6   (160, 14, 0) 1.6e-6   (160, 4, 1) 3.1e-6   (203, 7, 0) 1.3e-6   (203, 4, 1) l1 2.4e-6   (313, 4, 1) 2.4e-6
  (512, 14, 0) 1.2e-6   (512, 4, 1) 2.4e-6   (513, 14, 1) 1.8e-6   (513, 4, 0) 1.1e-6   (160, 4, 1) with MPDX_TRAIN_DEFERRED=0 3.2e-6

Where the hand derivation of the thresholds (batch 160 for the first 32x64 tile, none at 128) met the code, the code's boundaries are the ones tested: the
512-channel input gradient of ups[0] takes 32x64 from batch 73 on (so the tests at 96 / 128 ran one already), the 128-channel layers of 16 positions move to
NT = 64 at 153 (16x64) / 157 (the first 32x64 of a 128-channel layer) / 313 (all of them, the first with the GroupNorm backward in the epilogue), and the
256-channel layers of 8 positions never leave 32x32 (a 64-position tile of theirs needs 97.5 KiB of staging, choose_tile's budget is 96).  Cases 155 and 313
were added for the two regimes the issue's list left without an oracle case; 128 | 152 | 153 | 156 | 157 | 312 | 512 check each boundary's other side without one.
"""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import synth_sd, t, DIM_MULTS

pytestmark = pytest.mark.gpu

H, T = 64, 25
ROOT = Path(__file__).resolve().parent.parent


def _model(D, opt, T=T, loss_type="l2", predict_epsilon=True):
    import mpd_public_amd as m
    net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    return m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=predict_epsilon, loss_type=loss_type).cuda()


def _batch(B, D):
    """x0, noise, hard conditions at 0 and 63, t = (arange(B) * 7) % T - on the CPU"""
    x0, noise = t(f"bat_x0_{B}", (B, H, D), "uniform", 0.8), t(f"bat_noise_{B}", (B, H, D))
    hc = {0: t(f"bat_hc0_{B}", (B, D), "uniform", 0.7), H - 1: t(f"bat_hc1_{B}", (B, D), "uniform", 0.7)}
    return x0, noise, hc, (torch.arange(B) * 7) % T


def _cuda(hc):
    return {k: v.cuda() for k, v in hc.items()}


# ------------------------------------------------------------------------------------------------ the debug report of a pass
_PROG = re.compile(r"backward programs: up (\d) \(layers \[(-?\d+), (\d+)\)\), down (\d) \(variant (\d), layers \[0, (\d+)\]\)")
_JOBS = re.compile(r"backward: (\d+) weight-gradient jobs behind the chain")
_TILES = re.compile(r"backward: input-gradient tiles:(.*)")


def parse_report(text):
    """the LAST pass's report in `text` (stderr under MPDX_DEBUG_TRAIN) -> dict(up, down, jobs, tiles={'32x64': (convolutions, of them with the GroupNorm backward in the epilogue), ...})"""
    prog, jobs, tiles = _PROG.findall(text), _JOBS.findall(text), _TILES.findall(text)
    assert prog and jobs and tiles, text[-2000:]
    tl = {a: (int(b), int(c)) for a, b, c in re.findall(r"(\d+x\d+) x(\d+) \(gn (\d+)\)", tiles[-1])}
    assert tl or tiles[-1].strip() == "none", tiles[-1]
    return {"up": int(prog[-1][0]), "down": int(prog[-1][3]), "jobs": int(jobs[-1]), "tiles": tl}


def traced(capfd, monkeypatch, fn):
    """fn() with the pass's report switched on (a LIVE switch: read on every pass) -> (fn's result, the parsed report)"""
    capfd.readouterr()
    monkeypatch.setenv("MPDX_DEBUG_TRAIN", "1")
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv("MPDX_DEBUG_TRAIN")
    err = capfd.readouterr().err
    rep = parse_report(err)
    print(rep)
    return out, rep


# The tiles of the input-gradient convolutions a default pass launches itself, by batch (MI355X, 160-workgroup rule; `tile: (convolutions, of them with the
# GroupNorm backward in the epilogue)`).  Four levels: layers 18 ... 32 (the 256-channel level, the middle blocks, ups[0]) up to batch 512, all 45 from 513 on.
# Three levels: the two programs cover all 34 layers up to 512 - no launch of its own - and all 33 input-gradient convolutions run per layer from 513 on.
TILES = {   # (first batch, last batch the mix was seen at, mix)
    1: [(40, 49, {"32x16": (8, 7), "16x64": (1, 0), "16x32": (1, 0), "16x16": (5, 3)}),
        (77, 152, {"32x64": (1, 0), "32x32": (8, 7), "16x64": (1, 0), "16x32": (5, 3)}),
        (153, 156, {"32x64": (1, 0), "32x32": (8, 7), "16x64": (5, 3), "16x32": (1, 0)}),
        (157, 312, {"32x64": (2, 0), "32x32": (9, 7), "16x64": (4, 3)}),
        (313, 512, {"32x64": (6, 3), "32x32": (9, 7)}),      # the first GroupNorm backward on a 32x64 tile: four trajectories of 16 positions per tile
        (513, 530, {"32x64": (35, 21), "32x32": (9, 7)})],   # ... and one trajectory (L = 64) / two (L = 32) per tile on the outer levels
    0: [(48, 512, {}), (513, 530, {"32x64": (32, 21)})],
}
TILES_NOT_DEFERRED_160 = {"32x64": (22, 0), "32x32": (8, 0), "16x64": (14, 0)}   # four levels: 44 input-gradient convolutions, each its own launch


def expected_tiles(B, opt):
    (mix,) = [m for first, last, m in TILES[opt] if first <= B <= last]
    return mix


def check_path(rep, B, opt, deferred=True):
    """the path a pass takes at batch B (module docstring): fails when a rule's threshold moves, so that no case silently runs another path"""
    if not deferred:   # no program, nothing paired or late: every input-gradient convolution its own launch, none with the GroupNorm epilogue
        assert rep["up"] == 0 and rep["down"] == 0 and rep["jobs"] == 0, rep
        assert (B, opt) == (160, 1) and rep["tiles"] == TILES_NOT_DEFERRED_160, rep
        return
    progs = 1 if B <= 512 else 0   # MPDX_TRAIN_BWD_PROG_MAX_B
    assert rep["up"] == progs and rep["down"] == progs, rep
    assert rep["jobs"] > 0, rep   # the late launch (from batch 48 on)
    assert rep["tiles"] == expected_tiles(B, opt), (rep, expected_tiles(B, opt))


def check_grads(dm, loss, ref_loss, ref):
    assert abs(float(loss) - float(ref_loss)) < 5e-6 * max(1.0, abs(float(ref_loss))), (float(loss), float(ref_loss))
    worst, at = 0.0, None
    for name, p in dm.model.named_parameters():
        g, r = p.grad.detach().cpu().double(), ref[name]
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), name
        err, scale = float((g - r).abs().max()), max(float(r.abs().max()), 1e-7)
        if err / scale > worst:
            worst, at = err / scale, name
    return worst, at


# (B, D, dim_mults option, loss type, predict_epsilon, clipped Adam step behind it)
ORACLE_CASES = [
    (129, 4, 1, "l2", True, False),    # first batch past the 8 -> 4 divisor switch, odd
    (155, 4, 1, "l2", True, False),    # the four-batch window 153 ... 156 of the 16x64 tiles, odd
    (160, 14, 0, "l2", True, False),   # the issue's first batch of the large tiles (in fact: from 157 on) ... the three-level network: in the programs
    (160, 4, 1, "l2", True, False),    # ... the four-level one: per layer on the inner levels
    (203, 7, 0, "l2", True, False),    # odd, no multiple of 8: ragged trajectory chunks in the programs
    (203, 4, 1, "l1", False, False),   # 32x64 with a ragged last tile (L = 8 and L = 16), l1 / predict x0
    (313, 4, 1, "l2", True, False),    # first batch with every inner 128-channel convolution on 32x64, odd
    (512, 14, 0, "l2", True, True),    # the bench's batch; last batch with the backward programs; split factor saturated
    (512, 4, 1, "l2", True, False),
    (513, 14, 1, "l2", True, False),   # first batch without the programs; odd; the time MLP's 32-sample chunks end with a chunk of one
    (513, 4, 0, "l2", True, False),    # ... and the three-level network's only per-layer pass on the large tiles
]


@pytest.mark.parametrize("B,D,opt,loss_type,pred_eps,adam", ORACLE_CASES)
def test_loss_backward_above_batch_128_vs_oracle(capfd, monkeypatch, B, D, opt, loss_type, pred_eps, adam):
    """Loss and every gradient against float64 autograd of the oracle on both sides of each batch rule, each case on the path it claims (check_path);
    after the (512, 14, 0) pass one clipped Adam step against the oracle's clip_grad_norm + adam_step on the HIP gradients (an entry of the flat gradient
    left unwritten at a split count the small batches never produce would move its weight)."""
    from mpd_public_amd.trainer import TrainStep
    from oracle import train as otrain
    dm = _model(D, opt, loss_type=loss_type, predict_epsilon=pred_eps)
    x0, noise, hc, tt = _batch(B, D)
    ts = TrainStep(dm)
    (loss, _), rep = traced(capfd, monkeypatch, lambda: ts.loss_backward(x0.cuda(), _cuda(hc), t=tt.cuda(), noise=noise.cuda()))
    check_path(rep, B, opt)
    ref_loss, ref = otrain.loss_and_grads(synth_sd(D, opt), x0, tt, hc, noise, T, predict_epsilon=pred_eps, loss_type=loss_type, dtype=torch.float64)
    tol = 2e-4 if loss_type == "l2" else 2e-3   # l1: sign(e) flips where |e| ~ 1e-7
    worst, at = check_grads(dm, loss, ref_loss, ref)
    print(f"batch {B} x D = {D}, dim_mults option {opt}, {loss_type}: worst relative gradient error {worst:.2e} ({at})")
    assert worst <= tol, (at, worst)
    if adam:
        sd0 = synth_sd(D, opt)
        g_hip = {k: p.grad.detach().cpu().clone() for k, p in dm.model.named_parameters()}
        _, clipped = otrain.clip_grad_norm(g_hip, 1.0)
        want = otrain.adam_step({k: sd0[k].clone() for k in clipped}, clipped, {}, 1e-4)
        ts.adam_step(1e-4, max_norm=1.0)
        # (Adam's first step moves a weight by lr * g / (|g| + eps): where |g| is within rounding of eps = 1e-8 the quotient is not decided by fp32 arithmetic -
        #  such an entry may differ by up to one full step; bounds of test_training_at_other_horizons_vs_oracle)
        for name, p in dm.model.named_parameters():
            d = (p.detach().cpu() - want[name]).abs()
            assert float(d.max()) < 1.01e-4 and int((d > 5e-6).sum()) <= max(2, int(1e-3 * d.numel())), (name, float(d.max()), int((d > 5e-6).sum()))


@pytest.mark.parametrize("B,opt", [(128, 1), (152, 1), (153, 1), (156, 1), (157, 1), (312, 1), (512, 1), (128, 0), (512, 0)])
def test_the_tile_and_program_rules_switch_where_the_cases_assume(capfd, monkeypatch, B, opt):
    """The thresholds the oracle cases sit on from their other side, without an oracle: the tile mixes change at 153, 157, 313 and (with the programs) 513."""
    from mpd_public_amd.trainer import TrainStep
    dm = _model(4, opt)
    x0, noise, hc, tt = _batch(B, 4)
    _, rep = traced(capfd, monkeypatch, lambda: TrainStep(dm).loss_backward(x0.cuda(), _cuda(hc), t=tt.cuda(), noise=noise.cuda()))
    check_path(rep, B, opt)
    assert B == 128 or any(B in (first, last) for first, last, _ in TILES[opt]), "a batch chosen for its boundary"


def test_two_fresh_steps_at_batch_513_are_bit_equal():
    """No float atomics on the per-layer large-tile path either: two fresh TrainSteps give the same loss and flat gradient, bit for bit."""
    from mpd_public_amd.trainer import TrainStep
    B, D, opt = 513, 4, 1
    x0, noise, hc, tt = _batch(B, D)
    out = []
    for _ in range(2):
        ts = TrainStep(_model(D, opt))
        loss, _ = ts.loss_backward(x0.cuda(), _cuda(hc), t=tt.cuda(), noise=noise.cuda())
        out.append((float(loss), ts.fp.grad.detach().cpu().clone()))
    assert out[0][0] == out[1][0] and np.isfinite(out[0][0])
    assert torch.equal(out[0][1], out[1][1])


def test_one_train_step_grows_and_shrinks_through_the_batch_rules(capfd, monkeypatch):
    """Batches 40 -> 513 -> 40 -> 160 through ONE TrainStep: the workspace is re-allocated upward and its layout re-derived per pass, the backward programs
    go on, off and on again - every pass's loss and flat gradient equal those of a fresh TrainStep at that batch, bit for bit."""
    from mpd_public_amd.trainer import TrainStep
    D, opt = 4, 1
    x0, noise, hc, tt = _batch(513, D)

    def run(ts, B):
        return traced(capfd, monkeypatch, lambda: ts.loss_backward(x0[:B].cuda(), {k: v[:B].cuda() for k, v in hc.items()}, t=tt[:B].cuda(), noise=noise[:B].cuda()))
    fresh = {}
    for B in (40, 513, 160):
        ts = TrainStep(_model(D, opt))
        (loss, _), rep = run(ts, B)
        check_path(rep, B, opt)
        fresh[B] = (float(loss), ts.fp.grad.detach().cpu().clone())
    assert not torch.equal(fresh[40][1], fresh[160][1])
    ts = TrainStep(_model(D, opt))
    sizes = []
    for B in (40, 513, 40, 160):
        (loss, _), rep = run(ts, B)
        check_path(rep, B, opt)
        sizes.append(ts._ws.numel())
        assert float(loss) == fresh[B][0], B
        assert torch.equal(ts.fp.grad.detach().cpu(), fresh[B][1]), B
    assert sizes[1] > sizes[0] and sizes[1] == sizes[2] == sizes[3]


@pytest.mark.parametrize("first,then", [(64, 48), (513, 512)])
def test_a_smaller_batch_that_needs_the_larger_workspace_gets_it(first, then):
    """The workspace does not grow with the batch everywhere: the weight gradients' partial sums make batch 48 need twice the floats of batch 64 (below 64 the
    programs' layers may take four times the splits), 512 more than 513.  TrainStep used to keep the buffer of the LARGEST BATCH seen - a last, smaller
    batch of an epoch then ran past its end.  The buffer holds what the pass asks for, and the pass equals a fresh TrainStep's bit for bit."""
    from mpd_public_amd import _lib
    from mpd_public_amd.trainer import TrainStep
    D, opt = 4, 1
    x0, noise, hc, tt = _batch(first, D)

    def run(ts, B):
        loss, _ = ts.loss_backward(x0[:B].cuda(), {k: v[:B].cuda() for k, v in hc.items()}, t=tt[:B].cuda(), noise=noise[:B].cuda())
        return float(loss), ts.fp.grad.detach().cpu().clone()
    dm = _model(D, opt)
    lib, h = _lib.load(), dm.model._handle()
    need = {B: int(lib.mpdx_train_workspace_floats(h, B)) for B in (first, then)}
    assert need[then] > need[first], need   # what makes this pair a test
    ts = TrainStep(dm)
    run(ts, first)
    assert ts._ws.numel() >= need[first]
    got = run(ts, then)
    assert ts._ws.numel() >= need[then], (ts._ws.numel(), need)
    want = run(TrainStep(_model(D, opt)), then)
    assert got[0] == want[0] and torch.equal(got[1], want[1])


def test_non_deferred_fallback_at_batch_160_vs_oracle(tmp_path):
    """MPDX_TRAIN_DEFERRED=0 (read once per process: a subprocess) is the path train_ws takes by itself once a network's partial sums pass 96 M floats: every
    weight gradient reduced per layer, no backward program, no paired launch, nothing behind the chain - loss and every gradient against the fp64 oracle at
    the bounds above, on the large tiles of the un-paired input-gradient launches."""
    from oracle import train as otrain
    B, D, opt = 160, 4, 1
    out = tmp_path / "grads.pt"
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import torch, test_gpu_train_batches as M\n"
        "from mpd_public_amd.trainer import TrainStep\n"
        f"dm = M._model({D}, {opt}); x0, noise, hc, tt = M._batch({B}, {D}); ts = TrainStep(dm)\n"
        "loss, _ = ts.loss_backward(x0.cuda(), M._cuda(hc), t=tt.cuda(), noise=noise.cuda()); torch.cuda.synchronize()\n"
        "torch.save({'loss': float(loss), 'grads': {k: p.grad.detach().cpu() for k, p in dm.model.named_parameters()}}, %r)\n"
    ) % (str(ROOT), str(ROOT / "tests"), str(out))
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env={**os.environ, "MPDX_TRAIN_DEFERRED": "0", "MPDX_DEBUG_TRAIN": "1"},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = parse_report(r.stderr)
    print(rep)
    check_path(rep, B, opt, deferred=False)
    got = torch.load(out)
    x0, noise, hc, tt = _batch(B, D)
    ref_loss, ref = otrain.loss_and_grads(synth_sd(D, opt), x0, tt, hc, noise, T, predict_epsilon=True, loss_type="l2", dtype=torch.float64)
    assert abs(got["loss"] - float(ref_loss)) < 5e-6 * max(1.0, abs(float(ref_loss)))
    worst = 0.0
    for name, r64 in ref.items():
        g = got["grads"][name].double()
        assert g.shape == r64.shape and bool(torch.isfinite(g).all()), name
        err, scale = float((g - r64).abs().max()), max(float(r64.abs().max()), 1e-7)
        worst = max(worst, err / scale)
        assert err <= 2e-4 * scale, (name, err, scale)
    print(f"batch {B} x D = {D}, dim_mults option {opt}, MPDX_TRAIN_DEFERRED=0: worst relative gradient error {worst:.2e}")


def test_graph_replay_with_the_late_weight_gradient_launch_inside():
    """The first block of test_graph_replayed_steps_equal_eager_steps at batch 160 (D = 4, four levels): the captured iteration holds wgrad_multi_kernel (the late
    launch, on from batch 48) and the large-tile launches.  Six steps through step(use_graph=True), t and the noise supplied and the batch changing per step,
    against six eager loss_backward + adam_step pairs: losses, parameters and both Adam moments to 1e-6 relative."""
    from mpd_public_amd.trainer import TrainStep
    B, D, opt = 160, 4, 1
    x0, noise, hc, tt = _batch(B, D)
    x0, noise, hc = x0.cuda(), noise.cuda(), _cuda(hc)
    tts = [tt.cuda(), ((torch.arange(B) * 11 + 3) % T).cuda()]
    ts_e, ts_g = TrainStep(_model(D, opt)), TrainStep(_model(D, opt))
    losses_e, losses_g = [], []
    for k in range(6):
        tk = tts[k % 2]
        nz = noise * (1.0 + 0.1 * k)
        xb = x0 * (1.0 - 0.05 * k)   # the replay must read the copies, not the captured tensors' first contents
        le, _ = ts_e.loss_backward(xb, hc, t=tk, noise=nz)
        ts_e.adam_step(1e-3, max_norm=1.0)
        losses_e.append(float(le))
        losses_g.append(float(ts_g.step(xb, hc, 1e-3, max_norm=1.0, t=tk, noise=nz, use_graph=True)))
    assert "_graphs" in ts_g.__dict__ and len(ts_g._graphs) == 1, "the third step was meant to capture"
    assert ts_g.step_count == ts_e.step_count == 6
    assert len(set(losses_e)) == 6
    np.testing.assert_allclose(losses_g, losses_e, rtol=1e-6)
    a, b = ts_g.fp.flat.detach().cpu(), ts_e.fp.flat.detach().cpu()
    assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    for a, b in ((ts_g.exp_avg, ts_e.exp_avg), (ts_g.exp_avg_sq, ts_e.exp_avg_sq)):
        assert float((a - b).abs().max().cpu()) <= 1e-6 * float(b.abs().max().cpu())
