"""The arguments of the training entry points that trainer.TrainStep never passes (include/mpdx.h "training step"; kernels csrc/train.hpp,
csrc/loss.hpp, csrc/mpdx.hip): the weight table of mpdx_train_loss_backward, open ends (hard_start / hard_goal NULL), the optimiser kernels
at sizes, alignments and grid caps other than the network's, mpdx_weighted_loss at ragged shapes, mpdx_q_sample's clamp of t and
mpdx_add_noise without noise / with a chain output.  References: float64 autograd of the oracle (oracle/train.loss_and_grads with
`weights`) and tests/train_entry_ref.py (pinned on the CPU by tests/test_train_entry_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

import train_entry_ref as R
from helpers import synth_sd, t, DIM_MULTS

pytestmark = pytest.mark.gpu

T = 25
TT0 = torch.tensor([3, 24, 0, 12, 12, 7])   # TTS[0] of test_gpu_train.py
U = 2.0 ** -24   # one fp32 rounding to nearest, relative (half an ulp at the top of a binade)
SENTINEL = -12345.5


# ------------------------------------------------------------------------------------------------ the training pass
def _model(H, D, opt, loss_type="l2", predict_epsilon=True):
    import mpd_public_amd as m
    net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    return m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=predict_epsilon, loss_type=loss_type).cuda()


@functools.lru_cache(maxsize=None)
def _batch(H, D, B=6):
    x0, noise = t(f"te_x0_H{H}_D{D}_B{B}", (B, H, D), "uniform", 0.8), t(f"te_noise_H{H}_D{D}_B{B}", (B, H, D))
    hc = {0: t(f"te_hc0_H{H}_D{D}_B{B}", (B, D), "uniform", 0.7), H - 1: t(f"te_hc1_H{H}_D{D}_B{B}", (B, D), "uniform", 0.7)}
    tt = TT0 if B == 6 else (torch.arange(B) * 7) % T
    return x0, noise, hc, tt


def _weights(H, D, zero_velocity=False):
    w = 0.1 + t(f"te_w_H{H}_D{D}", (H, D), "uniform").abs()   # in [0.1, 1.1]
    if zero_velocity:
        w[:, D // 2:] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _oracle(H, D, opt, B, loss_type, pred_eps, ends, weighted, zero_velocity=False):
    """float64 autograd of the oracle, computed once per case and shared.  `ends`: which hard conditions are given, "both" | "none" | "start" | "goal"."""
    from oracle import train as otrain
    x0, noise, hc, tt = _batch(H, D, B)
    w = _weights(H, D, zero_velocity) if weighted else None
    return otrain.loss_and_grads(synth_sd(D, opt), x0, tt, _ends(hc, H, ends), noise, T, predict_epsilon=pred_eps, loss_type=loss_type, dtype=torch.float64,
                                 weights=w)


def _ends(hc, H, ends):
    return {"both": hc, "none": None, "start": {0: hc[0]}, "goal": {H - 1: hc[H - 1]}}[ends]


def _loss_backward_weighted(ts, x_start, hard_conds, tt, noise, weights, loss_scale=1.0):
    """lib.mpdx_train_loss_backward with every argument filled as TrainStep.loss_backward fills it, plus `weights_hd`"""
    from mpd_public_amd import _lib
    m = ts.model
    lib, h = _lib.load(), ts.unet._handle()
    x_start = x_start.to(torch.float32).contiguous()
    B, H, D = x_start.shape
    dev = x_start.device
    tt = tt.to(device=dev, dtype=torch.long).reshape(-1).contiguous()
    noise = noise.to(torch.float32).contiguous()
    weights = weights.to(device=dev, dtype=torch.float32).contiguous()
    assert weights.shape == (H, D)
    hs, hg = m._hard_tables(hard_conds, B, H, D, dev)
    need = int(lib.mpdx_train_workspace_floats(h, B))
    if ts._ws is None or ts._ws.numel() < need:
        ts._ws = torch.empty(need, dtype=torch.float32, device=dev)
    ts.pack(sync_engine=False)
    _lib.check(lib.mpdx_train_loss_backward(
        h, ts.fp.flat.data_ptr(), ts._packed().data_ptr(), ts.fp.packedT.data_ptr(), ts.fp.grad.data_ptr(), x_start.data_ptr(),
        noise.data_ptr(), tt.data_ptr(), m.sqrt_alphas_cumprod.data_ptr(), m.sqrt_one_minus_alphas_cumprod.data_ptr(),
        ts._freqs.data_ptr(), hs.data_ptr() if hs is not None else None, hg.data_ptr() if hg is not None else None, weights.data_ptr(),
        int(m.n_diffusion_steps), B, 1 if m.predict_epsilon else 0, 1 if m.loss_type == "l1" else 0, float(loss_scale),
        ts.loss_buf.data_ptr(), ts._ws.data_ptr(), _lib.current_stream()), "mpdx_train_loss_backward")
    if not ts.fp.grads_bound():
        ts.fp.bind_grads()
    return ts.loss_buf[0].clone()


def _hold_to_oracle(dm, loss, ref_loss, ref, loss_type, grad_scale=1.0, exact_zero_from=None):
    """the yardstick of test_gpu_train.py::test_loss_backward_every_gradient_vs_oracle: loss within 5e-6 max(1, |ref|), every parameter's gradient
    within 2e-4 (l2) / 2e-3 (l1) of the largest reference entry of that parameter.  -> worst relative gradient error"""
    assert abs(float(loss) - float(ref_loss)) < 5e-6 * max(1.0, abs(float(ref_loss))), (float(loss), float(ref_loss))
    worst = 0.0
    for name, p in dm.model.named_parameters():
        g, r = p.grad.detach().cpu().double(), ref[name] * grad_scale
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), name
        if exact_zero_from is not None and name in ("final_conv.1.weight", "final_conv.1.bias"):
            assert bool((g[exact_zero_from:] == 0.0).all()), name
            assert float(g[:exact_zero_from].abs().max()) > 0, name
        tol = (2e-4 if loss_type == "l2" else 2e-3) * max(float(r.abs().max()), 1e-7)
        err = float((g - r).abs().max())
        worst = max(worst, err / max(float(r.abs().max()), 1e-7))
        assert err <= tol, (name, err, float(r.abs().max()))
    return worst


# (H, D, opt, loss_type, pred_eps, loss_scale, zero velocity half): train_loss_kernel's LDS-staged form at H = 64 (32 rows x D <= 1024 per block; D = 32
# is the guard's edge), its padded-container form at H = 48 (Hc = 64; any D <= 32).  unet_input_dim = 32 throughout.
WEIGHTED_CASES = [(64, 4, 1, "l2", True, 1.0, False), (64, 14, 0, "l1", False, 1.0, False), (64, 32, 0, "l2", True, 1.0, False),
                  (48, 14, 1, "l2", True, 1.0, False), (48, 24, 1, "l2", True, 1.0, False),
                  (64, 4, 1, "l2", True, 0.25, False), (48, 14, 1, "l2", True, 1.0, True)]


@pytest.mark.parametrize("H,D,opt,loss_type,pred_eps,loss_scale,zero_velocity", WEIGHTED_CASES)
def test_weighted_loss_backward_every_gradient_vs_oracle(H, D, opt, loss_type, pred_eps, loss_scale, zero_velocity):
    """mpdx_train_loss_backward with a weight table (0.1 + |u|, or that with a zero velocity half): the loss - never scaled - and d (loss_scale *
    loss) / d (every parameter) against float64 autograd of (err * weights).mean().  With the velocity half of the table zero, rows d >= D / 2 of
    final_conv[1]'s weight and bias gradients are exactly 0.0 (every term of their sums is a product with a zero dE)."""
    from mpd_public_amd.trainer import TrainStep
    dm = _model(H, D, opt, loss_type, pred_eps)
    x0, noise, hc, tt = _batch(H, D)
    ts = TrainStep(dm)
    loss = _loss_backward_weighted(ts, x0.cuda(), {k: v.cuda() for k, v in hc.items()}, tt.cuda(), noise.cuda(), _weights(H, D, zero_velocity), loss_scale)
    ref_loss, ref = _oracle(H, D, opt, 6, loss_type, pred_eps, "both", True, zero_velocity)
    worst = _hold_to_oracle(dm, loss, ref_loss, ref, loss_type, grad_scale=loss_scale, exact_zero_from=D // 2 if zero_velocity else None)
    print(f"weighted H={H} D={D} opt={opt} {loss_type} scale={loss_scale} zero_velocity={zero_velocity}: loss {float(loss):.6f} (ref {float(ref_loss):.6f}), "
          f"worst relative gradient error {worst:.2e} (bound {2e-4 if loss_type == 'l2' else 2e-3:.0e})")


def test_weighted_loss_backward_plain_form_at_width_128_vs_oracle():
    """train_loss_kernel's third form (neither LDS-staged nor a padded container) runs where the staged form's guard fails at a power-of-two horizon:
    never at unet_input_dim 32 or 64 (D * C <= 1024 for every accepted D), but at width 128 with 8 < state_dim <= 16 (and 256 with 4 < state_dim <=
    16), which mpdx_unet_create accepts (GroupNorm groups of 16 / 32 channels).  Width 128 x (1, 2), D = 14, weighted, both ends conditioned."""
    import mpd_public_amd as m
    from mpd_public_amd import synthetic as syn
    from mpd_public_amd.trainer import TrainStep
    from oracle import train as otrain
    from oracle.unet import unet_param_shapes
    H, D, width, mults = 64, 14, 128, (1, 2)
    sd = syn.synth_state_dict(unet_param_shapes(D, width, mults))
    net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=width, dim_mults=mults)
    net.load_state_dict(sd, strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True, loss_type="l2").cuda()
    x0, noise, hc, tt = _batch(H, D)
    w = _weights(H, D)
    loss = _loss_backward_weighted(TrainStep(dm), x0.cuda(), {k: v.cuda() for k, v in hc.items()}, tt.cuda(), noise.cuda(), w)
    ref_loss, ref = otrain.loss_and_grads(sd, x0, tt, hc, noise, T, dtype=torch.float64, weights=w)
    worst = _hold_to_oracle(dm, loss, ref_loss, ref, "l2")
    print(f"weighted, plain form (width 128, D=14): loss {float(loss):.6f} (ref {float(ref_loss):.6f}), worst relative gradient error {worst:.2e} (bound 2e-04)")


@pytest.mark.parametrize("D,opt,B,ends", [(4, 1, 6, "none"), (4, 1, 6, "start"), (4, 1, 6, "goal"), (14, 0, 6, "none"), (14, 0, 6, "start"), (14, 0, 6, "goal"),
                                          (4, 1, 64, "none")])
def test_open_ends_loss_backward_vs_oracle(D, opt, B, ends):
    """TrainStep.loss_backward with no hard conditions or only one of the two (hard_start / hard_goal reach q_sample, the loss and its gradient as
    NULL): an open end's row carries loss and gradient, a conditioned one is masked.  B = 64: the late weight-gradient path."""
    from mpd_public_amd.trainer import TrainStep
    H, lt = 64, "l2"
    ref_loss, ref = _oracle(H, D, opt, B, lt, True, ends, False)
    _, both = _oracle(H, D, opt, B, lt, True, "both", False)
    k = "final_conv.1.weight"   # not vacuous: opening the end moves the reference by more than ten tolerances
    moved = float((ref[k] - both[k]).abs().max()) / float(ref[k].abs().max())
    assert moved > 10 * 2e-4, moved
    dm = _model(H, D, opt, lt, True)
    x0, noise, hc, tt = _batch(H, D, B)
    hcd = _ends({k_: v.cuda() for k_, v in hc.items()}, H, ends)
    loss, _ = TrainStep(dm).loss_backward(x0.cuda(), hcd, t=tt.cuda(), noise=noise.cuda())
    worst = _hold_to_oracle(dm, loss, ref_loss, ref, lt)
    print(f"open ends D={D} opt={opt} B={B} {ends}: reference moved {moved:.2e} of max|g| against both ends conditioned; worst relative gradient error "
          f"{worst:.2e} (bound 2e-04)")


# ------------------------------------------------------------------------------------------------ mpdx_weighted_loss
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("l1", [0, 1])
@pytest.mark.parametrize("B,H,D,all_ends", [(1, 8, 2, False), (3, 24, 7, True), (5, 48, 14, True), (40, 64, 14, False), (2, 64, 33, True)])
def test_weighted_loss_kernel_ragged_shapes_vs_ref(B, H, D, all_ends, l1, weighted):
    """mpdx_weighted_loss (one workgroup of 1024 threads, eight loads in flight per thread, indices advanced by carries in d and l) at 16 elements,
    at shapes where 1024 % D != 0 and the row index carries, and at 35 elements per thread (five unrolled trips).  The device sums in double; the
    fp32 roundings are the per-element ones weighted_loss_ref reproduces: 1e-6 relative."""
    from mpd_public_amd import _lib
    lib = _lib.load()
    tag = f"{B}_{H}_{D}"
    pred, targ = t(f"tewl_pred_{tag}", (B, H, D)), t(f"tewl_targ_{tag}", (B, H, D))
    w = (0.1 + t(f"tewl_w_{tag}", (H, D), "uniform").abs()) if weighted else None
    hs, hg = t(f"tewl_hs_{tag}", (B, D), "uniform"), t(f"tewl_hg_{tag}", (B, D), "uniform")
    dp, dt, dw, dhs, dhg = pred.cuda(), targ.cuda(), None if w is None else w.cuda(), hs.cuda(), hg.cuda()
    out = torch.full((3,), SENTINEL, device="cuda")
    worst = 0.0
    for use_s, use_g in ([(True, True), (True, False), (False, True), (False, False)] if all_ends else [(True, True)]):
        _lib.check(lib.mpdx_weighted_loss(dp.data_ptr(), dt.data_ptr(), None if dw is None else dw.data_ptr(), dhs.data_ptr() if use_s else None,
                                          dhg.data_ptr() if use_g else None, l1, out.data_ptr() + 4, B, H, D, _lib.current_stream()), "mpdx_weighted_loss")
        want = R.weighted_loss_ref(pred, targ, w, hs if use_s else None, hg if use_g else None, l1)
        got = out.cpu()
        assert float(got[0]) == SENTINEL and float(got[2]) == SENTINEL
        rel = abs(float(got[1]) - want) / want
        worst = max(worst, rel)
        assert rel <= 1e-6, (use_s, use_g, float(got[1]), want)
    print(f"weighted_loss {B}x{H}x{D} l1={l1} weighted={weighted}: worst relative error {worst:.2e} (bound 1e-06)")


# ------------------------------------------------------------------------------------------------ mpdx_adam_step / mpdx_ema_update
SIZES = [1, 3, 4, 5, 255, 1027, 4 * 2 ** 20 + 7]
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
LAYOUTS = {"aligned": (4, 4, 4, 4), "all_offset": (5, 5, 5, 5), "grads_offset": (4, 5, 4, 4)}   # elements in front of (params, grads, exp_avg, exp_avg_sq)


@functools.lru_cache(maxsize=None)
def _stream(name):
    """4 * 2^20 + 7 hash-uniform values in [-1, 1); every size takes a prefix"""
    return t(name, (SIZES[-1],), "uniform")


def _guarded(values, lead):
    """`values` on the device with `lead` sentinel elements in front (torch's allocations are 512-byte aligned: lead = 4 starts the range on a 16-byte
    boundary, 5 one float past it) and four behind"""
    n = values.numel()
    buf = torch.full((lead + n + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    buf[lead:lead + n] = values.cuda()
    assert buf.data_ptr() % 16 == 0
    return buf


def _guards_intact(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all())


def _norm_roundings(n):
    """fp32 roundings on the longest path into the gradient norm's sum of squares: sumsq_kernel runs min(ceil(n / 256), 1024) blocks of 256 threads, a
    thread chains one fmaf per element (ceil(n / threads) of them), then 6 xor-shuffle levels and 2 levels over the four waves; adam_kernel chains
    ceil(blocks / 256) partial sums per thread, then the same 6 + 2 levels"""
    nb = min((n + 255) // 256, 1024)
    return -(-n // (nb * 256)) + 8 + -(-nb // 256) + 8


def _gradient(n, step, mode):
    """step k's gradient: one sign per element over the three steps (b1 m and (1 - b1) g never cancel, so m' has a relative bound), magnitudes that
    change per element and step; scaled to norm 3 ("clip": max_norm 1 clips) or 0.3 ("under": it does not)"""
    g = (_stream("te_adam_g")[:n] * (0.25 + _stream(f"te_adam_s{step}")[:n].abs())).double()
    if mode != "off":
        g = g * ((3.0 if mode == "clip" else 0.3) / float(torch.sqrt((g * g).sum())))
    return g.float()


def _adam_three_steps(n, layout, mode, counter="host"):
    """Three consecutive mpdx_adam_step calls, each held to adam_ref on the SAME fp32 inputs (the device's own state of the step before).

    fp32 roundings (each at most U = 2^-24 relative; -ffp-contract may fuse some away, never add one), from adam_kernel and mpdx_adam_step:
      gi = g * coef                      1, only where clipping acts (coef == 1.0f is exact); coef itself: the norm's bound + 2 (nrm + 1e-6f, the division)
      m' = b1 m + (1 - b1) gi            4 (1 - b1, two products, the sum)                       + gi's                 -> N_m
      v' = b2 v + (1 - b2) gi gi         5 (1 - b2, three products, the sum)                     + twice gi's           -> N_v
      p - p' = step m' / (sqrt(v') / bc2_sqrt + eps),  step = lr / bc1
                                         8 (bc1 and bc2_sqrt: one rounding each of a double value; the divisions lr / bc1 and / bc2_sqrt; step * m';
                                            sqrtf; + eps; the last division) + N_m + N_v / 2                                     -> N_u
      p'                                 one more rounding, of p - update: within one ulp of p
      norm = sqrtf(sum g^2)              _norm_roundings(n) on an all-positive sum, halved by the square root
    Without clipping that is N_m = 4, N_v = 5, N_u = 14.5; clipping at n = 4 * 2^20 + 7 (37 roundings into the sum): 25.5, 48, 57.5.  Measured on the
    MI355X, in the same units: m' <= 2.1, v' <= 4.3, p - p' <= 5.7, norm and coef <= 1.2.  (With the bias corrections formed as 1.0f - (float)pow(beta, t),
    as they were, p - p' of step 2 is 50 ... 61: beta2^2 rounded to fp32 is 1.5e-5 of 1 - beta2^2.)
    -> per step [(p', m', v') fp32 CPU tensors], after the asserts."""
    from mpd_public_amd import _lib
    lib = _lib.load()
    lead = LAYOUTS[layout]
    max_norm = 0.0 if mode == "off" else 1.0
    bufs = [_guarded(0.5 * _stream("te_adam_p")[:n], lead[0]), _guarded(torch.zeros(n), lead[1]), _guarded(torch.zeros(n), lead[2]), _guarded(torch.zeros(n), lead[3])]
    ptr = [b.data_ptr() + 4 * l for b, l in zip(bufs, lead)]
    assert [p % 16 for p in ptr] == [4 * (l - 4) for l in lead]
    view = [b[l:l + n] for b, l in zip(bufs, lead)]
    scratch = torch.zeros(2048, dtype=torch.float32, device="cuda")
    if counter == "device_lr":
        scratch[5] = LR
    nr = _norm_roundings(n) / 2
    out, worst = [], {"p": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0, "coef": 0.0}
    for step in (1, 2, 3):
        g = _gradient(n, step, mode)
        view[1].copy_(g)
        p0, m0, v0 = (view[i].cpu() for i in (0, 2, 3))
        _lib.check(lib.mpdx_adam_step(ptr[0], ptr[1], ptr[2], ptr[3], n, -1.0 if counter == "device_lr" else LR, BETAS[0], BETAS[1], EPS,
                                      step if counter == "host" else -1, max_norm, scratch.data_ptr(), _lib.current_stream()), "mpdx_adam_step")
        p1, m1, v1 = (view[i].cpu() for i in (0, 2, 3))
        for b, l in zip(bufs, lead):
            assert _guards_intact(b, l, n), (n, layout, step)
        assert torch.equal(view[1].cpu(), g)
        if counter != "host":
            assert int(scratch.view(torch.int32)[4]) == step
        rp, rm, rv, norm, coef = R.adam_ref(p0, g, m0, v0, LR, BETAS, EPS, step, max_norm)
        clips = coef < 1.0
        assert clips == (mode == "clip")
        c = nr + 2 if clips else 0.0
        n_m, n_v = 4 + (1 + c if clips else 0), 5 + (2 + 2 * c if clips else 0)
        n_u = 8 + n_m + n_v / 2
        if max_norm > 0:
            dn, dc = float(scratch[0]), float(scratch[1])
            worst["norm"] = max(worst["norm"], abs(dn - norm) / norm / U)
            worst["coef"] = max(worst["coef"], abs(dc - coef) / coef / U)
            assert abs(dn - norm) <= nr * U * norm, (dn, norm)
            assert abs(dc - coef) <= nr * U * coef, (dc, coef)
        em, ev = (m1.double() - rm).abs() / rm.abs(), (v1.double() - rv).abs() / rv
        upd = (p0.double() - rp).abs()
        ep = ((p1.double() - rp).abs() - torch.from_numpy(np.spacing(p0.abs().numpy())).double()).clamp_min(0) / upd
        for key, e, bound in (("m", em, n_m), ("v", ev, n_v), ("p", ep, n_u)):
            worst[key] = max(worst[key], float(e.max()) / U)
            assert float(e.max()) <= bound * U, (key, n, layout, mode, step, float(e.max()) / U, bound)
        out.append((p1, m1, v1))
    print(f"adam n={n} {layout} {mode} {counter}: worst error in units of 2^-24 relative - m' {worst['m']:.2f} (bound {n_m:.1f}), v' {worst['v']:.2f} ({n_v:.1f}), "
          f"p - p' beyond one ulp of p {worst['p']:.2f} ({n_u:.1f}), norm {worst['norm']:.2f} ({nr:.1f}), coef {worst['coef']:.2f} ({nr:.1f})")
    return out


@pytest.mark.parametrize("mode", ["off", "clip", "under"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_sizes_alignments_and_clipping_vs_ref(n, layout, mode):
    """mpdx_adam_step at sizes that are all tail (1, 3), one vector and a tail (5), no multiple of the block (255, 1027) and past the grid caps of
    adam_kernel (4096 blocks) and sumsq_kernel (1024 blocks, eight strides deep) with a tail of 3 (4 * 2^20 + 7); with every pointer 16-byte aligned
    (the vector path), all four one float past a boundary, or only the gradients (the scalar path); without clipping (max_norm 0), with max_norm 1
    against a norm of 3 (clips) and of 0.3 (does not).  Guard elements around every range stay untouched.  Bounds: _adam_three_steps."""
    _adam_three_steps(n, layout, mode)


@pytest.mark.parametrize("mode", ["off", "clip"])
@pytest.mark.parametrize("n", [5, 1027])
def test_adam_step_device_counter_vs_ref(n, mode):
    """The form a captured iteration runs: the step count on the device (step = -1: scratch[4] counts 1, 2, 3), then the learning rate there as
    well (lr = -1: scratch[5]) - the same bounds against adam_ref at steps 1, 2, 3.  Whether the bits equal the host-counted form's (the bias
    corrections come from the device's pow instead of the host's) is printed, not asserted."""
    host = _adam_three_steps(n, "aligned", mode)
    for counter in ("device", "device_lr"):
        dev = _adam_three_steps(n, "aligned", mode, counter)
        same = all(torch.equal(a, b) for hs, ds in zip(host, dev) for a, b in zip(hs, ds))
        print(f"adam n={n} {mode}: {counter} form bit-equal to the host-counted form: {same}")


@pytest.mark.parametrize("layout", ["aligned", "all_offset", "params_offset"])
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_sizes_and_alignments_vs_ref(n, layout):
    """mpdx_ema_update: ema' = ema * beta + (1 - beta) * p.  Two fp32 roundings: 1 - beta is exact for beta in [0.5, 1] (here 0.995f), the product
    (1 - beta) * p rounds once, and the sum is the one rounding of the fused multiply-add of ema * beta (-ffp-contract=on); with ema and p of one
    sign both are relative to terms no larger than the result: 2 * 2^-24 relative."""
    from mpd_public_amd import _lib
    lib = _lib.load()
    le, lp = {"aligned": (4, 4), "all_offset": (5, 5), "params_offset": (4, 5)}[layout]
    p = _stream("te_ema_p")[:n]
    ema = p * (0.5 + _stream("te_ema_s")[:n].abs())
    be, bp = _guarded(ema, le), _guarded(p, lp)
    _lib.check(lib.mpdx_ema_update(be.data_ptr() + 4 * le, bp.data_ptr() + 4 * lp, n, 0.995, _lib.current_stream()), "mpdx_ema_update")
    assert _guards_intact(be, le, n) and _guards_intact(bp, lp, n) and torch.equal(bp[lp:lp + n].cpu(), p)
    want = R.ema_ref(ema, p, 0.995)
    rel = float(((be[le:le + n].cpu().double() - want).abs() / want.abs()).max())
    print(f"ema n={n} {layout}: worst relative error {rel / U:.2f} x 2^-24 (bound 2)")
    assert rel <= 2 * U


# ------------------------------------------------------------------------------------------------ mpdx_q_sample / mpdx_add_noise
def test_q_sample_clamps_t_bit_for_bit():
    """mpdx_q_sample clamps t to [0, T) (include/mpdx.h): t = [-1, 0, T-1, T, 2^40, 3] behaves as [0, 0, T-1, T-1, T-1, 3]; hard_start only; the
    output range sits between guard elements.  Bit equality with the three separately rounded fp32 operations."""
    from mpd_public_amd import _lib
    from oracle import schedules as osched
    lib = _lib.load()
    B, H, D = 6, 24, 7
    buf = osched.make_buffers(T, "exponential")
    a, b = buf["sqrt_alphas_cumprod"].float().contiguous(), buf["sqrt_one_minus_alphas_cumprod"].float().contiguous()
    x0, nz, hs = t("teq_x0", (B, H, D), "uniform", 0.8), t("teq_nz", (B, H, D)), t("teq_hs", (B, D), "uniform", 0.7)
    tt = torch.tensor([-1, 0, T - 1, T, 2 ** 40, 3], dtype=torch.long)
    n = B * H * D
    out = _guarded(torch.zeros(n), 4)
    dx, dn, dt_, da, db, dhs = x0.cuda(), nz.cuda(), tt.cuda(), a.cuda(), b.cuda(), hs.cuda()
    _lib.check(lib.mpdx_q_sample(dx.data_ptr(), dn.data_ptr(), dt_.data_ptr(), da.data_ptr(), db.data_ptr(), dhs.data_ptr(), None, out.data_ptr() + 16,
                                 B, H, D, T, _lib.current_stream()), "mpdx_q_sample")
    assert _guards_intact(out, 4, n)
    got = out[4:4 + n].cpu().reshape(B, H, D)
    assert torch.equal(got, R.q_sample_ref(x0, nz, tt, a, b, hs, None))
    assert torch.equal(got, R.q_sample_ref(x0, nz, torch.tensor([0, 0, T - 1, T - 1, T - 1, 3]), a, b, hs, None))
    assert torch.equal(got[:, 0], hs) and not torch.equal(got[:, -1], got[:, 0])


@pytest.mark.parametrize("B,H,D", [(3, 24, 7), (2, 64, 14)])
def test_add_noise_without_noise_with_chain_and_one_end_bit_for_bit(B, H, D):
    """mpdx_add_noise with noise == NULL (only the hard conditions and the chain copy act), with a chain output (equals x afterwards) and with
    hard_goal only: bit equality with x + (scale * noise) * extra in separately rounded fp32 operations."""
    from mpd_public_amd import _lib
    lib = _lib.load()
    n = B * H * D
    x, nz = t(f"tean_x_{B}", (B, H, D)), t(f"tean_nz_{B}", (B, H, D))
    hs, hg = t(f"tean_hs_{B}", (B, D), "uniform", 0.7), t(f"tean_hg_{B}", (B, D), "uniform", 0.7)
    dn, dhs, dhg = nz.cuda(), hs.cuda(), hg.cuda()
    scale, extra = 0.3, 0.7
    for noise, s, g, chain in ((None, hs, hg, False), (None, None, hg, True), (nz, None, hg, True), (nz, hs, None, False), (nz, None, None, True)):
        xb, cb = _guarded(x.reshape(-1), 4), _guarded(torch.zeros(n), 4)
        _lib.check(lib.mpdx_add_noise(xb.data_ptr() + 16, None if noise is None else dn.data_ptr(), None if s is None else dhs.data_ptr(),
                                      None if g is None else dhg.data_ptr(), scale, extra, cb.data_ptr() + 16 if chain else None, B, H, D,
                                      _lib.current_stream()), "mpdx_add_noise")
        assert _guards_intact(xb, 4, n) and _guards_intact(cb, 4, n)
        got = xb[4:4 + n].cpu().reshape(B, H, D)
        assert torch.equal(got, R.add_noise_ref(x, noise, s, g, scale, extra)), (noise is None, s is None, g is None)
        if chain:
            assert torch.equal(cb[4:4 + n].cpu().reshape(B, H, D), got)
        else:
            assert bool((cb[4:4 + n] == 0).all())
        if noise is None:   # nothing but the conditioned rows changed
            keep = slice(0 if s is None else 1, H if g is None else H - 1)
            assert torch.equal(got[:, keep], x[:, keep])
