"""Plain-torch restatements of the training entry points of include/mpdx.h that take the SAME fp32 inputs as the device
(test infrastructure; used by tests/test_train_entry_cpu.py, which pins them, and tests/test_gpu_train_entry.py).

  adam_ref, ema_ref, weighted_loss_ref   float64 arithmetic on the fp32 inputs (the scalars lr / betas / eps / beta are rounded to
                                         fp32 first: the entry points take them as C floats, so that IS the input)
  q_sample_ref, add_noise_ref            float32, the same three separately rounded operations as the kernels (which promise bit
                                         equality: __fmul_rn / __fadd_rn, no contraction)
"""
import numpy as np
import torch


def f32(x) -> float:
    """the value a C float argument carries"""
    return float(np.float32(x))


def adam_ref(p, g, m, v, lr, betas, eps, step, max_norm):
    """clip_grad_norm_(max_norm) (max_norm > 0) + one torch.optim.Adam step (no weight decay, no amsgrad) in float64.
    -> (p', m', v', norm, coef); norm = |g|_2, coef = min(1, max_norm / (norm + 1e-6)) (1.0 without clipping)."""
    p, g, m, v = (x.detach().cpu().double() for x in (p, g, m, v))
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    norm = float(torch.sqrt((g * g).sum()))
    coef = min(1.0, f32(max_norm) / (norm + 1e-6)) if max_norm and max_norm > 0 else 1.0
    g = g * coef
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p1 = p - (lr / bc1) * m1 / (v1.sqrt() / bc2 ** 0.5 + eps)
    return p1, m1, v1, norm, coef


def ema_ref(ema, p, beta):
    """EMA.update_model_average: ema * beta + (1 - beta) * p in float64"""
    beta = f32(beta)
    return ema.detach().cpu().double() * beta + (1.0 - beta) * p.detach().cpu().double()


def _condition(x, hs, hg):
    x = x.clone()
    if hs is not None:
        x[:, 0, :] = hs.detach().cpu().to(x.dtype)
    if hg is not None:
        x[:, -1, :] = hg.detach().cpu().to(x.dtype)
    return x


def weighted_loss_ref(pred, targ, w, hs, hg, l1):
    """mean over B*H*D of |e| or e^2 (times w[H, D] where given), e = apply_hard_conditioning(pred) - targ.  The per-element operations
    are the device's separately rounded fp32 ones (subtract, square, times weight); the sum and the mean are float64. -> python float"""
    pred, targ = pred.detach().cpu().float(), targ.detach().cpu().float()
    e = _condition(pred, hs, hg) - targ
    q = e.abs() if l1 else e * e
    if w is not None:
        q = q * w.detach().cpu().float()
    return float(q.double().sum() / q.numel())


def q_sample_ref(x0, noise, t, sqrt_ac, sqrt_1mac, hs, hg):
    """fp32: sqrt_ac[t_b] * x0 + sqrt_1mac[t_b] * noise (two rounded products, one rounded sum), t clamped to [0, T), then the hard conditions"""
    T = sqrt_ac.numel()
    tc = t.detach().cpu().long().clamp(0, T - 1)
    a, b = sqrt_ac.detach().cpu().float()[tc].reshape(-1, 1, 1), sqrt_1mac.detach().cpu().float()[tc].reshape(-1, 1, 1)
    x = a * x0.detach().cpu().float() + b * noise.detach().cpu().float()
    return _condition(x, hs, hg)


def add_noise_ref(x, noise, hs, hg, scale, extra):
    """fp32: x + (scale * noise) * extra (noise None: x), then the hard conditions"""
    x = x.detach().cpu().float().clone()
    if noise is not None:
        s, e = torch.tensor(scale, dtype=torch.float32), torch.tensor(extra, dtype=torch.float32)
        x = x + (s * noise.detach().cpu().float()) * e
    return _condition(x, hs, hg)
