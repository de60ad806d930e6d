"""Weight regimes for the U-Net's Conv1dBlocks, their float64 / float32 oracle evaluation and the bounds the kernels are held to.

synthetic.synth_state_dict gives GroupNorm weights in 1 +- 0.1, GroupNorm biases in +- 0.1 and convolution biases in +- 0.05: every GroupNorm input is O(1)
with variance O(0.1) and every Mish argument lies in about [-4, 4].  A checkpoint trained elsewhere promises none of that.  Each regime below is a pure
function state_dict -> state_dict applied to synth_state_dict's output, network-wide (every kernel family sees it); new values come from
synthetic.hash_uniform streams named after the parameter.

  plain       unchanged
  offset100   every *.block.0.bias += 100: a common offset in front of every GroupNorm (a one-pass variance cancels)
  tinyvar     every *.block.0.weight and *.block.0.bias x 1e-3: the variance is ~1e-7, eps = 1e-5 decides
  constgroup  every *.blocks.1.block.0.weight = 0, its bias = 0.25: variance exactly 0, constant regions, rstd = 1 / sqrt(eps) = 316 in the backward pass
  gsign       every *.block.2.weight ~ U(-1.5, 1.5), every 7th channel exactly 0
  bigaffine   *.block.2.weight ~ U(2, 10), *.block.2.bias ~ U(-20, 20): Mish arguments beyond 20.8 (softplus threshold / the exponent clamp), below -20
              and beyond 44.4 (where e^x (e^x + 2) overflows float32)
  bigtime     every *.cond_mlp.1.bias ~ U(-30, 30): the time bias added behind Mish is much larger than the activations

Bounds (K, K_G: measured, see profiles/unet_regimes.md and DESIGN.md section 6):
  forward   max|y - y64| <= K e_ref + 2^-23 max|y64|,                e_ref = max|fp32 oracle - fp64 oracle| of that very case (one torch thread)
  gradient  max|g - g64| <= K_G e_ref(tensor) + 2^-20 max|g64(tensor)| per tensor, e_ref from fp32 autograd of the oracle; a tensor whose fp64 gradient
            is exactly zero stays below 2^-20 max|g64| over ALL tensors
  loss      |loss - loss64| <= K_G |loss32 - loss64| + 2^-22 |loss64|
"""
import contextlib

import numpy as np
import torch

from mpd_public_amd import synthetic as syn
from oracle import train as otrain
from oracle import unet as ounet

REGIMES = ("plain", "offset100", "tinyvar", "constgroup", "gsign", "bigaffine", "bigtime")
K = 4      # forward: twice the largest ratio measured on the MI355X (1.75), rounded up (profiles/unet_regimes.md)
K_G = 4    # gradients and loss: likewise (2.00 on a gradient tensor, 1.89 on the loss)


def _u(regime, name, v, lo, hi):
    # (the stream is named `regime@parameter`.  Under `bigaffine` an argument above 44.4 needs a channel with weight > 9.7 AND bias > 19.5 - two or three of
    #  the network's ~5000 - and a position 2.4 sigma out on it: with this form of the name one such channel lies in a level every trajectory crosses with
    #  64 positions, so that even a batch of three reaches the overflow branch; assert_bigaffine_shares checks it per case, from the reference.)
    return torch.from_numpy(syn.hash_uniform(f"{regime}@{name}", v.numel(), lo, hi).astype(np.float32).reshape(tuple(v.shape)))


def apply_regime(sd, regime):
    """a new state dict (float32 clones); `sd` is left as it is"""
    assert regime in REGIMES, regime
    out = {k: v.clone() for k, v in sd.items()}
    for k, v in out.items():
        if regime == "offset100" and k.endswith(".block.0.bias"):
            v += 100.0
        elif regime == "tinyvar" and (k.endswith(".block.0.weight") or k.endswith(".block.0.bias")):
            v *= 1e-3
        elif regime == "constgroup" and k.endswith(".blocks.1.block.0.weight"):
            v.zero_()
        elif regime == "constgroup" and k.endswith(".blocks.1.block.0.bias"):
            v.fill_(0.25)
        elif regime == "gsign" and k.endswith(".block.2.weight"):
            v.copy_(_u(regime, k, v, -1.5, 1.5))
            v[::7] = 0.0
        elif regime == "bigaffine" and k.endswith(".block.2.weight"):
            v.copy_(_u(regime, k, v, 2.0, 10.0))
        elif regime == "bigaffine" and k.endswith(".block.2.bias"):
            v.copy_(_u(regime, k, v, -20.0, 20.0))
        elif regime == "bigtime" and k.endswith(".cond_mlp.1.bias"):
            v.copy_(_u(regime, k, v, -30.0, 30.0))
    return out


# ---------------------------------------------------------------------------------------------- evaluation
@contextlib.contextmanager
def one_thread():
    """the oracle's fp32 results move with the host's thread count (ATen's reduction order): ONE thread pins them on every host"""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(old)


@contextlib.contextmanager
def swapped_block(fn):
    """oracle.unet.conv1d_block replaced by fn(sd, prefix, x) for the enclosed calls (unet_forward and loss_and_grads look it up per call)"""
    old = ounet.conv1d_block
    ounet.conv1d_block = fn
    try:
        yield
    finally:
        ounet.conv1d_block = old


def _recording_block(args):
    """oracle.unet.conv1d_block with the same calls, keeping every Mish argument"""
    import torch.nn.functional as F

    def block(sd, p, x):
        w = sd[p + ".block.0.weight"]
        y = F.conv1d(x, w, sd[p + ".block.0.bias"], padding=w.shape[-1] // 2)
        y = F.group_norm(y, ounet.group_norm_n_groups(w.shape[0]), sd[p + ".block.2.weight"], sd[p + ".block.2.bias"], eps=1e-5)
        args.append(y.detach().reshape(-1))
        return F.mish(y)
    return block


def mish_shares(args):
    a = torch.cat(args)
    return float((a > 20.8).double().mean()), float((a < -20.0).double().mean()), int((a > 44.4).sum())


def forward_ref(sd, x, tv):
    """-> dict(y64, y32, e_ref, ymax, shares): the oracle's U-Net output in float64 and float32 (one thread), e_ref = max|y32 - y64|, ymax = max|y64|,
    shares = (share of the fp64 run's Mish arguments above 20.8, share below -20, number above 44.4)"""
    args = []
    with swapped_block(_recording_block(args)):
        y64 = ounet.unet_forward({k: v.double() for k, v in sd.items()}, x.double(), tv)
    shares = mish_shares(args)
    with one_thread():
        y32 = ounet.unet_forward(sd, x, tv)
    assert bool(torch.isfinite(y64).all()) and bool(torch.isfinite(y32).all())
    return {"y64": y64, "y32": y32, "e_ref": float((y32.double() - y64).abs().max()), "ymax": float(y64.abs().max()), "shares": shares}


def assert_bigaffine_shares(shares):
    """what makes `bigaffine` the regime of the three Mish branches - from the reference alone"""
    assert shares[0] >= 0.01 and shares[1] >= 0.01 and shares[2] >= 1, shares


def forward_ratio(y, ref, sl=slice(None)):
    """(max|y - y64| / (e_ref + floor), max|y - y64|, e_ref, floor) over the trajectories `sl` of the reference"""
    y64, y32 = ref["y64"][sl], ref["y32"][sl]
    err = float((y.detach().cpu().double() - y64).abs().max())
    e_ref, floor = float((y32.double() - y64).abs().max()), 2.0 ** -23 * float(y64.abs().max())
    return err / (e_ref + floor), err, e_ref, floor


def check_forward(y, ref, label, sl=slice(None), k=None):
    """finite and max|y - y64| <= K e_ref + 2^-23 max|y64|; prints the figures before it asserts; -> the ratio err / (e_ref + floor)"""
    k = K if k is None else k
    assert bool(torch.isfinite(y).all()), f"{label}: non-finite output"
    ratio, err, e_ref, floor = forward_ratio(y, ref, sl)
    print(f"REGIME fwd {label}: err {err:.3e} e_ref {e_ref:.3e} floor {floor:.3e} ratio {ratio:.3f}")
    assert err <= k * e_ref + floor, (label, err, e_ref, floor, ratio)
    return ratio


def grads_ref(sd, x0, tv, hc, noise, T):
    """-> dict(loss64, g64, loss32, g32, shares) of oracle.train.loss_and_grads in float64 and float32 (one thread); shares as forward_ref's, of the fp64 pass"""
    args = []
    with swapped_block(_recording_block(args)):
        loss64, g64 = otrain.loss_and_grads(sd, x0, tv, hc, noise, T, dtype=torch.float64)
    with one_thread():
        loss32, g32 = otrain.loss_and_grads(sd, x0, tv, hc, noise, T)
    return {"loss64": float(loss64), "g64": g64, "loss32": float(loss32), "g32": g32, "shares": mish_shares(args)}


def grad_ratios(loss, grads, ref):
    """-> (worst ratio, its tensor, loss ratio, number of tensors whose fp64 gradient is exactly zero, list of violations at K_G = 1 scale-free form):
    per tensor err / (e_ref + 2^-20 max|g64|); zero-gradient tensors: err / (2^-20 max|g64| over all tensors)"""
    gmax_all = max(float(g.abs().max()) for g in ref["g64"].values())
    worst, at, zeros, rows = 0.0, None, 0, []
    for name, g64 in ref["g64"].items():
        g = grads[name].detach().cpu().double()
        assert g.shape == g64.shape, name
        if not bool(torch.isfinite(g).all()):
            rows.append((name, float("inf"), 0.0, 0.0))
            worst, at = float("inf"), name
            continue
        err, gmax = float((g - g64).abs().max()), float(g64.abs().max())
        if gmax == 0.0:
            zeros += 1
            e_ref, floor = 0.0, 2.0 ** -20 * gmax_all
        else:
            e_ref, floor = float((ref["g32"][name].double() - g64).abs().max()), 2.0 ** -20 * gmax
        rows.append((name, err, e_ref, floor))
        if err / (e_ref + floor) > worst:
            worst, at = err / (e_ref + floor), name
    l_err, l_ref, l_floor = abs(float(loss) - ref["loss64"]), abs(ref["loss32"] - ref["loss64"]), 2.0 ** -22 * abs(ref["loss64"])
    return worst, at, (l_err, l_ref, l_floor), zeros, rows


def check_grads(loss, grads, ref, label, k=None):
    """loss and every gradient inside the bounds of the module docstring; prints the figures before it asserts; -> (worst ratio, loss ratio)"""
    k = K_G if k is None else k
    worst, at, (l_err, l_ref, l_floor), zeros, rows = grad_ratios(loss, grads, ref)
    print(f"REGIME bwd {label}: worst ratio {worst:.3f} ({at}) loss err {l_err:.3e} ref {l_ref:.3e} floor {l_floor:.3e} ratio {l_err / (l_ref + l_floor):.3f} "
          f"zero-gradient tensors {zeros}")
    assert np.isfinite(float(loss)), label
    bad = [(n, e, r, f) for n, e, r, f in rows if not e <= k * r + f]
    assert not bad, (label, bad[:5])
    assert l_err <= k * l_ref + l_floor, (label, l_err, l_ref, l_floor)
    return worst, l_err / (l_ref + l_floor)
