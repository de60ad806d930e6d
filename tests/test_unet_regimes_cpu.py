"""Proof, on the CPU, that the cases of tests/test_gpu_unet_regimes.py can fail: Conv1dBlock (convolution -> GroupNorm -> Mish) restated by hand in
float32, swapped into the oracle's U-Net, and held to the bounds of tests/regime_ref.py against the float64 oracle.

The `ok` restatement - two-pass biased variance, eps = 1e-5, Mish with the softplus threshold, the full GroupNorm backward - is inside the bounds on every
regime.  Each deliberately wrong variant - a one-pass variance, an unbiased variance, a missing or wrong eps, a Mish that overflows, statistics over the pad
rows of a horizon's container; in the backward pass a Mish derivative without its clamp, a GroupNorm backward without its vhat * mean(gm * vhat) term or with
rstd of var alone - misses them, or is non-finite, on at least one regime.  A variant no regime catches means the regimes are too weak."""
import pytest
import torch
import torch.nn.functional as F

import regime_ref as rr
from helpers import synth_sd, t
from oracle import unet as ounet

D, B, T = 4, 3, 100
_REF, _GREF = {}, {}


def _sd(regime, opt=1):
    return rr.apply_regime(synth_sd(D, opt), regime)


def _x(H):
    return t(f"regcpu_x_{H}", (B, H, D)), torch.full((B,), 37, dtype=torch.long)


def _fwd_ref(regime, H=64):
    if (regime, H) not in _REF:
        _REF[regime, H] = rr.forward_ref(_sd(regime), *_x(H))
    return _REF[regime, H]


def _batch(H=64):
    x0, noise = t("regcpu_x0", (B, H, D), "uniform", 0.8), t("regcpu_noise", (B, H, D))
    hc = {0: t("regcpu_hc0", (B, D), "uniform", 0.7), H - 1: t("regcpu_hc1", (B, D), "uniform", 0.7)}
    return x0, torch.tensor([3, 24, 61]), hc, noise


def _grad_ref(regime):
    if regime not in _GREF:
        x0, tv, hc, noise = _batch()
        _GREF[regime] = rr.grads_ref(_sd(regime), x0, tv, hc, noise, T)
    return _GREF[regime]


# ---------------------------------------------------------------------------------------------- the hand restatement
class _Normalize(torch.autograd.Function):
    """v [B, G, n] -> (v - mean) * rstd with the GroupNorm backward written out: dv = rstd (g - mean(g) - vhat mean(g vhat))"""
    @staticmethod
    def forward(ctx, v, eps, drop_vhat_term, bwd_eps):
        mean = v.mean(-1, keepdim=True)
        d = v - mean
        var = (d * d).mean(-1, keepdim=True)
        vhat = d * torch.rsqrt(var + eps)
        ctx.save_for_backward(vhat, var)
        ctx.opts = (drop_vhat_term, bwd_eps)
        return vhat

    @staticmethod
    def backward(ctx, g):
        vhat, var = ctx.saved_tensors
        drop, bwd_eps = ctx.opts
        rstd = torch.rsqrt(var + bwd_eps)
        dv = g - g.mean(-1, keepdim=True)
        if not drop:
            dv = dv - vhat * (g * vhat).mean(-1, keepdim=True)
        return rstd * dv, None, None, None


class _Mish(torch.autograd.Function):
    """Mish with the derivative written out as the kernels have it: th + v (1 - th^2) sigmoid(v), th = (n - 1) / (n + 1), n = (1 + e^min(v, 20))^2"""
    @staticmethod
    def forward(ctx, v, clamp):
        ctx.save_for_backward(v)
        ctx.clamp = clamp
        return F.mish(v)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        e = torch.exp(v.clamp(max=20.0) if ctx.clamp else v)
        n = (1.0 + e) * (1.0 + e)
        th = (n - 1.0) / (n + 1.0)
        return g * (th + v * (1.0 - th * th) * (e / (1.0 + e))), None


def make_block(variance="two-pass", unbiased=False, eps=1e-5, mish="threshold", container=False, hand_backward=False, mish_grad_clamp=True,
               drop_vhat_term=False, bwd_eps=1e-5):
    """conv1d_block of oracle/unet.py in the dtype of its operands, every step written out"""
    def block(sd, p, x):
        w, gamma, beta = sd[p + ".block.0.weight"], sd[p + ".block.2.weight"], sd[p + ".block.2.bias"]
        y = F.conv1d(x, w, sd[p + ".block.0.bias"], padding=w.shape[-1] // 2)
        Bn, C, L = y.shape
        G = ounet.group_norm_n_groups(C)
        v = y.reshape(Bn, G, -1)
        if hand_backward:
            vhat = _Normalize.apply(v, eps, drop_vhat_term, bwd_eps)
        else:
            n = v.shape[-1]
            if container:   # the rows behind the horizon are zero in a power-of-two container: statistics over ALL of its rows
                Lc = 1 << (L - 1).bit_length()
                vs = F.pad(y, (0, Lc - L)).reshape(Bn, G, -1)
                n = vs.shape[-1]
            else:
                vs = v
            mean = vs.sum(-1, keepdim=True) / n
            if variance == "one-pass":
                var = (vs * vs).sum(-1, keepdim=True) / n - mean * mean
            else:
                var = ((vs - mean) * (vs - mean)).sum(-1, keepdim=True) / n
            if unbiased:
                var = var * (n / (n - 1.0))
            vhat = (v - mean) / torch.sqrt(var + eps)
        u = vhat.reshape(Bn, C, L) * gamma[None, :, None] + beta[None, :, None]
        if hand_backward:
            return _Mish.apply(u, mish_grad_clamp)
        if mish == "unclamped":   # tanh(softplus(u)) = n / (n + 2), n = e^u (e^u + 2): overflows from u = 44.4 on
            e = torch.exp(u)
            n2 = e * (e + 2.0)
            return u * (n2 / (n2 + 2.0))
        return u * torch.tanh(torch.where(u > 20.0, u, torch.log1p(torch.exp(u.clamp(max=20.0)))))
    return block


def _forward_misses(block, regime, H=64):
    """does the float32 U-Net with `block` miss the forward bound (or is it non-finite) under `regime`?  -> (missed, ratio)"""
    ref = _fwd_ref(regime, H)
    x, tv = _x(H)
    with rr.swapped_block(block), rr.one_thread():
        y = ounet.unet_forward(_sd(regime), x, tv)
    if not bool(torch.isfinite(y).all()):
        return True, float("nan")
    ratio, err, e_ref, floor = rr.forward_ratio(y, ref)
    return not err <= rr.K * e_ref + floor, ratio


def _gradient_misses(block, regime):
    from oracle import train as otrain
    ref = _grad_ref(regime)
    x0, tv, hc, noise = _batch()
    with rr.swapped_block(block), rr.one_thread():
        loss, grads = otrain.loss_and_grads(_sd(regime), x0, tv, hc, noise, T)
    worst, at, (l_err, l_ref, l_floor), zeros, rows = rr.grad_ratios(loss, grads, ref)
    missed = any(not e <= rr.K_G * r + f for _, e, r, f in rows) or not l_err <= rr.K_G * l_ref + l_floor
    return missed, worst, zeros


# ---------------------------------------------------------------------------------------------- the regimes themselves
def test_regimes_are_pure_and_act_where_they_say():
    sd = synth_sd(D, 1)
    before = {k: v.clone() for k, v in sd.items()}
    for regime in rr.REGIMES:
        out = rr.apply_regime(sd, regime)
        assert all(torch.equal(sd[k], before[k]) for k in sd) and list(out) == list(sd)
        changed = {k for k in sd if not torch.equal(out[k], sd[k])}
        again = rr.apply_regime(sd, regime)
        assert all(torch.equal(out[k], again[k]) for k in sd)
        assert (regime == "plain") == (not changed)
        suffix = {"offset100": (".block.0.bias",), "tinyvar": (".block.0.weight", ".block.0.bias"), "constgroup": (".blocks.1.block.0.weight", ".blocks.1.block.0.bias"),
                  "gsign": (".block.2.weight",), "bigaffine": (".block.2.weight", ".block.2.bias"), "bigtime": (".cond_mlp.1.bias",), "plain": ()}[regime]
        assert changed == {k for k in sd if k.endswith(suffix)} if suffix else not changed
    g = rr.apply_regime(sd, "gsign")["mid_block1.blocks.0.block.2.weight"]
    assert bool((g[::7] == 0).all()) and float(g.min()) < -1.0 and float(g.max()) > 1.0
    a = rr.apply_regime(sd, "bigaffine")
    assert 2.0 <= float(a["mid_block1.blocks.0.block.2.weight"].min()) and float(a["mid_block1.blocks.0.block.2.bias"].abs().max()) <= 20.0


def test_bigaffine_reaches_all_three_mish_branches():
    """from the float64 reference alone: at least 1 % of the Mish arguments above 20.8, at least 1 % below -20, some above 44.4 - and none of it elsewhere"""
    rr.assert_bigaffine_shares(_fwd_ref("bigaffine")["shares"])
    assert _fwd_ref("plain")["shares"] == (0.0, 0.0, 0)


@pytest.mark.parametrize("regime", rr.REGIMES)
def test_ok_restatement_meets_the_forward_bound(regime):
    missed, ratio = _forward_misses(make_block(), regime)
    print(f"{regime}: e_ref {_fwd_ref(regime)['e_ref']:.2e}, ok ratio {ratio:.3f}")
    assert not missed, (regime, ratio)


WRONG_FORWARD = {   # variant -> (block, regimes to try, the likeliest first)
    "one-pass variance": (dict(variance="one-pass"), ("offset100",)),
    "unbiased variance": (dict(unbiased=True), ("plain", "gsign")),
    "no eps": (dict(eps=0.0), ("tinyvar", "constgroup")),
    "eps 1e-6": (dict(eps=1e-6), ("tinyvar", "constgroup")),
    "Mish n / (n + 2) unclamped": (dict(mish="unclamped"), ("bigaffine",)),
}


@pytest.mark.parametrize("variant", list(WRONG_FORWARD))
def test_wrong_forward_variant_is_caught(variant):
    kw, first = WRONG_FORWARD[variant]
    seen = {}
    for regime in first + tuple(r for r in rr.REGIMES if r not in first):
        missed, ratio = _forward_misses(make_block(**kw), regime)
        seen[regime] = ratio
        if missed:
            print(f"{variant}: caught under {regime} (ratio {ratio})")
            return
    pytest.fail(f"{variant}: no regime catches it {seen}")


def test_statistics_over_container_rows_are_caught_at_a_padded_horizon():
    """H = 48 in its 64-row container (24 in 32, 12 in 16, 6 in 8 on the inner levels): the `ok` form meets the bound there, the form that counts the
    zero rows behind the horizon does not"""
    for regime in ("plain", "offset100"):
        missed, ratio = _forward_misses(make_block(), regime, H=48)
        assert not missed, (regime, ratio)
    missed, ratio = _forward_misses(make_block(container=True), "plain", H=48)
    assert missed, ratio
    missed, ratio = _forward_misses(make_block(container=True), "plain", H=64)   # (no pad rows: the same arithmetic as `ok`)
    assert not missed, ratio


# ---------------------------------------------------------------------------------------------- gradients
GRAD_REGIMES = ("plain", "offset100", "tinyvar", "constgroup", "gsign", "bigaffine")


@pytest.mark.parametrize("regime", GRAD_REGIMES)
def test_ok_backward_meets_the_gradient_bound(regime):
    """float32 autograd of the hand restatement, and the hand-written Mish derivative (clamped at 20) and GroupNorm backward (all three terms, eps)"""
    for block in (make_block(), make_block(hand_backward=True)):
        missed, worst, zeros = _gradient_misses(block, regime)
        print(f"{regime}: worst ratio {worst:.3f}, zero-gradient tensors {zeros}")
        assert not missed, (regime, worst)
    if regime == "constgroup":
        assert zeros > 50   # everything in front of a zeroed convolution but the residual path
    if regime == "bigaffine":
        rr.assert_bigaffine_shares(_grad_ref(regime)["shares"])


WRONG_BACKWARD = {
    "mish_grad without the clamp at 20": (dict(mish_grad_clamp=False), ("bigaffine",)),
    "GroupNorm backward without vhat * mean(gm * vhat)": (dict(drop_vhat_term=True), ("plain", "gsign")),
    "GroupNorm backward with rstd of var without eps": (dict(bwd_eps=0.0), ("constgroup", "tinyvar")),
}


@pytest.mark.parametrize("variant", list(WRONG_BACKWARD))
def test_wrong_backward_variant_is_caught(variant):
    kw, first = WRONG_BACKWARD[variant]
    seen = {}
    for regime in first + tuple(r for r in GRAD_REGIMES if r not in first):
        missed, worst, _ = _gradient_misses(make_block(hand_backward=True, **kw), regime)
        seen[regime] = worst
        if missed:
            print(f"{variant}: caught under {regime} (worst ratio {worst})")
            return
    pytest.fail(f"{variant}: no regime catches it {seen}")
