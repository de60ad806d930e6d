"""Block-level cases of the linear self-attention launch (csrc/attn.hpp through mpdx_attention_block): shapes taken from the kernel's branch points,
formula-defined input regimes, the fp64 reference (oracle.unet.linear_attention_block on the valid positions) and the error bound derived from it.
Shared by tests/test_gpu_attention_block.py (the kernel) and tests/test_oracle_attention_cpu.py (the cases can tell wrong variants apart)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from helpers import t
from mpd_public_amd import synthetic as syn
from oracle import unet as ounet

# (C, L, Lv) -> batch sizes; what each shape reaches in attn_kernel (G = trajectories per workgroup = attn_cols(C, L) / L)
SHAPES = {
    (32, 64, 64): (1, 3),          # G = 1, 8-tile accumulator
    (256, 64, 64): (2,),           # 16-tile accumulator (attn_kernel<16>)
    (128, 128, 128): (2,),
    (32, 128, 128): (3,),          # two softmax elements per lane
    (64, 128, 96): (3,),
    (32, 128, 80): (3,),
    (256, 8, 8): (1, 4, 5, 7),     # G = 4, last group partial
    (64, 16, 16): (6,),            # G = 4
    (32, 2, 2): (1, 32, 33),       # G = 32, two lanes per softmax row
    (64, 32, 24): (3, 5),          # padded containers: Lv not a multiple of 16 / of 4 / odd
    (64, 16, 12): (3, 5),
    (128, 8, 6): (3, 5),
    (256, 8, 5): (3, 5),
    (32, 64, 40): (3, 5),
    (512, 8, 8): (3,),             # LayerNorm with two float4 per lane
    (512, 16, 16): (3,),
    (512, 8, 6): (3,),
}
REFUSED = ((256, 128, 128), (48, 64, 64), (32, 24, 24), (1024, 8, 8))
REGIMES = ("plain", "mean100", "tinyvar", "constrow", "sharp64", "sharp128", "gsign", "big")
# the shapes every regime other than `plain` runs on: one per row of the table above at least
REGIME_SHAPES = ((32, 64, 64), (256, 64, 64), (64, 128, 96), (256, 8, 8), (32, 2, 2), (64, 16, 12), (256, 8, 5), (32, 64, 40), (512, 8, 6))
CASES = [(s, "plain") for s in SHAPES] + [(s, r) for r in REGIMES[1:] for s in REGIME_SHAPES]

# max|gpu - fp64| <= K * max|fp32 restatement - fp64| + 2^-23 max|y|.  K covers the summation orders the kernel and torch differ in (MFMA chains of
# 4 against torch's blocked sums, a butterfly softmax reduction); fixed at twice the largest ratio max|gpu - fp64| / e_ref measured on the MI355X
# (1.65, `sharp64` at 256 channels on 8 positions), rounded up (DESIGN.md section 6 lists the ratios)
K = 4
P = "blk"   # state-dict prefix of the block's parameters


def case_id(case):
    (C, L, Lv), regime = case
    return f"C{C}_L{L}_Lv{Lv}_{regime}"


@functools.lru_cache(maxsize=None)
def block_params(C, regime):
    """fp32 state dict of one block at synthetic scale (to_qkv ~ U(+-1/sqrt(C)), to_out ~ U(+-1/sqrt(128)), g ~ 1, b ~ 0), then the regime's change"""
    shapes = {f"{P}.fn.fn.to_qkv.weight": (384, C, 1), f"{P}.fn.fn.to_out.weight": (C, 128, 1), f"{P}.fn.fn.to_out.bias": (C,),
              f"{P}.fn.norm.g": (1, C, 1), f"{P}.fn.norm.b": (1, C, 1)}
    sd = {k: torch.from_numpy(syn.synth_param(f"attnblk/C{C}/{k}", s).copy()) for k, s in shapes.items()}
    w = sd[f"{P}.fn.fn.to_qkv.weight"]
    if regime in ("sharp64", "sharp128"):     # peaked softmax: the k rows
        w[128:256] *= float(regime[5:])
    elif regime == "big":                     # q and v rows
        w[0:128] *= 16.0
        w[256:384] *= 16.0
    elif regime == "gsign":                   # negative and exactly-zero scales, shifts of O(1)
        g = 1.5 * t(f"attnblk/C{C}/gsign_g", (1, C, 1), "uniform")
        g[:, ::5] = 0.0
        sd[f"{P}.fn.norm.g"] = g
        sd[f"{P}.fn.norm.b"] = t(f"attnblk/C{C}/gsign_b", (1, C, 1), "uniform")
    return sd


@functools.lru_cache(maxsize=None)
def trajectory(C, L, Lv, regime, b):
    """input of trajectory b, [C, Lv] fp32; it does not depend on the batch it is put in"""
    x = t(f"attnblk/x/C{C}_L{L}_Lv{Lv}/{b}", (Lv, C)).T.contiguous()
    if regime == "mean100":
        x = x + 100.0
    elif regime == "tinyvar":
        x = x * 1e-3
    elif regime == "constrow":                # every other position exactly constant over the channels (values that sum exactly in any order), one of them zero
        for n in range(0, Lv, 2):
            x[:, n] = 0.25 * ((n // 2 + b) % 9 - 4)
    return x


def block_input(shape, regime, bs):
    """[len(bs), C, Lv] fp32: the trajectories `bs`"""
    C, L, Lv = shape
    return torch.stack([trajectory(C, L, Lv, regime, b) for b in bs])


def to_dtype(sd, dt):
    return {k: v.to(dt) for k, v in sd.items()}


# ------------------------------------------------------------------------------------ the restatement with one deliberate mistake (variant != None)
VARIANTS = ("softmax_no_max", "var_one_pass", "var_unbiased", "no_eps", "all_positions", "no_q_scale", "heads_ch")


def block_variant(sd, x, L, variant=None):
    """oracle.unet.linear_attention_block(sd, P, x) for x [B,C,Lv] (variant None: the same operations, bit for bit), or one wrong variant of it"""
    B, C, Lv = x.shape
    g, b = sd[f"{P}.fn.norm.g"], sd[f"{P}.fn.norm.b"]
    x_in = x
    if variant == "all_positions":            # the zero pad rows of the container take part in the softmax and the context
        x = F.pad(x, (0, L - Lv))
    n = x.shape[-1]
    mean = torch.mean(x, dim=1, keepdim=True)
    if variant == "var_one_pass":
        var = torch.mean(x * x, dim=1, keepdim=True) - mean * mean
    else:
        var = torch.var(x, dim=1, unbiased=variant == "var_unbiased", keepdim=True)
    xn = (x - mean) / (var + (0.0 if variant == "no_eps" else 1e-5)).sqrt() * g + b
    qkv = F.conv1d(xn, sd[f"{P}.fn.fn.to_qkv.weight"])
    if variant == "heads_ch":                 # '(c h)' instead of '(h c)'
        q, k, v = (a.reshape(B, 32, 4, n).transpose(1, 2) for a in qkv.chunk(3, dim=1))
    else:
        q, k, v = (a.reshape(B, 4, 32, n) for a in qkv.chunk(3, dim=1))
    if variant != "no_q_scale":
        q = q * 32 ** -0.5
    if variant == "softmax_no_max":
        e = k.exp()
        k = e / e.sum(-1, keepdim=True)
    else:
        k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q)
    out = (out.transpose(1, 2) if variant == "heads_ch" else out).reshape(B, 128, n)
    y = F.conv1d(out, sd[f"{P}.fn.fn.to_out.weight"], sd[f"{P}.fn.fn.to_out.bias"])[..., :Lv]
    return y + x_in


def reference(shape, regime, bs):
    """(y64 [B,C,Lv] fp64, e_ref, bound): the fp64 oracle of the trajectories `bs`, e_ref = max|the SAME restatement run in fp32 on the CPU - y64|, and
    the largest max|result - y64| a correct fp32 evaluation may show: K e_ref plus one fp32 rounding of the largest output"""
    sd, x = block_params(shape[0], regime), block_input(shape, regime, tuple(bs))
    y64 = ounet.linear_attention_block(to_dtype(sd, torch.float64), P, x.double())
    y32 = ounet.linear_attention_block(sd, P, x)
    e_ref = float((y32.double() - y64).abs().max())
    return y64, e_ref, K * e_ref + 2.0 ** -23 * float(y64.abs().max())


# ------------------------------------------------------------------------------------ the kernel
def run_block_gpu_raw(xc, sd, L, Lv, C):
    """mpdx_attention_block in place on the device tensor xc [B, L, C] with the (CPU, fp32) parameters sd; raises what the library refuses"""
    from mpd_public_amd import _lib
    dev = [sd[f"{P}.fn.{k}"].cuda().contiguous() for k in ("fn.to_qkv.weight", "fn.to_out.weight", "fn.to_out.bias", "norm.g", "norm.b")]
    _lib.check(_lib.load().mpdx_attention_block(_lib.ptr(xc), *(_lib.ptr(d) for d in dev), xc.shape[0], L, Lv, C, _lib.current_stream()),
               "mpdx_attention_block")


def run_block_gpu(shape, regime, bs):
    """mpdx_attention_block on the trajectories `bs` -> the whole container [B, L, C] (CPU tensor)"""
    C, L, Lv = shape
    xc = torch.zeros((len(bs), L, C))
    xc[:, :Lv, :] = block_input(shape, regime, tuple(bs)).transpose(1, 2)
    xc = xc.cuda().contiguous()
    run_block_gpu_raw(xc, block_params(C, regime), L, Lv, C)
    return xc.cpu()
