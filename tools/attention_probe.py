#!/usr/bin/env python3
"""Timing of the self-attention launches inside the U-Net pass (development tool; needs a GPU):  python tools/attention_probe.py [out.md]

H = 64, D = 4, dim_mults (1,2,4,8), B = 100 and B = 6400, one process.  Per attention launch: microseconds (median of REPS mpdx_unet_profile
passes, event pair per launch), algorithmic FLOPs and the fraction of the fp32 MFMA peak, next to the same pass's figure for the level's
`.1.blocks.1` convolution launch (the launch right before the block).  The whole pass with and without attention on the per-layer path
(MPDX_FUSED=0 for the plain network too, so both run the same convolution launches): mpdx_unet_time_units over all units, one event pair per pass.
Also lists the launches of the DEFAULT network on its default path."""
import ctypes as C
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]
import torch  # noqa: E402
import mpd_public_amd as m  # noqa: E402
from mpd_public_amd import _lib, synthetic as syn  # noqa: E402

PEAK = 157.3e12   # fp32 MFMA peak, FLOP/s
REPS, H, D, MULTS, T = 15, 64, 4, (1, 2, 4, 8), 100
lib = _lib.load()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def net(self_attention):
    n = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=32, dim_mults=MULTS, self_attention=self_attention)
    n.load_state_dict(syn.synth_state_dict({k: tuple(v.shape) for k, v in n.state_dict().items()}), strict=True)
    return n.cuda().eval()


def profile(n, B, x):
    hdl, packed, tab, ws = n.engine(T, B)
    cap = 160
    ms, fl, names, cnt = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_char_p * cap)(), C.c_int()
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(3 + REPS):
        _lib.check(lib.mpdx_unet_profile(hdl, packed.data_ptr(), tab.data_ptr(), n._timetab_T, x.data_ptr(), 50, B, ws.data_ptr(), st, cap, ms, fl, names, C.byref(cnt)))
        runs.append([ms[i] * 1e3 for i in range(cnt.value)])
    us = [statistics.median(r[i] for r in runs[3:]) for i in range(cnt.value)]
    nm = [names[i].decode() for i in range(cnt.value)]
    n_units = cnt.value - (1 if nm[-1].startswith("final_conv.1") else 0)
    out = C.c_float()
    _lib.check(lib.mpdx_unet_time_units(hdl, packed.data_ptr(), tab.data_ptr(), n._timetab_T, x.data_ptr(), 50, B, ws.data_ptr(), st, 0, n_units - 1, 30, C.byref(out)))
    return nm, us, [fl[i] for i in range(cnt.value)], out.value * 1e3


say("# Self-attention launches inside the U-Net pass (tools/attention_probe.py)")
say()
say(f"H = {H}, D = {D}, dim_mults {MULTS}, t = 50; per launch: median of {REPS} `mpdx_unet_profile` passes (event pair per launch, so each figure carries the ~5 us an event pair "
    "adds next to a short launch); pass: `mpdx_unet_time_units` over all units, 30 passes, one event pair per pass.  Peak = 157.3 TFLOP/s (fp32 MFMA).")
for B in (100, 6400):
    x = torch.randn(B, H, D, device="cuda", generator=torch.Generator("cuda").manual_seed(B))
    os.environ["MPDX_FUSED"] = "0"
    na, ua, fa, pass_a = profile(net(True), B, x)
    npl, upl, fpl, pass_p = profile(net(False), B, x)
    os.environ.pop("MPDX_FUSED")
    say()
    say(f"## B = {B}")
    say()
    say("| attention launch | MFLOP per trajectory | us | MFLOP | % of peak | the level's `.1.blocks.1` conv: us | MFLOP | % of peak | attention / conv peak fraction |")
    say("|---|---|---|---|---|---|---|---|---|")
    below = []
    for i, name in enumerate(na):
        if ".fn.fn.to_qkv" not in name:
            continue
        j = i - 1
        assert na[j].endswith(".blocks.1.block.0.weight"), na[j]
        fr_a, fr_c = fa[i] / (ua[i] * 1e-6) / PEAK, fa[j] / (ua[j] * 1e-6) / PEAK
        say(f"| `{name.replace('.fn.fn.to_qkv.weight', '')}` | {fa[i] / B / 1e6:.3f} | {ua[i]:.1f} | {fa[i] / 1e6:.1f} | {100 * fr_a:.1f} | {ua[j]:.1f} | {fa[j] / 1e6:.1f} | {100 * fr_c:.1f} | {fr_a / fr_c:.2f} |")
        if fr_a < 0.5 * fr_c:
            below.append(name.replace(".fn.fn.to_qkv.weight", ""))
    say()
    say(f"Whole pass, per-layer path: with attention {pass_a:.1f} us ({len(na)} launches), plain network {pass_p:.1f} us ({len(npl)} launches): +{pass_a - pass_p:.1f} us = +{100 * (pass_a / pass_p - 1):.1f} % "
        f"for +{100 * (sum(fa) / sum(fpl) - 1):.1f} % algorithmic FLOPs.  Sum of the attention launches' own figures: {sum(u for n_, u in zip(na, ua) if '.fn.fn.' in n_):.1f} us.")
    say(f"Attention launches below half the peak fraction of their level's conv: {', '.join(below) if below else 'none'}.")
    same = [n_ for n_ in na if ".fn.fn." not in n_] == npl
    say(f"The attention network's other launches are the plain per-layer network's launches, in order: {same}.")
    if B == 100:
        nd, ud, fd, pass_d = profile(net(False), B, x)
        say()
        say(f"Default network on its default path at B = {B} ({pass_d:.1f} us per pass): " + "; ".join(f"`{n_}`" for n_ in nd))

if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text("\n".join(lines) + "\n")
