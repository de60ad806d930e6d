"""The U-Net shapes mpdx_unet_create admits besides the two shipped networks, as one case table: tests/test_gpu_unet_shapes.py runs every row on the
GPU against the float64 oracle, tests/test_unet_shapes_cpu.py pins what the library builds for it (parameter table, fused programs, refusals).

A row is (name, H, unet_input_dim, dim_mults, D).  Weights are synthetic.synth_state_dict of oracle.unet.unet_param_shapes, inputs helpers.t, the
reference regime_ref.forward_ref / grads_ref with regime_ref's bounds.  What a row reaches:

  two, two-h32        generic segment + static program 2; at H = 32 every layer its own launch
  jump                32 -> 256 in one level; ups.0.0 is 512 -> 32 (the widest K onto the narrowest M)
  rep-first           identity residual on the first block of a level (downs.1.0 is 32 -> 32); D = 7: padded input channels
  rep-last, -h48      static programs 0 and 2 around a generic segment in a foreign network; at H = 48 the masked container
  four-128            programs 5 + 3, the joined launch, its paired form, the tail run; no seven-layer run; conv_wsn at B = 513
  four-256            the seven-layer run on a window that starts at downs.3.0.blocks.0 (a time-bias layer); conv_ws on nine layers at B = 513
  five, five-h128     4 positions at the coarsest level; the joined launch with n_levels == 5; at H = 128 every layer its own launch
  six                 three generic segments; 4 positions at the coarsest level
  wide-128, wide-64   256-channel rows on 64 positions

REFUSED rows are not created: (1,2,1) and (1,4,2) give ups.0.0 an identity residual over its concatenated input, which no kernel reads (a layer names
one residual slot of C_out channels); the others fail the GroupNorm-region rule of mpdx_unet_create."""
import torch

from helpers import t
from mpd_public_amd import synthetic as syn
from oracle.unet import unet_param_shapes

# (name, H, unet_input_dim, dim_mults, D)
CASES = (
    ("two", 64, 32, (1, 2), 4),
    ("two-h32", 32, 32, (1, 2), 4),
    ("jump", 64, 32, (1, 8), 4),
    ("rep-first", 64, 32, (1, 1, 2), 7),
    ("rep-last", 64, 32, (1, 2, 2), 4),
    ("rep-last-h48", 48, 32, (1, 2, 2), 4),
    ("four-128", 64, 32, (1, 2, 4, 4), 4),
    ("four-256", 64, 32, (1, 2, 8, 8), 4),
    ("five", 64, 32, (1, 2, 4, 8, 8), 4),
    ("five-h128", 128, 32, (1, 2, 4, 8, 8), 4),
    ("six", 128, 32, (1, 1, 2, 2, 4, 8), 4),
    ("wide-128", 64, 128, (1, 2), 4),
    ("wide-64", 64, 64, (1, 2, 2), 4),
)
# refused by the library (REFUSED below); the oracle and the reference run them: tests/golden/unet_shapes.npz, tests/test_unet_shapes_cpu.py
ORACLE_ONLY = (
    ("halving-121", 64, 32, (1, 2, 1), 4),
    ("halving-142", 64, 32, (1, 4, 2), 4),
)
ROWS = {c[0]: c for c in CASES + ORACLE_ONLY}
GOLDEN_ROWS = ("two", "rep-first", "rep-last", "halving-121", "halving-142", "five")   # make_golden.py --only unet_shapes: B = 2, t = 0 and 37
GOLDEN_T = (0, 37)

# mpdx_unet_fused_program per segment, in order ([]: no segment, every layer its own launch; -1: the generic op-list kernel)
PROGRAMS = {
    "two": [-1, 2], "two-h32": [], "jump": [-1], "rep-first": [-1], "rep-last": [0, -1, 2], "rep-last-h48": [], "four-128": [5, 3], "four-256": [0, 2],
    "five": [5, 3], "five-h128": [], "six": [-1, -1, -1], "wide-128": [], "wide-64": [-1],
}

# (H, unet_input_dim, dim_mults, the layer or words the message names)
REFUSED = (
    (64, 32, (1, 2, 1), "ups.0.0"), (64, 32, (1, 4, 2), "ups.0.0"), (64, 32, (1, 2, 4, 2), "ups.0.0"), (64, 32, (1, 2, 1, 2), "ups.1.0"),
    (16, 32, (1, 2), "GroupNorm region"), (16, 32, (1, 2, 4, 8), "GroupNorm region"), (64, 32, (1, 3), "GroupNorm region"), (64, 32, (1, 16), "GroupNorm region"),
    (64, 16, (1, 2), "GroupNorm region"), (128, 32, (1, 1, 1, 1, 1, 1, 1), "GroupNorm region"),
)

T_FWD = 37
_SD, _X = {}, {}


def state_dict(name):
    """the row's synthetic weights (one dict per row; callers do not write to it)"""
    if name not in _SD:
        _, H, W, mults, D = ROWS[name]
        _SD[name] = syn.synth_state_dict(unet_param_shapes(D, W, mults))
    return _SD[name]


def x_in(name, n=5):
    """the first n trajectories of ONE input tensor per row"""
    if name not in _X:
        _, H, W, mults, D = ROWS[name]
        _X[name] = t(f"shapes_x_{name}", (513, H, D))
    return _X[name][:n].contiguous()


def tvec(n, tv=T_FWD):
    return torch.full((n,), tv, dtype=torch.long)
