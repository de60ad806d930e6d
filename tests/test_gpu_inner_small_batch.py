"""The per-layer conv kernels of the inner U-Net levels (L = 8; csrc/conv_block.hpp GeoL8 / GeoUp8, conv_pair_kernel) at small batch: ragged
last tiles (clamped rows), full tiles next to a ragged one, the tiles of the headline batch, and the same kernels above one workgroup per CU.
Whatever is done to their staging, barriers or epilogue loads, no summation order may change: every bit-identity the other paths are held to
(batch independence, the weight-stationary kernels, the two forms of a plan) is asserted here on the smallest batches that reach those tiles.
Four-level network, H = 64."""
import os

import numpy as np
import pytest
import torch

from helpers import synth_sd, t, DIM_MULTS

pytestmark = pytest.mark.gpu

OPT = 1   # dim_mults (1, 2, 4, 8)


def _net(D, T=None, schedule="exponential"):
    import mpd_public_amd as m
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[OPT])
    net.load_state_dict(synth_sd(D, OPT), strict=True)
    net = net.cuda().eval()
    if T is None:
        return net
    return m.GaussianDiffusionModel(model=net, variance_schedule=schedule, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()


@pytest.fixture(scope="module")
def oracle_rows():
    """the CPU oracle on the 9 seeded trajectories of a (D, timestep) case, computed once (GroupNorm is per sample: a slice of the
    rows is the oracle of that slice)"""
    from oracle.unet import unet_forward
    cache = {}

    def get(D, tt):
        if (D, tt) not in cache:
            x = t(f"inner_small_x_D{D}", (9, 64, D))
            cache[(D, tt)] = (x, unet_forward(synth_sd(D, OPT), x, torch.full((9,), tt, dtype=torch.long)).numpy())
        return cache[(D, tt)]
    return get


@pytest.mark.parametrize("tt", [0, 41])
@pytest.mark.parametrize("D", [4, 14])
def test_small_batches_vs_oracle_and_row_independence(oracle_rows, D, tt):
    """B in {1, 4, 5, 9}: ragged last tiles (clamped rows in the staging and the epilogue), B = 9: full tiles plus a ragged one.
    Each output is within 2e-5 of the oracle (the U-Net tolerance of test_gpu_parity.py: 33 conv blocks of fp32 MFMA against MKL-DNN's
    summation order, |eps| ~ 0.3), and a trajectory's bits do not depend on the batch it sits in."""
    x, ref = oracle_rows(D, tt)
    net = _net(D)

    def run(sl):
        n = sl.stop - sl.start
        return net(x[sl].contiguous().cuda(), torch.full((n,), tt, dtype=torch.long, device="cuda"), None)
    full = run(slice(0, 9))
    assert bool(torch.isfinite(full).all())
    err = float(np.abs(full.cpu().numpy() - ref).max())
    print(f"D={D} t={tt} B=9 max|y - oracle| = {err:.3e}")
    assert err <= 2e-5
    for sl in (slice(0, 4), slice(3, 8)):   # B = 4 (rows 0 .. 3), B = 5 (rows 3 .. 7)
        part = run(sl)
        err = float(np.abs(part.cpu().numpy() - ref[sl]).max())
        print(f"D={D} t={tt} B={sl.stop - sl.start} max|y - oracle| = {err:.3e}")
        assert err <= 2e-5
        assert torch.equal(part, full[sl])
    for i in range(9):                      # B = 1, every row
        one = run(slice(i, i + 1))
        if i == 0:
            err = float(np.abs(one.cpu().numpy() - ref[:1]).max())
            print(f"D={D} t={tt} B=1 max|y - oracle| = {err:.3e}")
            assert err <= 2e-5
        assert torch.equal(one, full[i:i + 1]), i


def test_headline_tiles_with_a_ragged_last_tile_vs_oracle():
    """B = 99: the tiles of the headline batch (B = 100: [32x32] for 256 -> 256, [16x32] for 128 -> 128, at most one workgroup per CU) with a
    last tile of three trajectories instead of four; rows 96 .. 98 equal their own B = 3 run."""
    from oracle.unet import unet_forward
    D, tt, B = 4, 41, 99
    x = t("inner_small_x_B99", (B, 64, D))
    ref = unet_forward(synth_sd(D, OPT), x, torch.full((B,), tt, dtype=torch.long)).numpy()
    net = _net(D)
    y = net(x.cuda(), torch.full((B,), tt, dtype=torch.long, device="cuda"), None)
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f"B=99 max|y - oracle| = {err:.3e}")
    assert err <= 2e-5
    tail = net(x[96:].contiguous().cuda(), torch.full((3,), tt, dtype=torch.long, device="cuda"), None)
    assert torch.equal(tail, y[96:])


def test_per_layer_kernels_above_one_workgroup_per_cu_equal_weight_stationary():
    """B = 513: the per-layer kernels (MPDX_WS=0) with more workgroups than CUs against the weight-stationary kernels (MPDX_WS=1), which keep
    the same chains and orders: bit-identical outputs."""
    B, D = 513, 14
    net = _net(D)
    x = t("inner_small_ws_x", (B, 64, D)).cuda()
    tt = torch.full((B,), 41, dtype=torch.long, device="cuda")
    old = os.environ.get("MPDX_WS")
    try:
        os.environ["MPDX_WS"] = "1"
        y_ws = net(x, tt, None)
        os.environ["MPDX_WS"] = "0"
        y_pl = net(x, tt, None)
    finally:
        if old is None:
            os.environ.pop("MPDX_WS", None)
        else:
            os.environ["MPDX_WS"] = old
    assert bool(torch.isfinite(y_ws).all()) and float(y_ws.abs().max()) > 1e-3
    assert torch.equal(y_ws, y_pl)


def test_unguided_plan_both_forms_are_bit_identical():
    """T = 3 (+1) at B = 5: the whole plan as one mpdx_plan call (fused=True) and step by step through ddpm_sample_fn (fused=False) run the
    same kernels on the same injected noise: equal chains.  (Cosine schedule: the exponential one has no finite betas for 3 steps.)"""
    import mpd_public_amd as m
    D, T, B, n0 = 4, 3, 5, 1
    dm = _net(D, T, "cosine")
    noise = t("inner_small_plan_noise", (T + n0 + 1, B, 64, D)).cuda()
    hc = {0: t("inner_small_hc0", (D,), "uniform", 0.6).cuda(), 63: t("inner_small_hc1", (D,), "uniform", 0.6).cuda()}
    chains = [dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, n_diffusion_steps_without_noise=n0,
                               noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise, fused=fused) for fused in (True, False)]
    assert chains[0].shape == (T + n0 + 1, B, 64, D)
    assert bool(torch.isfinite(chains[0]).all())
    assert torch.equal(chains[0], chains[1])
