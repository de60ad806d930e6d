"""mpdx_plan's tail run (csrc/inner_run.hpp, RunSeqTail): the tail of up level 0 - the three 128 -> 128 Conv1dBlocks ups.0.0.blocks.1,
ups.0.1.blocks.0, ups.0.1.blocks.1 and Upsample1d(128) - as one persistent launch next to the seven-layer run.  The arithmetic is the per-layer
kernels', so every comparison is torch.equal between the handle's settings (mpdx_unet_set_inner_run_parts) on the same handle and noise: seven + tail,
seven alone, nothing.  mpdx_unet_inner_run_layers counts the layers inside run launches (11 per pass, 7 with the tail off); mpdx_unet_inner_runs
keeps counting the seven-layer launches alone.  After every plan the handle's status word is 0 and the outputs are finite.  No test drives the give-up
path."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import synth_sd, t, DIM_MULTS, product_guide

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
H = 64
T, N0 = 4, 2          # T = 4 + 2 steps without noise: six passes, one launch of each run per pass
P = T + N0
B_MAX = 129
SEVEN, TAIL = 1, 2    # mpdx_unet_set_inner_run_parts bits
SETTINGS = [SEVEN | TAIL, SEVEN, 0]   # compared: tail on, tail off with seven on, everything off

_MODELS, _NOISE = {}, {}


def _model(D, T=T, opt=1, horizon=H, tag=""):
    key = (D, T, opt, horizon, tag)
    if key not in _MODELS:
        import mpd_public_amd as m
        from mpd_public_amd import synthetic as syn
        net = m.TemporalUnet(n_support_points=horizon, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
        sd = synth_sd(D, opt) if horizon == H else syn.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
        net.load_state_dict(sd, strict=True)
        dm = m.GaussianDiffusionModel(model=net.cuda().eval(), variance_schedule="cosine", n_diffusion_steps=T, predict_epsilon=True)
        _MODELS[key] = dm.cuda().eval()
    return _MODELS[key]


def _noise(D, B, steps=P, horizon=H):
    """[steps + 1, B, horizon, D]: the first B trajectories of ONE tensor per (D, horizon), made once"""
    key = (D, steps, horizon)
    if key not in _NOISE:
        _NOISE[key] = t(f"tail_noise_D{D}_S{steps}_H{horizon}", (steps + 1, B_MAX, horizon, D)).cuda()
    return _NOISE[key][:, :B].contiguous()


def _hc(D, horizon=H):
    return {0: t("tail_hc0", (D,), "uniform", 0.6).cuda(), horizon - 1: t("tail_hc1", (D,), "uniform", 0.6).cuda()}


def _plan(dm, parts, hc, B, horizon=H, seed=None, join=True, **kw):
    """(x, chain, seven-layer launches, layers inside run launches) of one fused plan with the runs `parts` selected"""
    dm.model.set_inner_run_parts(parts)
    dm.model.set_plan_join(join)
    if seed is not None:
        dm.in_kernel_noise_min_bytes = 0
        dm.manual_seed(seed)
        dm._rng_offset = 5
    x, chain = dm.plan(hc, B, horizon, noise_std_extra_schedule_fn=lambda tt: 0.5, **kw)
    torch.cuda.synchronize()
    assert dm.model.status() == 0
    assert torch.isfinite(x).all() and (chain is None or torch.isfinite(chain).all())
    return x, chain, dm.model.inner_runs(), dm.model.inner_run_layers()


def _counts(parts, passes, selected=True):
    """(mpdx_unet_inner_runs, mpdx_unet_inner_run_layers) a plan of `passes` passes promises"""
    if not selected:
        return 0, 0
    return (passes if parts & SEVEN else 0), passes * ((7 if parts & SEVEN else 0) + (4 if parts & TAIL else 0))


def _settings_agree(dm, hc, B, selected=True, horizon=H, passes=P, settings=SETTINGS, **kw):
    got = [_plan(dm, parts, hc, B, horizon, **kw) for parts in settings]
    for parts, (x, chain, nr, nl) in zip(settings, got):
        assert (nr, nl) == _counts(parts, passes, selected), (parts, nr, nl)
        assert torch.equal(x, got[-1][0]), parts
        assert (chain is None) == (got[-1][1] is None) and (chain is None or torch.equal(chain, got[-1][1])), parts
    return got[0][0], got[0][1]


@pytest.mark.parametrize("in_kernel_noise", [False, True])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 8, 100, 128, 129])
@pytest.mark.parametrize("D", [4, 14])
def test_tail_run_equals_per_layer_kernels(D, B, in_kernel_noise):
    """B = 1, 3: one partly filled cluster of 8 workgroups; 4: a full one; 5: a ragged second tile; 8; 100: the headline's 25 clusters; 128: the largest
    batch that is selected (one workgroup per compute unit); 129: not selected.  With and without the chain, with plan-join on and off."""
    dm = _model(D)
    for return_chain in (True, False):
        for join in (True, False):
            kw = dict(n_diffusion_steps_without_noise=N0, return_chain=return_chain, join=join)
            if in_kernel_noise:
                kw["seed"] = 4321
            else:
                kw["noise"] = _noise(D, B)
            x, chain = _settings_agree(dm, _hc(D), B, selected=B <= 128, **kw)
            assert float(x.std()) > 0.05
            if chain is not None:
                assert torch.equal(x, chain[-1]) and not torch.equal(chain[1], chain[2])


def test_set_inner_run_selects_everything_and_the_tail_stands_alone():
    """set_inner_run(True) is seven + tail, (False) nothing; the tail alone (4 layers per pass, no seven-layer launch) gives the same bits."""
    D, B = 4, 5
    dm = _model(D)
    kw = dict(n_diffusion_steps_without_noise=N0, noise=_noise(D, B))
    xr, cr, nr, nl = _plan(dm, 0, _hc(D), B, **kw)
    assert (nr, nl) == (0, 0)
    for on, want in ((True, (P, 11 * P)), (False, (0, 0))):
        dm.model.set_inner_run(on)
        x, chain = dm.plan(_hc(D), B, H, noise_std_extra_schedule_fn=lambda tt: 0.5, **kw)
        torch.cuda.synchronize()
        assert dm.model.status() == 0 and (dm.model.inner_runs(), dm.model.inner_run_layers()) == want
        assert torch.equal(x, xr) and torch.equal(chain, cr)
    x, chain, nr, nl = _plan(dm, TAIL, _hc(D), B, **kw)
    assert (nr, nl) == (0, 4 * P)
    assert torch.equal(x, xr) and torch.equal(chain, cr)
    from mpd_public_amd import _lib
    assert _lib.load().mpdx_unet_set_inner_run_parts(dm.model._handle(), 4) < 0   # an unknown part
    dm.model.set_inner_run(True)


def test_plans_back_to_back_and_two_handles_alternating():
    """The two runs share the handle's counters (the base advances by 8 x layers with every launch of either kind) and the counters belong to the
    handle: plans in a row on one handle, and two handles taking turns on one stream, give what the per-layer kernels give."""
    D, B = 4, 8
    a, b = _model(D), _model(D, tag="second")
    assert a.model._handle().value != b.model._handle().value
    kw = dict(n_diffusion_steps_without_noise=N0, noise=_noise(D, B))
    for dm in (a, b):
        dm.model.set_inner_run(True)
        dm.model.set_plan_join(True)
    got = []
    for dm in (a, a, a, b, a, b, a):
        x, chain = dm.plan(_hc(D), B, H, noise_std_extra_schedule_fn=lambda tt: 0.5, **kw)
        assert (dm.model.inner_runs(), dm.model.inner_run_layers()) == (P, 11 * P)
        got.append((x, chain))
    torch.cuda.synchronize()
    assert a.model.status() == 0 and b.model.status() == 0
    xr, cr, nr, nl = _plan(a, 0, _hc(D), B, **kw)
    assert (nr, nl) == (0, 0)
    for x, chain in got:
        assert torch.equal(x, xr) and torch.equal(chain, cr)


def test_batch_that_grows_and_shrinks_between_plans():
    """A launch advances the counters of its own clusters only: a handle whose batch shrinks and grows again (more clusters than the launch before)
    still starts every run of either kind from counters that agree."""
    D = 4
    dm = _model(D, tag="resize")
    for B in (8, 4, 12, 4, 100, 1, 128):
        _settings_agree(dm, _hc(D), B, n_diffusion_steps_without_noise=N0, noise=_noise(D, B))


def test_guided_panda_plan_uses_both_runs():
    """B = 4 in two contexts, T = 4 + 2, guide from t < 2: the inner levels do not see the guide, so guided iterations take both runs."""
    import mpd_public_amd as m
    D, B, npc = 14, 4, 2
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args={"device": "cuda", "dtype": torch.float32})
    dm = _model(D)
    hc = {0: t("tail_ctx_hc0", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0),
          H - 1: t("tail_ctx_hc1", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0)}
    kw = dict(n_diffusion_steps_without_noise=N0, noise=_noise(D, B), guide=product_guide(ds).cuda(), n_guide_steps=2, t_start_guide=2, n_per_context=npc)
    got = []
    for parts in SETTINGS:
        x, chain, nr, nl = _plan(dm, parts, hc, B, **kw)
        assert (nr, nl) == _counts(parts, P), (parts, nr, nl)
        got.append((x, chain, dm.last_guide_flags.clone()))
    assert not torch.equal(got[0][1][-1], got[0][1][-2])
    for x, chain, flags in got[:-1]:
        assert torch.equal(x, got[-1][0]) and torch.equal(chain, got[-1][1]) and torch.equal(flags, got[-1][2])


@pytest.mark.parametrize("opt,horizon", [(0, 64), (1, 48)])
def test_networks_without_the_sequences_plan_as_before(opt, horizon):
    """A three-level network (no level on 8 positions) and a horizon in a zero-padded container: no run of either kind, outputs as before."""
    D, B = 4, 3
    dm = _model(D, T, opt, horizon)
    kw = dict(n_diffusion_steps_without_noise=N0, noise=_noise(D, B, horizon=horizon))
    _settings_agree(dm, _hc(D, horizon), B, False, horizon, **kw)


_PAIR_OFF_CODE = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import test_gpu_inner_run_tail as M
D, B = 4, 5
dm = M._model(D)
kw = dict(n_diffusion_steps_without_noise=M.N0, noise=M._noise(D, B))
M._settings_agree(dm, M._hc(D), B, **kw)
M._settings_agree(dm, M._hc(D), B, join=False, **kw)
print("pairs-off ok")
"""


def test_pairs_off_in_a_process_of_its_own():
    """MPDX_PAIR=0 (read once per process): blocks[0] and the residual 1x1 conv of a block are two launches; both runs are still found and the plan
    still equals the all-off plan."""
    code = _PAIR_OFF_CODE.format(root=str(ROOT), tests=str(ROOT / "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), env={**os.environ, "MPDX_PAIR": "0"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pairs-off ok" in r.stdout, r.stderr[-3000:]


def test_tail_run_chain_vs_oracle():
    """T = 3 + 1, B = 2 against the CPU oracle at the tolerances of test_run_chain_vs_oracle (2e-3 over the chain, 5e-4 on the result: fp32
    summation order, amplified by the x0 estimate at large t)."""
    from oracle import diffusion as odiff
    D, To, B, n0 = 4, 3, 2, 1
    dm = _model(D, To)
    noise = t("tail_noise_oracle", (To + n0 + 1, B, H, D))
    hc = {0: t("tail_hc0", (D,), "uniform", 0.6), H - 1: t("tail_hc1", (D,), "uniform", 0.6)}
    x, chain, nr, nl = _plan(dm, SEVEN | TAIL, {k: v.cuda() for k, v in hc.items()}, B, n_diffusion_steps_without_noise=n0, noise=noise.cuda())
    assert (nr, nl) == _counts(SEVEN | TAIL, To + n0)
    nthr = torch.get_num_threads()
    torch.set_num_threads(1)   # (the oracle's fp32 chain moves with the host's thread count: one thread pins it)
    try:
        ref = odiff.run_inference(synth_sd(D, 1), hc, noise, To, variance_schedule="cosine", n_diffusion_steps_without_noise=n0, noise_std=0.5).numpy()
    finally:
        torch.set_num_threads(nthr)
    got = chain.cpu().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
    print("max |chain - oracle| per row:", err)
    assert err.max() < 2e-3, err
    assert err[-1] < 5e-4, err
