"""mpdx_plan's inner-level run (csrc/inner_run.hpp): the seven consecutive 256 -> 256 Conv1dBlocks of the innermost level as one persistent launch
whose workgroups hand their tiles to each other inside the launch.  The arithmetic is the per-layer kernels', so every comparison here is
torch.equal between the handle option (mpdx_unet_set_inner_run) on and off, on the same handle and noise; the oracle test uses the tolerances of
test_joined_chain_vs_oracle.  After every plan the handle's status word is 0 and the outputs are finite.  No test drives the give-up path."""
import numpy as np
import pytest
import torch

from helpers import synth_sd, t, DIM_MULTS, product_guide

pytestmark = pytest.mark.gpu

H = 64
T, N0 = 4, 2          # T = 4 + 2 steps without noise: six passes, one run each
B_MAX = 129

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


def _noise(D, B, steps=T + N0, horizon=H):
    """[steps + 1, B, horizon, D]: the first B trajectories of ONE tensor per (D, horizon), made once"""
    key = (D, steps, horizon)
    if key not in _NOISE:
        _NOISE[key] = t(f"run_noise_D{D}_S{steps}_H{horizon}", (steps + 1, B_MAX, horizon, D)).cuda()
    return _NOISE[key][:, :B].contiguous()


def _hc(D, horizon=H):
    return {0: t("run_hc0", (D,), "uniform", 0.6).cuda(), horizon - 1: t("run_hc1", (D,), "uniform", 0.6).cuda()}


def _plan(dm, run, hc, B, horizon=H, seed=None, join=True, **kw):
    """(x, chain, run launches) of one fused plan with the inner-run option set to `run`"""
    dm.model.set_inner_run(run)
    dm.model.set_plan_join(join)
    if seed is not None:
        dm.in_kernel_noise_min_bytes = 0
        dm.manual_seed(seed)
        dm._rng_offset = 5
    x, chain = dm.plan(hc, B, horizon, noise_std_extra_schedule_fn=lambda tt: 0.5, **kw)
    torch.cuda.synchronize()
    assert dm.model.status() == 0
    assert torch.isfinite(x).all() and (chain is None or torch.isfinite(chain).all())
    return x, chain, dm.model.inner_runs()


def _on_equals_off(dm, hc, B, want_runs, horizon=H, **kw):
    xa, ca, na = _plan(dm, True, hc, B, horizon, **kw)
    xb, cb, nb = _plan(dm, False, hc, B, horizon, **kw)
    assert (na, nb) == (want_runs, 0), (na, nb)
    assert torch.equal(xa, xb)
    assert (ca is None) == (cb is None) and (ca is None or torch.equal(ca, cb))
    return xa, ca


@pytest.mark.parametrize("in_kernel_noise", [False, True])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 8, 100, 128, 129])
@pytest.mark.parametrize("D", [4, 14])
def test_run_equals_per_layer_kernels(D, B, in_kernel_noise):
    """B = 1, 3: one partly filled cluster of 8 workgroups; 4: a full one; 5: a ragged second tile; 8; 100: the headline's 25 clusters; 128: the largest
    batch that is selected (one workgroup per compute unit); 129: not selected.  With and without the chain, with plan-join on and off."""
    dm = _model(D)
    want = T + N0 if B <= 128 else 0
    for return_chain in (True, False):
        for join in (True, False):
            kw = dict(n_diffusion_steps_without_noise=N0, return_chain=return_chain, join=join)
            if in_kernel_noise:
                kw["seed"] = 4321
            else:
                kw["noise"] = _noise(D, B)
            x, chain = _on_equals_off(dm, _hc(D), B, want, **kw)
            assert float(x.std()) > 0.05
            if chain is not None:
                assert torch.equal(x, chain[-1]) and not torch.equal(chain[1], chain[2])


def test_three_plans_back_to_back_and_two_handles_alternating():
    """The counters are never reset (the base advances with every launch) and belong to the handle: plans in a row on one handle, and two handles
    taking turns on one stream, give what the per-layer kernels give."""
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
        assert dm.model.inner_runs() == T + N0
        got.append((x, chain))
    torch.cuda.synchronize()
    assert a.model.status() == 0 and b.model.status() == 0
    xr, cr, n = _plan(a, False, _hc(D), B, **kw)
    assert n == 0
    for x, chain in got:
        assert torch.equal(x, xr) and torch.equal(chain, cr)


def test_batch_that_grows_and_shrinks_between_plans():
    """A launch advances the counters of its own clusters only: a handle whose batch shrinks and grows again (more clusters than the launch before)
    still starts every run from counters that agree."""
    D = 4
    dm = _model(D, tag="resize")
    for B in (8, 4, 12, 4, 100, 1, 128):
        _on_equals_off(dm, _hc(D), B, T + N0, n_diffusion_steps_without_noise=N0, noise=_noise(D, B))


def test_guided_panda_plan_uses_the_run():
    """B = 4 in two contexts, T = 4 + 2, guide from t < 2: the inner levels do not see the guide, so guided iterations take the run too."""
    import mpd_public_amd as m
    D, B, npc = 14, 4, 2
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args={"device": "cuda", "dtype": torch.float32})
    dm = _model(D)
    hc = {0: t("run_ctx_hc0", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0),
          H - 1: t("run_ctx_hc1", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0)}
    kw = dict(n_diffusion_steps_without_noise=N0, noise=_noise(D, B), guide=product_guide(ds).cuda(), n_guide_steps=2, t_start_guide=2, n_per_context=npc)
    xa, ca, na = _plan(dm, True, hc, B, **kw)
    fa = dm.last_guide_flags.clone()
    xb, cb, nb = _plan(dm, False, hc, B, **kw)
    fb = dm.last_guide_flags.clone()
    assert (na, nb) == (T + N0, 0)
    assert not torch.equal(ca[-1], ca[-2])
    assert torch.equal(ca, cb) and torch.equal(xa, xb) and torch.equal(fa, fb)


@pytest.mark.parametrize("opt,horizon", [(0, 64), (1, 48)])
def test_networks_without_the_seven_layers_plan_as_before(opt, horizon):
    """A three-level network (no 256-channel level) and a horizon in a zero-padded container: no run, outputs as before."""
    D, B = 4, 3
    dm = _model(D, T, opt, horizon)
    kw = dict(n_diffusion_steps_without_noise=N0, noise=_noise(D, B, horizon=horizon))
    _on_equals_off(dm, _hc(D, horizon), B, 0, horizon, **kw)


def test_run_chain_vs_oracle():
    """T = 3 + 1, B = 2 against the CPU oracle at the tolerances of test_joined_chain_vs_oracle (2e-3 over the chain, 5e-4 on the result: fp32
    summation order, amplified by the x0 estimate at large t)."""
    from oracle import diffusion as odiff
    D, To, B, n0 = 4, 3, 2, 1
    dm = _model(D, To)
    noise = t("run_noise_oracle", (To + n0 + 1, B, H, D))
    hc = {0: t("run_hc0", (D,), "uniform", 0.6), H - 1: t("run_hc1", (D,), "uniform", 0.6)}
    x, chain, nr = _plan(dm, True, {k: v.cuda() for k, v in hc.items()}, B, n_diffusion_steps_without_noise=n0, noise=noise.cuda())
    assert nr == To + n0
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
