"""mpdx_plan's joined launch (csrc/fused_level.hpp fused_join_kernel): on an unguided iteration that has a successor, the step's up program and
the next step's down program run as one launch.  Same ops in the same order as the separate kernels, so everything here is BIT-identical
with the handle option (mpdx_unet_set_plan_join) on and off; the oracle test uses the tolerance of the unguided chain tests of
test_gpu_parity.py.  The programs exist for H = 64 only: the shapes are small in B and T."""
import numpy as np
import pytest
import torch

from helpers import synth_sd, t, DIM_MULTS, product_guide

pytestmark = pytest.mark.gpu

H = 64


def _model(D, T, opt=1, horizon=H):
    import mpd_public_amd as m
    from mpd_public_amd import synthetic as syn
    net = m.TemporalUnet(n_support_points=horizon, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    if horizon == H:
        sd = synth_sd(D, opt)
    else:
        sd = syn.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict(sd, strict=True)
    dm = m.GaussianDiffusionModel(model=net.cuda().eval(), variance_schedule="cosine", n_diffusion_steps=T, predict_epsilon=True)
    return dm.cuda().eval()   # (cosine: the exponential schedule has no finite buffers at T = 3 or 4)


def _hc(D, horizon=H):
    return {0: t("join_hc0", (D,), "uniform", 0.6).cuda(), horizon - 1: t("join_hc1", (D,), "uniform", 0.6).cuda()}


def _plan(dm, join, hc, B, horizon=H, seed=None, **kw):
    """(x, chain, joined launches) of one fused plan with the option set to `join`"""
    dm.model.set_plan_join(join)
    if seed is not None:
        dm.in_kernel_noise_min_bytes = 0    # the in-kernel draw, not a pre-generated tensor
        dm.manual_seed(seed)
        dm._rng_offset = 5
    x, chain = dm.plan(hc, B, horizon, noise_std_extra_schedule_fn=lambda tt: 0.5, **kw)
    return x, chain, dm.model.plan_joined()


@pytest.mark.parametrize("in_kernel_noise", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [4, 14])
def test_joined_equals_separate(D, B, in_kernel_noise):
    """T = 4 + 2 steps without noise: the t = 0 steps (no noise term) and the last iteration (no successor: the separate up program)."""
    T, n0 = 4, 2
    dm = _model(D, T)
    kw = dict(n_diffusion_steps_without_noise=n0)
    if in_kernel_noise:
        kw["seed"] = 4321
    else:
        kw["noise"] = t(f"join_noise_D{D}_B{B}", (T + n0 + 1, B, H, D)).cuda()
    xa, ca, na = _plan(dm, True, _hc(D), B, **kw)
    xb, cb, nb = _plan(dm, False, _hc(D), B, **kw)
    assert na == T + n0 - 1 and nb == 0, (na, nb)     # every iteration but the last is joined with its successor
    assert torch.isfinite(ca).all() and float(ca[1].std()) > 0.1 and not torch.equal(ca[1], ca[2])
    assert torch.equal(ca, cb) and torch.equal(xa, xb)
    assert torch.equal(xa, ca[-1])


def test_joined_equals_stepwise_protocol():
    """As test_fused_plan_equals_stepwise_protocol, at a shape of its own: the reference-shaped Python loop runs the separate kernels."""
    import mpd_public_amd as m
    D, T, B, n0 = 4, 4, 3, 2
    dm = _model(D, T)
    dm.model.set_plan_join(True)
    kw = dict(n_samples=B, horizon=H, return_chain=True, sample_fn=m.ddpm_sample_fn, n_diffusion_steps_without_noise=n0,
              noise_std_extra_schedule_fn=lambda tt: 0.5, noise=t("join_noise_proto", (T + n0 + 1, B, H, D)).cuda())
    a = dm.run_inference(None, _hc(D), fused=True, **kw)
    assert dm.model.plan_joined() == T + n0 - 1
    b = dm.run_inference(None, _hc(D), fused=False, **kw)
    assert a.shape == (T + n0 + 1, B, H, D)
    assert torch.equal(a, b) and torch.isfinite(a).all()


@pytest.mark.parametrize("panda", [False, True])
def test_guided_plan_joined_equals_separate(panda):
    """B = 4 in two contexts, T = 4 + 2, guide from t < 2: iterations i = 3, 2 are unguided, i = 1, 0, -1, -2 guided - the transitions
    unguided -> unguided (joined), unguided -> guided (joined: the guide runs after the NEXT pass), guided -> guided (separate)."""
    import mpd_public_amd as m
    D, T, n0, B, npc = (14 if panda else 4), 4, 2, 4, 2
    ds = m.TrajectoryDataset("EnvSpheres3D" if panda else "EnvDense2D", "RobotPanda" if panda else "RobotPointMass",
                             tensor_args={"device": "cuda", "dtype": torch.float32})
    dm = _model(D, T)
    hc = {0: t("join_ctx_hc0", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0),
          H - 1: t("join_ctx_hc1", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0)}
    kw = dict(n_diffusion_steps_without_noise=n0, noise=t(f"join_noise_guided_{D}", (T + n0 + 1, B, H, D)).cuda(), guide=product_guide(ds).cuda(),
              n_guide_steps=2, t_start_guide=2, n_per_context=npc)
    xa, ca, na = _plan(dm, True, hc, B, **kw)
    fa = dm.last_guide_flags.clone()
    xb, cb, nb = _plan(dm, False, hc, B, **kw)
    fb = dm.last_guide_flags.clone()
    assert (na, nb) == (2, 0)
    assert torch.isfinite(ca).all() and not torch.equal(ca[-1], ca[-2])
    assert torch.equal(ca, cb) and torch.equal(xa, xb)
    assert fa.numel() == (T + n0) * 3 * (B // npc) and torch.equal(fa, fb)


def test_joined_without_chain():
    D, T, B, n0 = 4, 4, 3, 2
    dm = _model(D, T)
    kw = dict(n_diffusion_steps_without_noise=n0, noise=t("join_noise_nochain", (T + n0 + 1, B, H, D)).cuda(), return_chain=False)
    xa, ca, na = _plan(dm, True, _hc(D), B, **kw)
    xb, cb, nb = _plan(dm, False, _hc(D), B, **kw)
    assert ca is None and cb is None and (na, nb) == (T + n0 - 1, 0)
    assert torch.isfinite(xa).all() and torch.equal(xa, xb)


def test_joined_chain_vs_oracle():
    """T = 3 + 1, B = 2 against the CPU oracle, at the tolerance of the unguided chain tests of test_gpu_parity.py (2e-3 over the chain,
    5e-4 on the result: fp32 summation order, amplified by the x0 estimate at large t)."""
    from oracle import diffusion as odiff
    D, T, B, n0 = 4, 3, 2, 1
    dm = _model(D, T)
    noise = t("join_noise_oracle", (T + n0 + 1, B, H, D))
    hc = {0: t("join_hc0", (D,), "uniform", 0.6), H - 1: t("join_hc1", (D,), "uniform", 0.6)}
    x, chain, nj = _plan(dm, True, {k: v.cuda() for k, v in hc.items()}, B, n_diffusion_steps_without_noise=n0, noise=noise.cuda())
    assert nj == T + n0 - 1
    nthr = torch.get_num_threads()
    torch.set_num_threads(1)   # (the oracle's fp32 chain moves with the host's thread count: one thread pins it)
    try:
        ref = odiff.run_inference(synth_sd(D, 1), hc, noise, T, variance_schedule="cosine", n_diffusion_steps_without_noise=n0, noise_std=0.5).numpy()
    finally:
        torch.set_num_threads(nthr)
    got = chain.cpu().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
    print("max |chain - oracle| per row:", err)
    assert err.max() < 2e-3, err
    assert err[-1] < 5e-4, err


@pytest.mark.parametrize("opt,horizon", [(0, 64), (1, 48)])
def test_networks_without_the_two_programs_plan_as_before(opt, horizon):
    """A three-level network (other programs) and a horizon in a zero-padded container (no programs): the option changes nothing, no joined launch."""
    D, T, B, n0 = 4, 4, 3, 2
    dm = _model(D, T, opt, horizon)
    kw = dict(n_diffusion_steps_without_noise=n0, noise=t(f"join_noise_fb_{opt}_{horizon}", (T + n0 + 1, B, horizon, D)).cuda())
    xa, ca, na = _plan(dm, True, _hc(D, horizon), B, horizon, **kw)
    xb, cb, nb = _plan(dm, False, _hc(D, horizon), B, horizon, **kw)
    assert (na, nb) == (0, 0)
    assert torch.isfinite(ca).all() and torch.equal(ca, cb) and torch.equal(xa, xb)
