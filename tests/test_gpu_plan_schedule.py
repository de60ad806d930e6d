"""mpdx_plan's launch schedule (csrc/mpdx.hip PlanSchedule + walk_pass): ONE walk serves every program mask together with the inner-level run and the
joined launch, and decides in one place whether the separate final kernel follows a pass.  The combinations no other test drives: every subset of the
handle's fused segments (MPDX_FUSED_MASK, read live) x run on / off x join on / off, on an unguided plan, on a guided one (a joined unguided pass
followed by a guided pass: first unit skipped, mode-2 final), at a batch that takes the join without the run, and on a network that takes neither.
Run and join change no arithmetic, so the comparisons between the options are torch.equal; the oracle comparison uses the tolerances of
test_run_chain_vs_oracle / test_joined_chain_vs_oracle.  Every plan ends with status() == 0 and finite outputs."""
import contextlib
import os

import numpy as np
import pytest
import torch

from helpers import synth_sd, t, DIM_MULTS, product_guide

pytestmark = pytest.mark.gpu

H, D = 64, 4
T, N0 = 4, 2          # T = 4 + 2 steps without noise: six passes
OPTIONS = [(True, True), (True, False), (False, True), (False, False)]   # (run, join)

_MODELS = {}


def _model(T=T, horizon=H):
    if (T, horizon) not in _MODELS:
        import mpd_public_amd as m
        from mpd_public_amd import synthetic as syn
        net = m.TemporalUnet(n_support_points=horizon, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[1])
        sd = synth_sd(D, 1) if horizon == H else syn.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
        net.load_state_dict(sd, strict=True)
        dm = m.GaussianDiffusionModel(model=net.cuda().eval(), variance_schedule="cosine", n_diffusion_steps=T, predict_epsilon=True)
        _MODELS[(T, horizon)] = dm.cuda().eval()
    return _MODELS[(T, horizon)]


def _programs(dm):
    """the static program of every fused segment of the handle (mpdx_unet_fused_program), in segment = mask bit order"""
    from mpd_public_amd import _lib
    lib, h, out = _lib.load(), dm.model._handle(), []
    while lib.mpdx_unet_fused_program(h, len(out)) != -2:
        out.append(lib.mpdx_unet_fused_program(h, len(out)))
    return out


def _joinable(dm, mask):
    """the pass starts with the three-level down program (5) and ends with the up program that holds the final op (3): both segments enabled"""
    progs = _programs(dm)
    return 5 in progs and 3 in progs and all((mask >> progs.index(p)) & 1 for p in (5, 3))


@contextlib.contextmanager
def _fused_mask(mask):
    """MPDX_FUSED_MASK set live around the enclosed plans, as helpers.kernel_path sets MPDX_FUSED"""
    old = os.environ.get("MPDX_FUSED_MASK")
    os.environ["MPDX_FUSED_MASK"] = hex(mask)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MPDX_FUSED_MASK", None)
        else:
            os.environ["MPDX_FUSED_MASK"] = old


def _hc(horizon=H):
    return {0: t("sched_hc0", (D,), "uniform", 0.6).cuda(), horizon - 1: t("sched_hc1", (D,), "uniform", 0.6).cuda()}


def _plan(dm, run, join, hc, B, horizon=H, **kw):
    """(x, chain, run launches, joined launches) of one fused plan under the two handle options"""
    dm.model.set_inner_run(run)
    dm.model.set_plan_join(join)
    x, chain = dm.plan(hc, B, horizon, noise_std_extra_schedule_fn=lambda tt: 0.5, **kw)
    torch.cuda.synchronize()
    assert dm.model.status() == 0
    assert torch.isfinite(x).all() and torch.isfinite(chain).all()
    return x, chain, dm.model.inner_runs(), dm.model.plan_joined()


def _all_options_agree(dm, hc, B, want_runs, want_joined, horizon=H, **kw):
    """the four (run, join) settings give the same bits; the counters are what the schedule promises.  Returns the (run on, join on) result."""
    got = [_plan(dm, run, join, hc, B, horizon, **kw) for run, join in OPTIONS]
    for (run, join), (x, chain, nr, nj) in zip(OPTIONS, got):
        assert (nr, nj) == (want_runs if run else 0, want_joined if join else 0), (run, join, nr, nj)
        assert torch.equal(x, got[0][0]) and torch.equal(chain, got[0][1]), (run, join)
    return got[0]


def test_every_mask_with_run_and_join():
    """B = 5: one full cluster of the run and a ragged second one.  The run needs only the seven per-layer units, so it is taken at every mask; the
    join needs both programs."""
    dm, B = _model(), 5
    progs = _programs(dm)
    assert len(progs) >= 2
    noise = t("sched_noise", (T + N0 + 1, B, H, D)).cuda()
    assert any(_joinable(dm, mask) for mask in range(1 << len(progs)))
    for mask in range(1 << len(progs)):
        with _fused_mask(mask):
            x, chain, _, _ = _all_options_agree(dm, _hc(), B, T + N0, T + 1 if _joinable(dm, mask) else 0, n_diffusion_steps_without_noise=N0, noise=noise)
        assert torch.equal(x, chain[-1]) and float(x.std()) > 0.05 and not torch.equal(chain[1], chain[2])


def test_every_mask_vs_oracle():
    """T = 3 + 1, B = 2, (run on, join on) at every mask against the CPU oracle: 2e-3 over the chain, 5e-4 on the result (fp32 summation order,
    amplified by the x0 estimate at large t) - the tolerances of test_run_chain_vs_oracle and test_joined_chain_vs_oracle."""
    from oracle import diffusion as odiff
    To, B, n0 = 3, 2, 1
    dm = _model(To)
    noise = t("sched_noise_oracle", (To + n0 + 1, B, H, D))
    hc = {0: t("sched_hc0", (D,), "uniform", 0.6), H - 1: t("sched_hc1", (D,), "uniform", 0.6)}
    nthr = torch.get_num_threads()
    torch.set_num_threads(1)   # (the oracle's fp32 chain moves with the host's thread count: one thread pins it)
    try:
        ref = odiff.run_inference(synth_sd(D, 1), hc, noise, To, variance_schedule="cosine", n_diffusion_steps_without_noise=n0, noise_std=0.5).numpy()
    finally:
        torch.set_num_threads(nthr)
    for mask in range(1 << len(_programs(dm))):
        with _fused_mask(mask):
            x, chain, nr, nj = _plan(dm, True, True, {k: v.cuda() for k, v in hc.items()}, B, n_diffusion_steps_without_noise=n0, noise=noise.cuda())
        assert (nr, nj) == (To + n0, To + n0 - 1 if _joinable(dm, mask) else 0), (mask, nr, nj)
        got = chain.cpu().numpy()
        assert got.shape == ref.shape
        err = np.abs(got - ref).reshape(got.shape[0], -1).max(1)
        print(f"mask {mask}: max |chain - oracle| per row:", err)
        assert err.max() < 2e-3, (mask, err)
        assert err[-1] < 5e-4, (mask, err)


def test_every_mask_guided():
    """B = 4 in two contexts, guide from t < 2: iterations i = 3, 2 are unguided and (where the mask admits it) joined with their successors, so the first
    guided pass starts at its second unit and ends in the mode-2 final; guided passes take the run."""
    import mpd_public_amd as m
    B, npc = 4, 2
    ds = m.TrajectoryDataset("EnvDense2D", "RobotPointMass", tensor_args={"device": "cuda", "dtype": torch.float32})
    dm = _model()
    hc = {0: t("sched_ctx_hc0", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0),
          H - 1: t("sched_ctx_hc1", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0)}
    kw = dict(n_diffusion_steps_without_noise=N0, noise=t("sched_noise_guided", (T + N0 + 1, B, H, D)).cuda(), guide=product_guide(ds).cuda(),
              n_guide_steps=2, t_start_guide=2, n_per_context=npc)
    for mask in range(1 << len(_programs(dm))):
        with _fused_mask(mask):
            xa, ca, ra, ja = _plan(dm, True, True, hc, B, **kw)
            fa = dm.last_guide_flags.clone()
            xb, cb, rb, jb = _plan(dm, False, False, hc, B, **kw)
            fb = dm.last_guide_flags.clone()
        assert (ra, ja, rb, jb) == (T + N0, 2 if _joinable(dm, mask) else 0, 0, 0), (mask, ra, ja, rb, jb)
        assert not torch.equal(ca[-1], ca[-2])
        assert torch.equal(xa, xb) and torch.equal(ca, cb), mask
        assert fa.numel() == (T + N0) * 3 * (B // npc) and torch.equal(fa, fb), mask


def test_batch_beyond_the_run_keeps_the_join():
    """B = 129, every segment on: more workgroups than the run may have (one per compute unit), one joined workgroup per compute unit still holds."""
    dm, B = _model(), 129
    full = (1 << len(_programs(dm))) - 1
    assert _joinable(dm, full)
    with _fused_mask(full):
        _all_options_agree(dm, _hc(), B, 0, T + 1, n_diffusion_steps_without_noise=N0, noise=t("sched_noise_129", (T + N0 + 1, B, H, D)).cuda())


def test_container_horizon_takes_neither():
    """Horizon 48 in a container of 64 rows: the schedule selects neither option at any mask, and the options change nothing."""
    horizon, B = 48, 3
    dm = _model(T, horizon)
    noise = t("sched_noise_h48", (T + N0 + 1, B, horizon, D)).cuda()
    for mask in range(1 << len(_programs(dm))):
        with _fused_mask(mask):
            _all_options_agree(dm, _hc(horizon), B, 0, 0, horizon, n_diffusion_steps_without_noise=N0, noise=noise)
