"""GPU parity of the cost-guidance kernel (csrc/guide.hpp, hand-derived gradients) against the oracle's guide
(autograd over oracle/costs.py through the reference-pinned manager glue of oracle/guide.py)."""
from math import ceil

import numpy as np
import pytest
import torch

from guide_ref import input_ambiguity, judge
from helpers import synth_sd, t, oracle_guide, product_guide, obstacle_hugging_trajs, DIM_MULTS

pytestmark = pytest.mark.gpu

CASES = [("EnvNarrowPassageDense2D", "RobotPointMass"), ("EnvSimple2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")]


@pytest.mark.parametrize("env_id,robot_id", CASES + [("EnvSpheres3D", "RobotPointMass3D")])
@pytest.mark.parametrize("scale", [0.9, 1.06])  # in range / beyond +-1 (whole-tensor clip branch of the normaliser)
@pytest.mark.parametrize("weights", [(1e-2, 1e-7), (1.0, 1e-4)])  # reference defaults (inference.py:55-56) / un-attenuated
def test_guide_increment_vs_oracle(env_id, robot_id, scale, weights):
    import mpd_public_amd as m
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args={"device": "cuda", "dtype": torch.float32})
    B = 7
    x = obstacle_hugging_trajs(ds, B, seed=f"g/{env_id}", scale=scale)
    og, comp = oracle_guide(ds, *weights, dtype=torch.float64)
    ref = og(x.double()).numpy()
    pg = product_guide(ds, *weights).cuda()
    got = pg(x.cuda()).cpu().numpy()
    assert got.shape == ref.shape == (B, 64, ds.state_dim)
    assert np.abs(ref).max() > 0
    # endpoints are zeroed exactly; hinge / arg-min decisions of points within 1e-5 of a tie may legitimately differ between fp32 and fp64: the
    # support waypoints they reach are ambiguous (tests/guide_ref.py, decided from the fp64 reference alone); EVERY other waypoint must agree to
    # fp32 rounding of the per-term gradients
    judge(got, ref, input_ambiguity(og, comp, x, robot_id, env_id), weights[0], f"{env_id} {robot_id} scale {scale} w {weights}")


@pytest.mark.parametrize("env_id,robot_id", [("EnvSimple2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")])
@pytest.mark.parametrize("name", ["Identity", "FixedLimitsNormalizer", "SafeLimitsNormalizer", "GaussianNormalizer"])
def test_guide_increment_with_the_other_normalizers_vs_oracle(env_id, robot_id, name):
    """TrajectoryDataset(normalizer=...) (trajectories.py:26): the guide kernel un-normalises with the limits a LimitsNormalizer subclass ends up
    with, not at all under Identity (trajectories in real units), or with x * stds + means under a GaussianNormalizer (normalization.py:140-141:
    no range test - the scale 1.3 trajectories below would be clipped by a limits class)."""
    import mpd_public_amd as m
    ta = {"device": "cuda", "dtype": torch.float32}
    ds0 = m.TrajectoryDataset(env_id, robot_id, tensor_args=ta)
    if name == "GaussianNormalizer":   # (built from data in the reference: here statistics that put the same trajectories at the same places)
        ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=ta)
        mins, maxs = ds0.normalizer.mins.cpu(), ds0.normalizer.maxs.cpu()
        means = 0.5 * (mins + maxs) + 0.03 * t(f"gn_mean/{env_id}", (ds.state_dim,), "uniform")
        stds = 0.5 * (maxs - mins) / 1.3 * (1.0 + 0.1 * t(f"gn_std/{env_id}", (ds.state_dim,), "uniform"))
        ds.normalizer = m.GaussianNormalizer(means, stds).to("cuda")
    else:
        ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=ta, normalizer=name)
    assert type(ds.normalizer).__name__ == name
    x = obstacle_hugging_trajs(ds0, 7, seed=f"gn/{env_id}", scale=1.3 if name == "GaussianNormalizer" else 0.9)
    if name == "Identity":
        x = ds0.normalizer.unnormalize(x.cuda()).cpu()
    og, comp = oracle_guide(ds, dtype=torch.float64)
    ref = og(x.double()).numpy()
    got = product_guide(ds).cuda()(x.cuda()).cpu().numpy()
    assert np.abs(ref).max() > 0
    judge(got, ref, input_ambiguity(og, comp, x, robot_id, name), 1e-2, f"{env_id} {robot_id} {name}")


def test_guided_plan_under_gaussian_normalizer_fused_equals_stepwise_and_oracle_start():
    """A GaussianNormalizer dataset under the HIP guide: fused plan == step-by-step protocol loop bit for bit, and both track the
    oracle loop with the oracle's GaussianNormalizer through the first guided steps."""
    import mpd_public_amd as m
    from oracle import diffusion as odiff
    T, B = 25, 4
    ds, dm, noise, hc, n0 = _guided_setup("EnvDense2D", "RobotPointMass", T, B, 0)
    mins, maxs = ds.normalizer.mins.cpu(), ds.normalizer.maxs.cpu()
    ds.normalizer = m.GaussianNormalizer(0.5 * (mins + maxs) + 0.02, 0.45 * (maxs - mins)).to("cuda")
    pg = product_guide(ds, 1e-2, 1e-7).cuda()
    kw = dict(n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=pg, n_guide_steps=5,
              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5,
              noise=noise.cuda())
    a = dm.run_inference(None, hc, fused=True, **kw)
    b = dm.run_inference(None, hc, fused=False, **kw)
    assert torch.equal(a, b)
    og, _ = oracle_guide(ds, 1e-2, 1e-7)
    ref = odiff.run_inference(synth_sd(ds.state_dim, 0), {k: v.cpu() for k, v in hc.items()}, noise, T, noise_std=0.5, guide=og, n_guide_steps=5,
                              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0)
    k_guide = T - ceil(0.25 * T)
    err = (a.cpu() - ref).abs().reshape(a.shape[0], -1).amax(1).numpy()
    assert err[: k_guide + 2].max() < 2e-3, err[: k_guide + 2]


@pytest.mark.parametrize("env_id,robot_id", [("EnvDense2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")])
@pytest.mark.parametrize("H", [32, 128, 48, 96])
def test_guide_increment_other_horizons_vs_oracle(env_id, robot_id, H):
    """Horizons other than 64: the support points of a trajectory map to the lanes of one (H <= 64) or two (H <= 128) waves; the GP
    prior's neighbours come from the LDS-staged state (no cross-lane traffic: the support index may cross the wave boundary).
    The increment equals the oracle's autograd guide, end points zeroed."""
    import mpd_public_amd as m
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args={"device": "cuda", "dtype": torch.float32})
    ds.n_support_points = H
    B, D = 5, ds.state_dim
    qd = D // 2
    a_, b_ = t(f"gh/{env_id}/a", (B, 1, qd), "uniform", 0.9), t(f"gh/{env_id}/b", (B, 1, qd), "uniform", 0.9)
    sgrid = torch.linspace(0, 1, H).reshape(1, H, 1)
    x = torch.cat([a_ + (b_ - a_) * sgrid + 0.04 * t(f"gh/{env_id}/n{H}", (B, H, qd)), 0.3 * t(f"gh/{env_id}/v{H}", (B, H, qd))], -1).contiguous()
    w = (1e-2, 1e-7)
    og, comp = oracle_guide(ds, *w, dtype=torch.float64)
    ref = og(x.double()).numpy()
    got = product_guide(ds, *w).cuda()(x.cuda()).cpu().numpy()
    assert got.shape == ref.shape == (B, H, D) and np.abs(ref).max() > 0
    judge(got, ref, input_ambiguity(og, comp, x, robot_id, f"H={H}"), w[0], f"{env_id} {robot_id} H={H}")
    # the post-loop metrics kernel on the same horizons: path length / smoothness sums over all H - 1 segments
    from oracle.normalizer import LimitsNormalizer
    xu = LimitsNormalizer(ds.normalizer.mins.cpu(), ds.normalizer.maxs.cpu()).unnormalize(x)
    mt = ds.task.trajectory_metrics(xu.cuda()).cpu().numpy()
    np.testing.assert_allclose(mt[:, 1], np.linalg.norm(np.diff(xu[..., :qd].numpy(), axis=1), axis=-1).sum(-1), rtol=2e-5)
    np.testing.assert_allclose(mt[:, 2], np.linalg.norm(np.diff(xu[..., qd:].numpy(), axis=1), axis=-1).sum(-1), rtol=2e-5)


@pytest.mark.parametrize("env_id,robot_id", CASES[::2])
def test_guide_apply_mode_updates_state_flags_and_hard_conditions(env_id, robot_id):
    """mpdx_guide_step in apply mode == x + guide(x), hard conditioning, and max|x_new| for the next range test."""
    import ctypes as C
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args={"device": "cuda", "dtype": torch.float32})
    B, D = 6, ds.state_dim
    x = obstacle_hugging_trajs(ds, B, seed=f"apply/{env_id}", scale=1.03).cuda()
    pg = product_guide(ds).cuda()
    inc = pg(x)
    hs, hg = t("apply_hs", (B, D), "uniform").cuda(), t("apply_hg", (B, D), "uniform").cuda()
    want = x + inc
    want[:, 0], want[:, -1] = hs, hg
    lib, gp = _lib.load(), pg.device_params(x.device)
    # two contexts of 3 trajectories each: per-context range test
    flag_in = torch.zeros(2, dtype=torch.int32, device="cuda")
    _lib.check(lib.mpdx_absmax(x.data_ptr(), flag_in.data_ptr(), 3, B, 64, D, _lib.current_stream()))
    amax = x.abs().reshape(2, -1).max(1)[0]
    assert torch.equal(flag_in.view(torch.float32), amax)
    assert bool((amax > 1.0001).all())  # both contexts take the clip branch here, as the single-context guide call did
    flag_out = torch.zeros(2, dtype=torch.int32, device="cuda")
    y = x.clone()
    _lib.check(lib.mpdx_guide_step(C.byref(gp), y.data_ptr(), None, hs.data_ptr(), hg.data_ptr(), flag_in.data_ptr(), flag_out.data_ptr(),
                                   3, B, 64, D, _lib.current_stream()))
    assert torch.equal(y, want)
    assert torch.equal(flag_out.view(torch.float32), want.abs().reshape(2, -1).max(1)[0])


def _guided_setup(env_id, robot_id, T, B, opt):
    import mpd_public_amd as m
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args={"device": "cuda", "dtype": torch.float32})
    D = ds.state_dim
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
    n0 = 5
    noise = t(f"guided_noise/{env_id}", (T + n0 + 1, B, 64, D))
    start = ds.normalizer.normalize(torch.cat([t(f"gs/{env_id}", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    goal = ds.normalizer.normalize(torch.cat([t(f"gg/{env_id}", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    return ds, dm, noise, {0: start, 63: goal}, n0


@pytest.mark.parametrize("env_id,robot_id,opt", [("EnvNarrowPassageDense2D", "RobotPointMass", 0), ("EnvSpheres3D", "RobotPanda", 1)])
def test_guided_plan_vs_oracle_chain(env_id, robot_id, opt):
    """Full guided plan (mpdx_plan: U-Net + posterior mean + 5 guide iterations + noise) against the oracle loop with
    the oracle guide, at the reference's default weights (inference.py:55-56).  (Much larger weights make the guided
    dynamics chaotic - steps of O(1) in normalised units across obstacle boundaries - and no two fp32 implementations
    agree then.)"""
    import mpd_public_amd as m
    from oracle import diffusion as odiff
    T, B = 25, 5
    ds, dm, noise, hc, n0 = _guided_setup(env_id, robot_id, T, B, opt)
    w = (1e-2, 1e-7)
    og, _ = oracle_guide(ds, *w, dtype=torch.float32)
    pg = product_guide(ds, *w).cuda()
    kw = dict(n_guide_steps=5, t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0)
    chain = dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=pg,
                             noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise.cuda(), **kw).cpu().numpy()
    ref = odiff.run_inference(synth_sd(ds.state_dim, opt), {k: v.cpu() for k, v in hc.items()}, noise, T, noise_std=0.5, guide=og,
                              **kw).numpy()
    unguided = odiff.run_inference(synth_sd(ds.state_dim, opt), {k: v.cpu() for k, v in hc.items()}, noise, T, noise_std=0.5,
                                   n_diffusion_steps_without_noise=n0).numpy()
    assert np.abs(ref[-1] - unguided[-1]).max() > 5e-3, "guidance must matter in this test"
    err = np.abs(chain - ref).reshape(chain.shape[0], -1).max(1)
    k_guide = T - ceil(0.25 * T)  # chain index after which guide iterations run
    assert err[: k_guide + 1].max() < 2e-3, err   # un-guided part: fp32 tolerance of the unguided chain test
    # guided part: the hinge gradient is discontinuous and norm-clipped to unit length, so a waypoint within fp32
    # rounding of a margin (or of an argmin tie) moves by exactly one increment w = 1e-2 in one implementation and not in
    # the other.  Only ISOLATED waypoints may differ, by a few increments at most; everything else stays at 2e-3.
    # (measured: errors stay ~5e-6 until the first guided step, then grow by fractions of an increment per flip.)
    d = np.abs(chain[-1] - ref[-1]).max(-1)        # [B, H]
    assert np.median(d) < 2e-3, np.median(d)
    assert (d > w[0]).mean() < 0.02, (d > w[0]).mean()     # isolated waypoints only ...
    # ... and by a few increments at most.  Which waypoint flips depends on last-bit rounding of the ~20 guided U-Net passes before it
    # (measured worst waypoint over builds: 1.0 - 1.6 w), so the bound is a COUNT: at most 2 of the 320 waypoints beyond 1.5 w, none beyond 5 w
    assert int((d > 1.5 * w[0]).sum()) <= 2, (int((d > 1.5 * w[0]).sum()), d.max())
    assert d.max() < 5 * w[0], d.max()
    # north_star: trajectory-level results identical to 3 s.f. (path length and smoothness of the planned trajectories)
    qd = ds.state_dim // 2
    for name, fn in (("path_length", lambda z: np.linalg.norm(np.diff(z[..., :qd], axis=1), axis=-1).sum(-1)),
                     ("smoothness", lambda z: np.linalg.norm(np.diff(z[..., qd:], axis=1), axis=-1).sum(-1))):
        a_, b_ = fn(chain[-1]).mean(), fn(ref[-1]).mean()
        assert abs(a_ - b_) <= 5e-3 * abs(b_), (name, a_, b_)  # 3 significant figures


@pytest.mark.parametrize("env_id,robot_id,opt", [("EnvNarrowPassageDense2D", "RobotPointMass", 0), ("EnvSpheres3D", "RobotPanda", 1)])
def test_prior_then_guide_post_loop_vs_oracle(env_id, robot_id, opt):
    """planner_alg = 'diffusion_prior_then_guide' (inference.py:263-282): an UNGUIDED plan, then (t_start_guide + n0) * n_guide_steps
    pure guide iterations `guide_gradient_steps(trajs, hard_conds, guide, n_guide_steps=1)`, each appended to the chain.  VALUES of
    every post-loop iterate against oracle.guide applied the same way - once from the SAME starting trajectories (isolates the
    post-loop arithmetic: 60 compounding guide kernels) and once end to end from the oracle's own unguided plan."""
    import mpd_public_amd as m
    from oracle import diffusion as odiff
    T, B = 25, 5
    ds, dm, noise, hc, n0 = _guided_setup(env_id, robot_id, T, B, opt)
    w = (1e-2, 1e-7)
    og, _ = oracle_guide(ds, *w, dtype=torch.float32)
    pg = product_guide(ds, *w).cuda()
    n_guide_steps, t_start_guide = 5, ceil(0.25 * T)
    n_post = (t_start_guide + n0) * n_guide_steps
    chain = dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=None,
                             n_guide_steps=n_guide_steps, t_start_guide=t_start_guide, n_diffusion_steps_without_noise=n0,
                             noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise.cuda())
    hc_b = {k: v.reshape(1, -1).expand(B, -1).contiguous() for k, v in hc.items()}
    x, post = chain[-1].clone(), []
    for _ in range(n_post):   # the entry's loop (mpd_public_amd/inference.py), on the HIP guide kernel
        x = m.guide_gradient_steps(x, hard_conds=hc_b, guide=pg, n_guide_steps=1, unnormalize_data=False)
        post.append(x.cpu())
    post = torch.stack(post).numpy()
    hc_cpu = {k: v.cpu() for k, v in hc.items()}

    def oracle_post(x0):
        xs, xo = [], x0.clone()
        for _ in range(n_post):
            xo = odiff.guide_gradient_steps(xo, hc_cpu, og, 1)
            xs.append(xo.clone())
        return torch.stack(xs).numpy()
    same = oracle_post(chain[-1].cpu())                       # same start
    ref_chain = odiff.run_inference(synth_sd(ds.state_dim, opt), hc_cpu, noise, T, noise_std=0.5, n_diffusion_steps_without_noise=n0)
    e2e = oracle_post(ref_chain[-1])                          # end to end
    moved = np.abs(same[-1] - chain[-1].cpu().numpy()).max()
    assert moved > 5e-3, f"the post-loop guidance must move the trajectories in this test (moved {moved:.2e})"
    # hard conditions hold on every iterate, bit for bit
    for k, v in hc_cpu.items():
        assert (post[:, :, k, :] == v.numpy()[None, None]).all()
    # first iterate from the same start: one guide kernel against one oracle autograd pass
    d0 = np.abs(post[0] - same[0]).max(-1)
    assert (d0 > 2e-6).mean() < 0.01, (d0 > 2e-6).mean()
    for name, ref in (("same start", same), ("end to end", e2e)):
        d = np.abs(post - ref).max(-1)                         # [n_post, B, H]
        # as in test_guided_plan_vs_oracle_chain: a waypoint within fp32 rounding of a hinge / arg-min boundary moves by one increment
        # (w = 1e-2) in one implementation and not in the other; isolated waypoints only, a few increments at most, at every iterate
        assert np.median(d[-1]) < 2e-3, (name, np.median(d[-1]))
        frac = (d > w[0]).reshape(n_post, -1).mean(1)
        assert frac.max() < 0.03, (name, frac.max())
        assert d.max() < 8 * w[0], (name, d.max())
        qd = ds.state_dim // 2
        for mname, fn in (("path_length", lambda z: np.linalg.norm(np.diff(z[..., :qd], axis=1), axis=-1).sum(-1)),
                          ("smoothness", lambda z: np.linalg.norm(np.diff(z[..., qd:], axis=1), axis=-1).sum(-1))):
            a_, b_ = fn(post[-1]).mean(), fn(ref[-1]).mean()
            assert abs(a_ - b_) <= 5e-3 * abs(b_), (name, mname, a_, b_)   # 3 significant figures


@pytest.mark.parametrize("H", [32, 128, 48])
def test_guided_plan_other_horizons_fused_equals_stepwise_and_tracks_oracle(H):
    """A full guided plan at H = 32 / 128 (Panda): mpdx_plan == the step-by-step protocol loop bit for bit, the un-guided part of the
    chain equals the oracle's, and the guided end result stays within the guided-chain tolerance class (isolated waypoints may take
    the other hinge branch)."""
    import mpd_public_amd as m
    from mpd_public_amd import synthetic as syn
    from oracle import diffusion as odiff
    T, B, n0 = 25, 3, 3
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args={"device": "cuda", "dtype": torch.float32})
    ds.n_support_points = H
    D = ds.state_dim
    net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[1])
    sd = syn.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict(sd, strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
    noise = t(f"gh_noise_{H}", (T + n0 + 1, B, H, D))
    start = ds.normalizer.normalize(torch.cat([t("gh_s", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    goal = ds.normalizer.normalize(torch.cat([t("gh_g", (D // 2,), "uniform", 0.6).cuda(), torch.zeros(D // 2, device="cuda")]))
    hc = {0: start, H - 1: goal}
    w = (1e-2, 1e-7)
    pg = product_guide(ds, *w).cuda()
    kw = dict(n_samples=B, horizon=H, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=pg, n_guide_steps=5, t_start_guide=ceil(0.25 * T),
              n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise.cuda())
    a = dm.run_inference(None, hc, fused=True, **kw)
    b = dm.run_inference(None, hc, fused=False, **kw)
    assert torch.equal(a, b)
    og, _ = oracle_guide(ds, *w, dtype=torch.float32)
    ref = odiff.run_inference(sd, {k: v.cpu() for k, v in hc.items()}, noise, T, noise_std=0.5, guide=og, n_guide_steps=5,
                              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0).numpy()
    chain = a.cpu().numpy()
    k_guide = T - ceil(0.25 * T)
    err = np.abs(chain - ref).reshape(chain.shape[0], -1).max(1)
    assert err[: k_guide + 1].max() < 2e-3, err
    d = np.abs(chain[-1] - ref[-1]).max(-1)
    assert np.median(d) < 2e-3 and (d > w[0]).mean() < 0.03 and d.max() < 5 * w[0], (np.median(d), (d > w[0]).mean(), d.max())


def test_guided_plan_fused_equals_stepwise():
    import mpd_public_amd as m
    T, B = 25, 4
    ds, dm, noise, hc, n0 = _guided_setup("EnvDense2D", "RobotPointMass", T, B, 0)
    pg = product_guide(ds, 1e-2, 1e-7).cuda()
    kw = dict(n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=pg, n_guide_steps=5,
              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5,
              noise=noise.cuda())
    a = dm.run_inference(None, hc, fused=True, **kw)
    b = dm.run_inference(None, hc, fused=False, **kw)   # p_sample_loop -> ddpm_sample_fn -> guide_gradient_steps -> guide(x)
    assert torch.equal(a, b)


def test_guided_plan_under_identity_normalizer_fused_equals_stepwise_and_oracle_start():
    """A dataset built with normalizer='Identity' (trajectories.py:26): the fused plan, the step-by-step protocol loop and - up to the first guided
    step's tolerance - the oracle loop with the oracle's Identity agree; the kernel's range test plays no part."""
    import mpd_public_amd as m
    from oracle import diffusion as odiff
    T, B = 25, 4
    _, dm, noise, hc, n0 = _guided_setup("EnvDense2D", "RobotPointMass", T, B, 0)
    ds = m.TrajectoryDataset("EnvDense2D", "RobotPointMass", tensor_args={"device": "cuda", "dtype": torch.float32}, normalizer="Identity")
    pg = product_guide(ds, 1e-2, 1e-7).cuda()
    kw = dict(n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=pg, n_guide_steps=5,
              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5,
              noise=noise.cuda())
    a = dm.run_inference(None, hc, fused=True, **kw)
    b = dm.run_inference(None, hc, fused=False, **kw)
    assert torch.equal(a, b)
    og, _ = oracle_guide(ds, 1e-2, 1e-7)
    ref = odiff.run_inference(synth_sd(ds.state_dim, 0), {k: v.cpu() for k, v in hc.items()}, noise, T, noise_std=0.5, guide=og, n_guide_steps=5,
                              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0)
    k_guide = T - ceil(0.25 * T)
    err = (a.cpu() - ref).abs().reshape(a.shape[0], -1).amax(1).numpy()
    assert err[: k_guide + 2].max() < 2e-3, err[: k_guide + 2]


def test_multi_context_batch_equals_separate_plans():
    """BASELINE configs[4] shape in miniature: several start/goal contexts in one batch (per-trajectory hard conditions,
    per-context normaliser range test) == one plan per context, bit for bit."""
    import mpd_public_amd as m
    from mpd_public_amd.parallel import plan_contexts
    T, n, C = 25, 4, 3
    ds, dm, _, _, n0 = _guided_setup("EnvDense2D", "RobotPointMass", T, n, 0)
    D = ds.state_dim
    pg = product_guide(ds, 1e-2, 1e-7).cuda()
    noise = t("mc_noise", (T + n0 + 1, C * n, 64, D)).cuda()
    noise[0, n:2 * n] *= 1.5   # make context 1's early iterates exceed the +-1 range while the others need not
    starts = torch.stack([ds.normalizer.normalize(torch.cat([t(f"mc_s{c}", (2,), "uniform", 0.7).cuda(), torch.zeros(2, device="cuda")])) for c in range(C)])
    goals = torch.stack([ds.normalizer.normalize(torch.cat([t(f"mc_g{c}", (2,), "uniform", 0.7).cuda(), torch.zeros(2, device="cuda")])) for c in range(C)])
    kw = dict(n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5, guide=pg, n_guide_steps=5,
              t_start_guide=ceil(0.25 * T))
    batched, (lo, hi) = plan_contexts(dm, starts, goals, n, horizon=64, noise=noise, **kw)
    assert (lo, hi) == (0, C) and batched.shape == (C * n, 64, D)
    for c in range(C):
        x, _ = dm.plan({0: starts[c], 63: goals[c]}, n, 64, noise=noise[:, c * n:(c + 1) * n].contiguous(), return_chain=False, **kw)
        assert torch.equal(batched[c * n:(c + 1) * n], x), c


def test_panda_guide_rejects_interpolation_that_exceeds_lds():
    """The Panda kernel keeps FK results and per-group gradients of every interpolated point in LDS: 512 points do not fit
    160 KB.  The C ABI must refuse (error code + message), not launch."""
    import mpd_public_amd as m
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args={"device": "cuda", "dtype": torch.float32})
    costs = [m.CostCollision(ds.robot, 64, field=f, sigma_coll=1.0) for f in ds.task.get_collision_fields()]
    comp = m.CostComposite(ds.robot, 64, costs, weights_cost_l=[1e-2] * len(costs))
    g = m.GuideManagerTrajectoriesWithVelocity(ds, comp, clip_grad=True, interpolate_trajectories_for_collision=True,
                                               num_interpolated_points_for_collision=512).cuda()
    x = obstacle_hugging_trajs(ds, 3, seed="lds_cap").cuda()
    with pytest.raises(RuntimeError, match="LDS"):
        g(x)
    ok = m.GuideManagerTrajectoriesWithVelocity(ds, comp, clip_grad=True, interpolate_trajectories_for_collision=True,
                                                num_interpolated_points_for_collision=192).cuda()
    assert bool(torch.isfinite(ok(x)).all())   # 192 points fit (3 passes of the 64-lane point loop)


# ---------------------------------------------------------------------------------------------- options of the guide manager
@pytest.mark.parametrize("env_id,robot_id", CASES[::2])
def test_guide_clip_by_value_vs_oracle(env_id, robot_id):
    """clip_grad_rule='value' (guides.py:232-236): per-element clip to +-max_grad_value instead of the per-waypoint norm clip."""
    import mpd_public_amd as m
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args={"device": "cuda", "dtype": torch.float32})
    x = obstacle_hugging_trajs(ds, 6, seed=f"clipv/{env_id}", scale=0.95)
    for mv in (0.1, 0.35):
        og, comp = oracle_guide(ds, 1.0, 1e-4, dtype=torch.float64, clip_grad_rule="value", max_grad_value=mv)
        ref = og(x.double()).numpy()
        got = product_guide(ds, 1.0, 1e-4, clip_grad_rule="value", max_grad_value=mv).cuda()(x.cuda()).cpu().numpy()
        norm_ref = product_guide(ds, 1.0, 1e-4).cuda()(x.cuda()).cpu().numpy()
        assert np.abs(got - norm_ref).max() > 1e-3, "the two clip rules must differ on this input"
        judge(got, ref, input_ambiguity(og, comp, x, robot_id, f"value clip {mv}"), 1.0, f"{env_id} {robot_id} value clip {mv}")
    with pytest.raises(NotImplementedError):
        m.GuideManagerTrajectoriesWithVelocity(ds, product_guide(ds).cost, clip_grad=True, clip_grad_rule="median")


def test_gp_half_factor_switch_vs_oracle():
    """The GP prior with and without GPMP2's 1/2 (undecidable from the reference tree: explicit switch).
    Un-clipped, the GP increment halves exactly; with the norm clip it only changes where |grad| < max_grad_norm."""
    import mpd_public_amd as m
    ds = m.TrajectoryDataset("EnvDense2D", "RobotPointMass", tensor_args={"device": "cuda", "dtype": torch.float32})
    x = (0.02 * t("gph/x", (5, 64, 4))).contiguous()   # near-constant trajectories far from obstacles: only the GP term acts
    x[..., :2] += 0.9
    for clip in (False, True):
        out = {}
        for half in (False, True):
            og, _ = oracle_guide(ds, 0.0, 1e-3, clip_grad=clip, dtype=torch.float64, gp_half_factor=half)
            ref = og(x.double()).numpy()
            got = product_guide(ds, 0.0, 1e-3, clip_grad=clip, gp_half_factor=half).cuda()(x.cuda()).cpu().numpy()
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-7)
            out[half] = got
        assert np.abs(out[False]).max() > 0
        if not clip:
            np.testing.assert_allclose(out[True], 0.5 * out[False], rtol=1e-6, atol=1e-12)


def test_python_cost_callable_guide_vs_reference_golden(golden_dir):
    """A guide around an ARBITRARY Python cost (guides.py:190's contract) takes the torch-autograd path on the GPU; the
    reference's own manager produced these vectors with the same toy cost (tests/golden/make_golden.py)."""
    import mpd_public_amd as m
    from helpers import toy_cost, load_npz
    g = load_npz(golden_dir / "guide.npz")
    for robot, D, env in (("RobotPointMass", 4, "EnvSimple2D"), ("RobotPanda", 14, "EnvSpheres3D")):
        ds = m.TrajectoryDataset(env, robot, tensor_args={"device": "cuda", "dtype": torch.float32})
        gm = m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost, clip_grad=True, interpolate_trajectories_for_collision=True).cuda()
        assert not gm.is_native
        for scale, tag in ((0.5, "inrange"), (0.9, "clipped")):
            x = t(f"guide_x_D{D}", (5, 64, D), "uniform", scale=scale * 1.2).cuda()
            np.testing.assert_allclose(gm(x).cpu().numpy(), g[f"guide_D{D}_{tag}"], rtol=2e-5, atol=2e-7)


def test_python_cost_guided_chain_vs_reference_golden(golden_dir):
    """run_inference with a Python-cost guide: the step-by-step protocol loop (HIP U-Net + step kernels, torch-autograd guide)
    against the chain the real reference produced with the same toy cost."""
    import mpd_public_amd as m
    from helpers import toy_cost, load_npz
    g = load_npz(golden_dir / "guide.npz")
    D, T, B, n0, opt = 4, 25, 4, 5, 0
    ds = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass", tensor_args={"device": "cuda", "dtype": torch.float32})
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
    gm = m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost, clip_grad=True, interpolate_trajectories_for_collision=True).cuda()
    noise = t("chain_noise_guided", (T + n0 + 1, B, 64, D))
    hc = {0: t("chain_hc0", (D,), "uniform").cuda(), 63: t("chain_hc1", (D,), "uniform").cuda()}
    chain = dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=gm, n_guide_steps=5,
                             t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5,
                             noise=noise.cuda()).cpu().numpy()
    ref = g["guided_chain_opt0"]
    assert chain.shape == ref.shape
    np.testing.assert_allclose(chain, ref, rtol=0, atol=2e-3)
    np.testing.assert_allclose(chain[-1], ref[-1], rtol=0, atol=5e-4)


def test_scale_grad_by_std_fused_equals_stepwise_and_oracle():
    """scale_grad_by_std=True (sample_functions.py:41-43,77-78): every guide increment times model_var[t].  Stays on the fused
    mpdx_plan path (coefs[t].guide_scale), bit-identical to the protocol loop, and follows the oracle."""
    import mpd_public_amd as m
    from oracle import diffusion as odiff
    T, B = 25, 4
    ds, dm, noise, hc, n0 = _guided_setup("EnvDense2D", "RobotPointMass", T, B, 0)
    w = (1.0, 1e-4)   # model_var ~ 1e-2..1e-4 in the guided range: use un-attenuated weights so that the scaled increments matter
    pg = product_guide(ds, *w).cuda()
    kw = dict(n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=pg, n_guide_steps=5,
              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5,
              noise=noise.cuda(), scale_grad_by_std=True)
    a = dm.run_inference(None, hc, fused=True, **kw)
    b = dm.run_inference(None, hc, fused=False, **kw)
    assert torch.equal(a, b)
    plain = dm.run_inference(None, hc, fused=True, **dict(kw, scale_grad_by_std=False))
    assert not torch.equal(a, plain)
    og, _ = oracle_guide(ds, *w, dtype=torch.float32)
    ref = odiff.run_inference(synth_sd(ds.state_dim, 0), {k: v.cpu() for k, v in hc.items()}, noise, T, noise_std=0.5, guide=og, n_guide_steps=5,
                              t_start_guide=ceil(0.25 * T), n_diffusion_steps_without_noise=n0, scale_grad_by_std=True).numpy()
    d = np.abs(a.cpu().numpy()[-1] - ref[-1]).max(-1)
    assert np.median(d) < 2e-3 and d.max() < 5e-2, (np.median(d), d.max())


def test_zero_guide_steps_is_unguided():
    """n_guide_steps=0: the reference's `for _ in range(0)` runs no guide iteration; both paths must equal the unguided plan."""
    import mpd_public_amd as m
    T, B = 25, 3
    ds, dm, noise, hc, n0 = _guided_setup("EnvDense2D", "RobotPointMass", T, B, 0)
    pg = product_guide(ds).cuda()
    kw = dict(n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, n_diffusion_steps_without_noise=n0,
              noise_std_extra_schedule_fn=lambda tt: 0.5, noise=noise.cuda())
    plain = dm.run_inference(None, hc, **kw)
    for fused in (True, False):
        z = dm.run_inference(None, hc, fused=fused, guide=pg, n_guide_steps=0, t_start_guide=ceil(0.25 * T), **kw)
        assert torch.equal(z, plain), fused


def test_ddim_accepts_unbatched_and_cpu_hard_conditions():
    """ddim_sample / p_sample_loop normalise hard conditions ([D] broadcast, CPU -> device) before the kernels index them as
    hs[b*D+d] (a [D] tensor was read out of bounds for b > 0)."""
    import mpd_public_amd as m
    D, T, B = 4, 25, 5
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[0])
    net.load_state_dict(synth_sd(D, 0), strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
    x_T = t("ddim_hc_noise", (8, B, 64, D))
    hc1 = {0: t("chain_hc0", (D,), "uniform"), 63: t("chain_hc1", (D,), "uniform")}            # [D], on the CPU
    hcB = {k: v.reshape(1, -1).expand(B, -1).contiguous().cuda() for k, v in hc1.items()}      # [B,D], on the GPU
    xa, ca = dm.conditional_sample(hc1, horizon=64, batch_size=B, ddim=True, return_chain=True, noise=x_T)
    xb, cb = dm.conditional_sample(hcB, horizon=64, batch_size=B, ddim=True, return_chain=True, noise=x_T)
    assert torch.equal(ca, cb)
    assert torch.equal(xa[:, 0], hcB[0]) and torch.equal(xa[:, 63], hcB[63])
    pa, _ = dm.conditional_sample(hc1, horizon=64, batch_size=B, return_chain=True, noise=t("psl_noise", (T + 1, B, 64, D)))
    assert torch.equal(pa[:, 0], hcB[0]) and torch.equal(pa[:, 63], hcB[63])
    with pytest.raises(ValueError):
        dm.conditional_sample({0: torch.zeros(3, D)}, horizon=64, batch_size=B, ddim=True, noise=x_T)


def test_unet_deepcopy_rebuilds_its_own_engine():
    """copy.deepcopy(model) (the reference's EMA pattern): parameters are copied, the native handle / packed weights are not
    shared; both copies keep working and a parameter change in one does not leak into the other."""
    import copy
    import mpd_public_amd as m
    D = 4
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[0])
    net.load_state_dict(synth_sd(D, 0), strict=True)
    net = net.cuda().eval()
    x, tt = t("dc_x", (3, 64, D)).cuda(), torch.full((3,), 7, dtype=torch.long, device="cuda")
    y0 = net(x, tt)
    ema = copy.deepcopy(net)
    assert ema._h is None and ema._packed is None
    assert torch.equal(ema(x, tt), y0)
    with torch.no_grad():
        ema.final_conv[1].bias.add_(1.0)
    assert torch.allclose(ema(x, tt), y0 + 1.0, atol=1e-6) and torch.equal(net(x, tt), y0)
    del ema   # must not free the original's handle
    assert torch.equal(net(x, tt), y0)


def test_guide_options_and_sampler_options_vs_reference_golden(golden_dir):
    """Vectors from the REAL reference (tests/golden/guide_opts.npz): clip_grad_rule='value', clip_grad=False, a
    scale_grad_by_std=True chain and a guided DDIM chain (n_guide_steps=3 requested, one applied) - product on the GPU
    (HIP U-Net / step kernels; the toy Python cost takes the torch-autograd guide path)."""
    import mpd_public_amd as m
    from helpers import toy_cost, load_npz
    g = load_npz(golden_dir / "guide_opts.npz")
    for robot, D, env in (("RobotPointMass", 4, "EnvSimple2D"), ("RobotPanda", 14, "EnvSpheres3D")):
        ds = m.TrajectoryDataset(env, robot, tensor_args={"device": "cuda", "dtype": torch.float32})
        x = t(f"guide_x_D{D}", (5, 64, D), "uniform", scale=0.6).cuda()
        for mv in (0.1, 0.004):
            gm = m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost, clip_grad=True, clip_grad_rule="value", max_grad_value=mv,
                                                        interpolate_trajectories_for_collision=True).cuda()
            np.testing.assert_allclose(gm(x).cpu().numpy(), g[f"value_D{D}_mv{mv}"], rtol=2e-5, atol=2e-7)
        gm = m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost, clip_grad=False, interpolate_trajectories_for_collision=True).cuda()
        np.testing.assert_allclose(gm(x).cpu().numpy(), g[f"noclip_D{D}"], rtol=2e-5, atol=2e-7)

    def big_cost(x, x_interpolated=None, return_invidual_costs_and_weights=False, **kw):
        cl, _ = toy_cost(x, x_interpolated=x_interpolated)
        return cl, [1.0, 0.3]

    D, T, B, n0, opt = 4, 25, 4, 5, 0
    ds = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass", tensor_args={"device": "cuda", "dtype": torch.float32})
    net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    dm = m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
    hc = {0: t("chain_hc0", (D,), "uniform").cuda(), 63: t("chain_hc1", (D,), "uniform").cuda()}
    gm = m.GuideManagerTrajectoriesWithVelocity(ds, big_cost, clip_grad=True, interpolate_trajectories_for_collision=True).cuda()
    chain = dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, sample_fn=m.ddpm_sample_fn, guide=gm, n_guide_steps=5,
                             t_start_guide=ceil(0.25 * T), scale_grad_by_std=True, n_diffusion_steps_without_noise=n0,
                             noise_std_extra_schedule_fn=lambda tt: 0.5, noise=t("chain_noise_guided", (T + n0 + 1, B, 64, D)).cuda()).cpu().numpy()
    np.testing.assert_allclose(chain, g["scaled_chain_opt0"], rtol=0, atol=2e-3)
    np.testing.assert_allclose(chain[-1], g["scaled_chain_opt0"][-1], rtol=0, atol=5e-4)
    gm = m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost, clip_grad=True, interpolate_trajectories_for_collision=True).cuda()
    chain = dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, ddim=True, guide=gm, n_guide_steps=3, t_start_guide=13,
                             noise=t("ddim_noise", (8, B, 64, D)).cuda()).cpu().numpy()
    ref = g["ddim_guided_chain_opt0"]
    assert chain.shape == ref.shape
    np.testing.assert_allclose(chain, ref, rtol=2e-4, atol=2e-4 * np.abs(ref).max())
