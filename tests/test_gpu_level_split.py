"""The paired form of mpdx_plan's joined launch (csrc/fused_level.hpp fused_join_split_kernel): the 128-channel down level of the joined kernel on two
compute units per trajectory.  A wave still owns a whole 16 x 16 tile for the whole K and a GroupNorm group is one tile, so everything here is
BIT-identical with the handle option (mpdx_unet_set_level_split) on and off.  Shapes as in test_gpu_plan_join.py: H = 64, T = 4 + 2."""
import pytest
import torch

from helpers import synth_sd, t, DIM_MULTS, product_guide

pytestmark = pytest.mark.gpu

H = 64
T, N0 = 4, 2
_models = {}


def _model(D, opt=1, horizon=H):
    """one model (one handle: one exchange area, one set of counters) per network for the whole module"""
    key = (D, opt, horizon)
    if key not in _models:
        import mpd_public_amd as m
        from mpd_public_amd import synthetic as syn
        net = m.TemporalUnet(n_support_points=horizon, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
        sd = synth_sd(D, opt) if horizon == H else syn.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
        net.load_state_dict(sd, strict=True)
        dm = m.GaussianDiffusionModel(model=net.cuda().eval(), variance_schedule="cosine", n_diffusion_steps=T, predict_epsilon=True)
        _models[key] = dm.cuda().eval()
    return _models[key]


def _hc(D, horizon=H):
    return {0: t("split_hc0", (D,), "uniform", 0.6).cuda(), horizon - 1: t("split_hc1", (D,), "uniform", 0.6).cuda()}


def _plan(dm, split, hc, B, horizon=H, seed=None, **kw):
    """(x, chain, joined launches, paired launches) of one fused plan with the option set to `split`; the handle's status is 0 afterwards"""
    dm.model.set_plan_join(True)
    dm.model.set_level_split(split)
    if seed is not None:
        dm.in_kernel_noise_min_bytes = 0    # the in-kernel draw, not a pre-generated tensor
        dm.manual_seed(seed)
        dm._rng_offset = 5
    x, chain = dm.plan(hc, B, horizon, noise_std_extra_schedule_fn=lambda tt: 0.5, n_diffusion_steps_without_noise=N0, **kw)
    torch.cuda.synchronize()
    assert dm.model.status() == 0
    return x, chain, dm.model.plan_joined(), dm.model.plan_split()


def _noise_kw(name, B, D, in_kernel_noise, horizon=H):
    return dict(seed=4321) if in_kernel_noise else dict(noise=t(name, (T + N0 + 1, B, horizon, D)).cuda())


@pytest.mark.parametrize("in_kernel_noise", [False, True])
@pytest.mark.parametrize("D", [4, 14])
def test_split_equals_unsplit(D, in_kernel_noise):
    """One trajectory, an odd count, the nb8 round-up boundary (8 | 9: surplus blocks leave), two groups of 8 (16 | 17).  Growing and shrinking batches on
    one handle: the counters are re-zeroed when the batch grows, their base advances otherwise."""
    dm = _model(D)
    for B in (1, 2, 3, 8, 9, 16, 17):
        kw = _noise_kw(f"split_noise_D{D}_B{B}", B, D, in_kernel_noise)
        xa, ca, ja, sa = _plan(dm, True, _hc(D), B, **kw)
        xb, cb, jb, sb = _plan(dm, False, _hc(D), B, **kw)
        assert ja == jb == T + N0 - 1 and sa == ja and sb == 0, (B, ja, jb, sa, sb)   # every iteration but the last is joined, and paired
        assert torch.isfinite(ca).all() and float(ca[1].std()) > 0.1 and not torch.equal(ca[1], ca[2]), B
        assert torch.equal(ca, cb) and torch.equal(xa, xb), B


@pytest.mark.parametrize("panda", [False, True])
def test_guided_plan_split_equals_unsplit(panda):
    """The transitions of test_guided_plan_joined_equals_separate: B = 4 in two contexts, guide from t < 2 - unguided -> unguided and unguided -> guided are
    joined (paired), guided -> guided is not."""
    import mpd_public_amd as m
    D, B, npc = (14 if panda else 4), 4, 2
    ds = m.TrajectoryDataset("EnvSpheres3D" if panda else "EnvDense2D", "RobotPanda" if panda else "RobotPointMass",
                             tensor_args={"device": "cuda", "dtype": torch.float32})
    dm = _model(D)
    hc = {0: t("split_ctx_hc0", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0),
          H - 1: t("split_ctx_hc1", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0)}
    kw = dict(noise=t(f"split_noise_guided_{D}", (T + N0 + 1, B, H, D)).cuda(), guide=product_guide(ds).cuda(), n_guide_steps=2, t_start_guide=2,
              n_per_context=npc)
    xa, ca, ja, sa = _plan(dm, True, hc, B, **kw)
    fa = dm.last_guide_flags.clone()
    xb, cb, jb, sb = _plan(dm, False, hc, B, **kw)
    fb = dm.last_guide_flags.clone()
    assert (ja, sa, jb, sb) == (2, 2, 2, 0)
    assert torch.isfinite(ca).all() and not torch.equal(ca[-1], ca[-2])
    assert torch.equal(ca, cb) and torch.equal(xa, xb)
    assert fa.numel() == (T + N0) * 3 * (B // npc) and torch.equal(fa, fb)


def test_largest_batch_is_paired_the_next_is_not():
    """B = 128: 2 x 128 workgroups, one per compute unit.  B = 129 would need 2 x 136: the joined launch as it was."""
    D = 4
    dm = _model(D)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (128, 129):
        kw = _noise_kw(f"split_noise_big_B{B}", B, D, False)
        xa, ca, ja, sa = _plan(dm, True, _hc(D), B, **kw)
        xb, cb, jb, sb = _plan(dm, False, _hc(D), B, **kw)
        joined = T + N0 - 1 if B <= cus else 0
        assert ja == jb == joined and sb == 0
        assert sa == (joined if 2 * 8 * -(-B // 8) <= cus else 0), (B, sa, cus)
        assert torch.isfinite(ca).all() and torch.equal(ca, cb) and torch.equal(xa, xb)


@pytest.mark.parametrize("opt,horizon", [(0, 64), (1, 48)])
def test_networks_without_the_joined_launch_are_never_paired(opt, horizon):
    """A three-level network (other programs) and a horizon of 48 in a zero-padded container (no programs): no joined launch, so no paired one."""
    D, B = 4, 3
    dm = _model(D, opt, horizon)
    kw = _noise_kw(f"split_noise_fb_{opt}_{horizon}", B, D, False, horizon)
    xa, ca, ja, sa = _plan(dm, True, _hc(D, horizon), B, horizon, **kw)
    xb, cb, jb, sb = _plan(dm, False, _hc(D, horizon), B, horizon, **kw)
    assert (ja, sa, jb, sb) == (0, 0, 0, 0)
    assert torch.isfinite(ca).all() and torch.equal(ca, cb) and torch.equal(xa, xb)


def test_back_to_back_plans_then_a_larger_batch():
    """Two plans on one handle (the counters are not reset: the second starts from the first's base + 9 per launch), then a larger batch (the counters are
    zeroed), then the first batch again: all equal to the unpaired plans."""
    D = 4
    dm = _model(D)
    ref = {}
    for B in (5, 12):
        kw = _noise_kw(f"split_noise_b2b_B{B}", B, D, False)
        ref[B] = (kw, _plan(dm, False, _hc(D), B, **kw))
    for B in (5, 5, 12, 5):
        kw, (xb, cb, jb, sb) = ref[B]
        xa, ca, ja, sa = _plan(dm, True, _hc(D), B, **kw)
        assert sa == ja == jb == T + N0 - 1 and sb == 0
        assert torch.equal(ca, cb) and torch.equal(xa, xb), B
