"""The width of mpdx_plan's two persistent runs (csrc/inner_run.hpp): a cluster of 8 workgroups owns 4 whole trajectories (width 32, one workgroup per
compute unit) or 2 (width 16, up to two per compute unit).  The K split over the eight waves, the fixed-order reduction and the per-region GroupNorm do
not depend on the width, so every comparison is torch.equal against the same plan with the runs off, on the same handle and noise, at width 16, 32 and
0 (automatic).  mpdx_unet_inner_runs / _inner_run_layers keep their values at every width (7 and 4 layers per pass).  After every plan the handle's
status word is 0 and the outputs are finite.  No test drives the give-up path."""
import pytest
import torch

import test_gpu_inner_run_tail as M
from helpers import t, product_guide

pytestmark = pytest.mark.gpu

H, N0, P = M.H, M.N0, M.P
SEVEN, TAIL = M.SEVEN, M.TAIL
WIDTHS = [16, 32, 0]


@pytest.fixture(autouse=True)
def _defaults_after():
    """the models are shared with the other run tests: every test leaves them at the default width with both runs selected"""
    yield
    for dm in M._MODELS.values():
        dm.model.set_inner_run_width(0)
        dm.model.set_inner_run(True)
        dm.model.set_plan_join(True)


def _plan(dm, width, parts, hc, B, **kw):
    dm.model.set_inner_run_width(width)
    return M._plan(dm, parts, hc, B, **kw)


def _same(got, ref, what):
    assert torch.equal(got[0], ref[0]), what
    assert (got[1] is None) == (ref[1] is None) and (got[1] is None or torch.equal(got[1], ref[1])), what


def _widths_agree(dm, hc, B, parts=SEVEN | TAIL, selected=True, widths=WIDTHS, passes=P, **kw):
    """the plan with the runs off, then with `parts` at every width: the same bits, the counts the parts promise"""
    ref = _plan(dm, 0, 0, hc, B, **kw)
    assert ref[2:] == (0, 0)
    for w in widths:
        got = _plan(dm, w, parts, hc, B, **kw)
        assert got[2:] == M._counts(parts, passes, selected), (w, parts, got[2:])
        _same(got, ref, (w, parts, B))
    return ref[0], ref[1]


@pytest.mark.parametrize("in_kernel_noise", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 17, 100, 127, 128, 129])
@pytest.mark.parametrize("D", [4, 14])
def test_every_width_equals_per_layer_kernels(D, B, in_kernel_noise):
    """B = 1: half a narrow cluster; 2: one full narrow cluster; 3: a ragged second narrow cluster, one partly filled wide one; 4, 5; 17: a ragged
    ninth narrow cluster, the first beyond one group of 8 clusters; 100: the headline; 127, 128: the cap - two workgroups on every compute unit at
    width 16; 129: selected at no width.  With and without the chain, with plan-join on and off."""
    dm = M._model(D)
    for return_chain in (True, False):
        for join in (True, False):
            kw = dict(n_diffusion_steps_without_noise=N0, return_chain=return_chain, join=join)
            if in_kernel_noise:
                kw["seed"] = 4321
            else:
                kw["noise"] = M._noise(D, B)
            x, chain = _widths_agree(dm, M._hc(D), B, selected=B <= 128, **kw)
            assert float(x.std()) > 0.05
            if chain is not None:
                assert torch.equal(x, chain[-1]) and not torch.equal(chain[1], chain[2])


@pytest.mark.parametrize("parts", [SEVEN, TAIL])
@pytest.mark.parametrize("B", [3, 100])
def test_each_run_alone_at_width_16(parts, B):
    """the parts and the width are independent: seven alone (7 layers per pass) and the tail alone (4, no seven-layer launch) at width 16"""
    D = 4
    _widths_agree(M._model(D), M._hc(D), B, parts=parts, widths=[16], n_diffusion_steps_without_noise=N0, noise=M._noise(D, B))


def test_width_changes_between_plans_on_one_handle():
    """16 -> 32 -> 16 -> 0 at a fixed batch, then batches that grow and shrink across widths: a launch with more clusters than the one of its width
    before zeroes that width's counters, and every plan still starts from counters that agree."""
    D = 4
    dm = M._model(D, tag="narrow-resize")
    ref = {}
    for B, w in [(5, 16), (5, 32), (5, 16), (5, 0), (5, 32), (5, 16), (100, 16), (8, 32), (100, 32), (3, 16), (128, 16), (4, 0), (128, 32), (128, 16)]:
        kw = dict(n_diffusion_steps_without_noise=N0, noise=M._noise(D, B))
        if B not in ref:
            ref[B] = _plan(dm, 0, 0, M._hc(D), B, **kw)
        got = _plan(dm, w, SEVEN | TAIL, M._hc(D), B, **kw)
        assert got[2:] == (P, 11 * P), (B, w, got[2:])
        _same(got, ref[B], (B, w))


def test_two_handles_at_different_widths_taking_turns():
    """the counters and the width belong to the handle: a narrow and a wide handle alternating on one stream give what the per-layer kernels give"""
    D, B = 4, 8
    a, b = M._model(D, tag="narrow-a"), M._model(D, tag="narrow-b")
    assert a.model._handle().value != b.model._handle().value
    kw = dict(n_diffusion_steps_without_noise=N0, noise=M._noise(D, B))
    for dm, w in ((a, 16), (b, 32)):
        dm.model.set_inner_run(True)
        dm.model.set_plan_join(True)
        dm.model.set_inner_run_width(w)
    got = []
    for dm in (a, b, a, a, b, a, b, b):
        x, chain = dm.plan(M._hc(D), B, H, noise_std_extra_schedule_fn=lambda tt: 0.5, **kw)
        assert (dm.model.inner_runs(), dm.model.inner_run_layers()) == (P, 11 * P)
        got.append((x, chain))
    torch.cuda.synchronize()
    assert a.model.status() == 0 and b.model.status() == 0
    ref = _plan(a, 0, 0, M._hc(D), B, **kw)
    assert ref[2:] == (0, 0)
    for x, chain in got:
        assert torch.isfinite(x).all()
        _same((x, chain), ref, "alternating")


def test_guided_panda_plan_at_width_16():
    """B = 6 in three contexts, T = 4 + 2, guide from t < 2: the inner levels do not see the guide, so guided iterations take both narrow runs"""
    import mpd_public_amd as m
    D, B, npc = 14, 6, 2
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args={"device": "cuda", "dtype": torch.float32})
    dm = M._model(D)
    hc = {0: t("narrow_ctx_hc0", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0),
          H - 1: t("narrow_ctx_hc1", (B // npc, D), "uniform", 0.6).cuda().repeat_interleave(npc, 0)}
    kw = dict(n_diffusion_steps_without_noise=N0, noise=M._noise(D, B), guide=product_guide(ds).cuda(), n_guide_steps=2, t_start_guide=2, n_per_context=npc)
    ref = _plan(dm, 0, 0, hc, B, **kw)
    ref_flags = dm.last_guide_flags.clone()
    assert ref[2:] == (0, 0) and not torch.equal(ref[1][-1], ref[1][-2])
    got = _plan(dm, 16, SEVEN | TAIL, hc, B, **kw)
    assert got[2:] == (P, 11 * P)
    _same(got, ref, "guided")
    assert torch.equal(dm.last_guide_flags, ref_flags)


def test_set_inner_run_width_refuses_other_values():
    """-1, 8 and 64 are refused with a negative code and change nothing; 0 restores the automatic width"""
    from mpd_public_amd import _lib
    D, B = 4, 5
    dm = M._model(D)
    lib, h = _lib.load(), dm.model._handle()
    kw = dict(n_diffusion_steps_without_noise=N0, noise=M._noise(D, B))
    ref = _plan(dm, 0, 0, M._hc(D), B, **kw)
    assert lib.mpdx_unet_set_inner_run_width(h, 16) == 0
    for bad in (-1, 8, 64):
        assert lib.mpdx_unet_set_inner_run_width(h, bad) < 0, bad
    assert lib.mpdx_unet_set_inner_run_width(None, 16) < 0
    got = M._plan(dm, SEVEN | TAIL, M._hc(D), B, **kw)     # still at width 16
    assert got[2:] == (P, 11 * P)
    _same(got, ref, "after refused widths")
    assert lib.mpdx_unet_set_inner_run_width(h, 0) == 0
    got = M._plan(dm, SEVEN | TAIL, M._hc(D), B, **kw)
    assert got[2:] == (P, 11 * P)
    _same(got, ref, "automatic again")
