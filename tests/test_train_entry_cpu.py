"""The references the GPU tests of the training entry points lean on (tests/test_gpu_train_entry.py), pinned on the CPU before anything
on the device is held to them: the weighted loss of the oracle (oracle/diffusion.p_losses, oracle/train.loss_and_grads with `weights`)
and the float64 restatements of tests/train_entry_ref.py against torch's own optimiser."""
import numpy as np
import torch

import train_entry_ref as R
from helpers import synth_sd, t

D, OPT, T, B, H = 4, 0, 25, 2, 64


def _inputs():
    x0, noise = t("tecpu_x0", (B, H, D), "uniform", 0.8), t("tecpu_noise", (B, H, D))
    hc = {0: t("tecpu_hc0", (B, D), "uniform", 0.7), H - 1: t("tecpu_hc1", (B, D), "uniform", 0.7)}
    return x0, noise, hc, torch.tensor([3, 24])


def test_unit_weights_give_the_unweighted_loss_and_gradients_fp64():
    from oracle import train as otrain
    x0, noise, hc, tt = _inputs()
    sd = synth_sd(D, OPT)
    for lt in ("l2", "l1"):
        l0, g0 = otrain.loss_and_grads(sd, x0, tt, hc, noise, T, loss_type=lt, dtype=torch.float64)
        l1, g1 = otrain.loss_and_grads(sd, x0, tt, hc, noise, T, loss_type=lt, dtype=torch.float64, weights=torch.ones(H, D))
        assert abs(float(l1) - float(l0)) <= 1e-12 * abs(float(l0))
        worst = 0.0
        for k in g0:
            worst = max(worst, float((g1[k] - g0[k]).abs().max()) / float(g0[k].abs().max()))
        print(f"{lt}: unit weights vs unweighted, worst relative gradient difference {worst:.2e}")
        assert worst <= 1e-12


def test_no_weights_is_the_old_expression_bit_for_bit_fp32():
    from oracle import diffusion as odiff, schedules as osched, train as otrain
    from oracle.unet import unet_forward
    x0, noise, hc, tt = _inputs()
    sd = synth_sd(D, OPT)
    buf = osched.make_buffers(T, "exponential")
    x_noisy = odiff.apply_hard_conditioning(odiff.q_sample(buf, x0, tt, noise), hc)
    x_recon = odiff.apply_hard_conditioning(unet_forward(sd, x_noisy, tt), hc)
    old = {"l2": torch.nn.functional.mse_loss(x_recon, noise, reduction="none").mean(), "l1": (x_recon - noise).abs().mean()}
    for lt in ("l2", "l1"):
        assert torch.equal(odiff.p_losses(sd, x0, tt, hc, noise, T, loss_type=lt), old[lt])
        assert torch.equal(odiff.p_losses(sd, x0, tt, hc, noise, T, loss_type=lt, weights=None), old[lt])
        assert torch.equal(otrain.loss_and_grads(sd, x0, tt, hc, noise, T, loss_type=lt)[0], old[lt])
    # and the weights do act: a table of twos doubles the loss (exactly: a power of two)
    two = odiff.p_losses(sd, x0, tt, hc, noise, T, weights=torch.full((H, D), 2.0))
    assert torch.equal(two, 2.0 * old["l2"])


def test_zero_weight_columns_give_exactly_zero_gradient_rows_of_final_conv():
    from oracle import train as otrain
    x0, noise, hc, tt = _inputs()
    w = 0.1 + t("tecpu_w", (H, D), "uniform").abs()
    w[:, D // 2:] = 0.0
    for dtype in (torch.float32, torch.float64):
        _, g = otrain.loss_and_grads(synth_sd(D, OPT), x0, tt, hc, noise, T, dtype=dtype, weights=w)
        gw, gb = g["final_conv.1.weight"], g["final_conv.1.bias"]
        assert bool((gw[D // 2:] == 0).all()) and bool((gb[D // 2:] == 0).all())
        assert float(gw[:D // 2].abs().min(1).values.max()) > 0 and bool((gb[:D // 2] != 0).all())


def test_adam_ref_three_steps_vs_torch_adam_and_clip_grad_norm_fp64():
    """adam_ref chained over three steps against torch.optim.Adam + clip_grad_norm_ on float64 tensors (the scalars are fp32-representable,
    as adam_ref rounds them).  Measured: p' and v' 2e-15 relative element by element; m' 2e-15 of its largest element (b1 m and (1 - b1) g
    cancel in single elements when the gradient changes sign between steps: 5e-13 relative to such an element).  Asserted at 1e-14."""
    n = 1027
    lr, betas, eps = R.f32(1e-3), (R.f32(0.9), R.f32(0.999)), R.f32(1e-8)
    for max_norm, gscale in ((0.0, 1.0), (1.0, 1.0), (1.0, 1e-3)):   # no clipping / norm ~ 18 > 1: clips / norm < 1: does not
        p0 = t("tecpu_adam_p", (n,), "uniform", 0.5).double()
        prm = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([prm], lr=lr, betas=betas, eps=eps)
        p, m, v = p0.float(), torch.zeros(n), torch.zeros(n)
        pd, md, vd = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        worst = 0.0
        for step in (1, 2, 3):
            g = (gscale * t(f"tecpu_adam_g{step}", (n,), "uniform")).double()
            prm.grad = g.clone()
            norm_t = float(torch.nn.utils.clip_grad_norm_([prm], max_norm)) if max_norm > 0 else None
            opt.step()
            pd, md, vd, norm, coef = R.adam_ref(pd, g, md, vd, lr, betas, eps, step, max_norm)
            if norm_t is not None:
                assert abs(norm - norm_t) <= 1e-13 * norm_t
                assert (coef < 1.0) == (gscale == 1.0)
            st = opt.state[prm]
            for got, want, scale in ((pd, prm.detach(), None), (md, st["exp_avg"], st["exp_avg"].abs().max()), (vd, st["exp_avg_sq"], None)):
                worst = max(worst, float(((got - want).abs() / (want.abs().clamp_min(1e-300) if scale is None else scale)).max()))
        print(f"max_norm {max_norm} gscale {gscale}: adam_ref vs torch.optim.Adam over three steps, worst relative difference {worst:.2e}")
        assert worst <= 1e-14
    # the fp32-input form is the same function: one step from fp32 tensors equals the float64 arithmetic on their values
    g32 = t("tecpu_adam_g1", (n,), "uniform")
    a = R.adam_ref(p, g32, m, v, lr, betas, eps, 1, 1.0)
    b = R.adam_ref(p.double(), g32.double(), m.double(), v.double(), lr, betas, eps, 1, 1.0)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def test_adam_ref_rounds_the_scalars_to_fp32():
    p, g, z = torch.tensor([0.5]), torch.tensor([0.25]), torch.zeros(1)
    a = R.adam_ref(p, g, z, z, 1e-3, (0.9, 0.999), 1e-8, 2, 0.0)
    b = R.adam_ref(p, g, z, z, float(np.float32(1e-3)), (float(np.float32(0.9)), float(np.float32(0.999))), float(np.float32(1e-8)), 2, 0.0)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert float(a[2]) == (1.0 - float(np.float32(0.999))) * 0.0625


def test_ema_ref_vs_oracle_ema_update():
    from oracle import train as otrain
    beta = R.f32(0.995)
    ema, p = t("tecpu_ema", (1027,), "uniform"), t("tecpu_ema_p", (1027,), "uniform")
    want = otrain.ema_update({"w": ema.double()}, {"w": p.double()}, beta)["w"]
    got = R.ema_ref(ema, p, 0.995)
    assert float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()) <= 1e-15


def test_fp32_references_round_three_times():
    """q_sample_ref / add_noise_ref are the separately rounded fp32 operations (not a float64 value rounded once), clamp t and apply the ends"""
    x0, nz = t("tecpu_q_x0", (4, 8, 3), "uniform", 0.8), t("tecpu_q_nz", (4, 8, 3))
    a, b = t("tecpu_q_a", (5,), "uniform").abs(), t("tecpu_q_b", (5,), "uniform").abs()
    hs = t("tecpu_q_hs", (4, 3), "uniform")
    got = R.q_sample_ref(x0, nz, torch.tensor([-1, 5, 2 ** 40, 3]), a, b, hs, None)
    tc = torch.tensor([0, 4, 4, 3])
    want = (a[tc].reshape(-1, 1, 1) * x0) + (b[tc].reshape(-1, 1, 1) * nz)
    assert torch.equal(got[:, 1:], want[:, 1:]) and torch.equal(got[:, 0], hs)
    once = (a[tc].reshape(-1, 1, 1).double() * x0.double() + b[tc].reshape(-1, 1, 1).double() * nz.double()).float()
    assert not torch.equal(want, once)
    x = t("tecpu_an_x", (4, 8, 3))
    got = R.add_noise_ref(x, nz, None, hs, 0.3, 0.7)
    want = x + (torch.tensor(0.3) * nz) * torch.tensor(0.7)
    assert torch.equal(got[:, :-1], want[:, :-1]) and torch.equal(got[:, -1], hs)
    assert torch.equal(R.add_noise_ref(x, None, None, None, 0.3, 0.7), x)
    pred, targ, w = t("tecpu_wl_p", (4, 8, 3)), t("tecpu_wl_t", (4, 8, 3)), 0.1 + t("tecpu_wl_w", (8, 3), "uniform").abs()
    p2 = pred.clone(); p2[:, 0] = hs
    for l1 in (0, 1):
        e = (p2 - targ).double()
        want = float(((e.abs() if l1 else e * e) * w.double()).mean())
        assert abs(R.weighted_loss_ref(pred, targ, w, hs, None, l1) - want) <= 2e-7 * want
