"""The device random streams against tests/philox_ref.py (Philox4x32-10 and the mappings include/mpdx.h documents, restated in float64):
mpdx_randn element by element, the host's stream bookkeeping (fill_randn, the plan's x_T), and the training pass's device draws of the
timesteps and the noise (mpdx_train_draw), step by step.

Tolerance of a normal: a wrong bit anywhere in the generator moves a value by O(1); what separates a correct float32 Box-Muller from the float64
one is the rounding of u and of 2 pi u (together <= 4.3e-7 in the angle) times r <= 5.89, plus a few ulp of logf / sqrtf / sincosf: 2-5e-6 at
the tail.  Bound 1e-5.  Measured on an MI355X: 2.7e-6 over 4 x 2^20 + 7 elements, 1.2e-6 ... 1.8e-6 on the small shapes, 1.7e-6 ... 2.0e-6 on the training
draws.  (Before philox_radius evaluated u -> 1 by a series the large shape measured 2.6e-5: float32 rounding of k + 0.5, magnified by 1 / r - DESIGN.md
section 6, tests/test_philox_ref_cpu.py::test_float32_radius_near_u_equal_one.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as pr
from helpers import synth_sd, t, DIM_MULTS

pytestmark = pytest.mark.gpu

TOL = 1e-5
SEEDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)          # the key's low word, its high word, both
SENTINEL = 777.0


def _randn(n, seed, offset, pad=9):
    """mpdx_randn through the C ABI into a buffer padded with a sentinel -> (values [n], padding [pad]) on the host"""
    from mpd_public_amd import _lib
    buf = torch.full((n + pad,), SENTINEL, device="cuda")
    _lib.check(_lib.load().mpdx_randn(buf.data_ptr(), n, C.c_uint64(seed), C.c_uint64(offset), _lib.current_stream()), "mpdx_randn")
    h = buf.cpu().numpy()
    return h[:n].astype(np.float64), h[n:]


def _check(n, seed, offset):
    got, pad = _randn(n, seed, offset)
    assert (pad == SENTINEL).all(), f"n={n}: written behind the last element"
    err = float(np.abs(got - pr.randn(n, seed, offset)).max())
    assert err <= TOL, f"n={n} seed={seed:#x} offset={offset:#x}: max|z_gpu - z_ref64| = {err:.3e}"
    return err


# (counter offset, sizes): a ragged last quad at every residue, one block and several; the low word's carry inside one launch; a live high
# word; the 64-bit wrap-around (counters only: no large buffers)
OFFSETS = ((0, (1, 3, 4, 5, 1023)), (1, (5,)), (2 ** 32 - 3, (37,)), (2 ** 40 + 5, (5, 1023)), (2 ** 64 - 2, (16,)))


@pytest.mark.parametrize("seed", SEEDS)
def test_randn_elements_equal_the_reference(seed):
    worst = max(_check(n, seed, off) for off, sizes in OFFSETS for n in sizes)
    print(f"seed {seed:#x}: max|z_gpu - z_ref64| = {worst:.3e}")


def test_randn_grid_stride_loop_and_ragged_tail():
    """The launch caps its grid at 4096 blocks of 256 threads: 2^20 quads.  4 * 2^20 + 7 elements are the one shape that enters the
    grid-stride loop and ends in a ragged quad; the offset puts the low counter word's carry at the quads the loop's second trip draws."""
    n = 4 * 2 ** 20 + 7
    worst = _check(n, 2 ** 64 - 1, 2 ** 32 - 2 ** 20)
    print(f"n = {n}: max|z_gpu - z_ref64| = {worst:.3e}")


def _dm(D, opt, T, H=64):
    import mpd_public_amd as m
    net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=32, dim_mults=DIM_MULTS[opt])
    net.load_state_dict(synth_sd(D, opt), strict=True)
    return m.GaussianDiffusionModel(model=net, n_diffusion_steps=T, predict_epsilon=True, loss_type="l2").cuda()


def test_fill_randn_advances_the_stream_by_quads():
    seed = 0x1234567 << 32 | 99
    dm = _dm(4, 0, 25).manual_seed(seed)
    a, b = dm.fill_randn(torch.empty(5, device="cuda")), dm.fill_randn(torch.empty(7, device="cuda"))
    assert dm._rng_offset == 4                     # 5 elements take two counters, 7 take two more
    assert float(np.abs(a.cpu().numpy() - pr.randn(5, seed, 0)).max()) <= TOL
    assert float(np.abs(b.cpu().numpy() - pr.randn(7, seed, 2)).max()) <= TOL


@pytest.mark.parametrize("in_kernel", [False, True])
def test_plan_starts_from_the_stream_and_consumes_its_share(in_kernel):
    """An unguided plan with device noise: x_T is the stream's first B H D elements at the offset the model stood at, and the plan leaves
    the offset (steps + 1) B H D / 4 counters further - whether the steps' noise is pre-generated or drawn inside the step kernels."""
    D, T, n0, B, H = 4, 25, 5, 2, 64
    seed, off0 = 2 ** 63 + 12345, 2 ** 32 - 7       # the plan's stream crosses the low word's carry
    dm = _dm(D, 0, T).eval().manual_seed(seed)
    dm._rng_offset = off0
    if in_kernel:
        dm.in_kernel_noise_min_bytes = 0
    hc = {0: t("rng_plan_hc0", (D,), "uniform", 0.6).cuda(), H - 1: t("rng_plan_hc1", (D,), "uniform", 0.6).cuda()}
    chain = dm.run_inference(None, hc, n_samples=B, horizon=H, return_chain=True, n_diffusion_steps_without_noise=n0)
    n = B * H * D
    assert tuple(chain.shape) == (T + n0 + 1, B, H, D) and dm._rng_offset == off0 + (T + n0 + 1) * n // 4
    err = np.abs(chain[0].cpu().numpy().astype(np.float64) - pr.randn(n, seed, off0).reshape(B, H, D))[:, 1:H - 1]
    assert float(err.max()) <= TOL, float(err.max())


@pytest.mark.parametrize("B,H,D,T,opt", [(6, 64, 4, 25, 1), (5, 64, 14, 100, 1),
                                         (3, 128, 24, 25, 0)])   # H D / 4 = 768 quads per sample: beyond the draw loop's 512 threads
def test_training_draws_equal_the_reference(B, H, D, T, opt):
    """TrainStep.step without t / noise draws both on the device (mpdx_train_draw).  For every replayed step k (the device-resident step
    count the draw was armed with, read before the step): t[b] is EXACTLY randint(seed ^ K_TIMESTEP, k B + b, T), and quad q of sample b's
    noise is normal4(seed ^ K_NOISE, (k B + b) (H D / 4) + q) - two key domains, a stream position that advances by B per step."""
    from mpd_public_amd.trainer import TrainStep
    seed = 0x5DEECE66D1234567
    dm = _dm(D, opt, T, H).manual_seed(seed)
    x0 = t(f"rng_train_x0_{H}_{D}", (B, H, D), "uniform", 0.8).cuda()
    hc = {0: t(f"rng_train_hc0_{D}", (B, D), "uniform", 0.7).cuda(), H - 1: t(f"rng_train_hc1_{D}", (B, D), "uniform", 0.7).cuda()}
    ts = TrainStep(dm)
    nq, ks, worst = H * D // 4, [], 0.0
    for _ in range(8):
        k = int(ts.scratch.view(torch.int32)[4])
        loss = float(ts.step(x0, hc, 1e-3, max_norm=1.0, use_graph=True))
        assert np.isfinite(loss)
        if not getattr(ts, "_graphs", None):
            continue                                # (the first two calls run eagerly)
        g = next(iter(ts._graphs.values()))
        tt, nz = g["t"].cpu().numpy(), g["noise"].cpu().numpy().astype(np.float64).reshape(B, nq, 4)
        pos = k * B + np.arange(B)
        np.testing.assert_array_equal(tt, pr.randint(seed ^ pr.K_TIMESTEP, pos.astype(np.uint64), T), err_msg=f"step {k}")
        ctr = (pos[:, None] * nq + np.arange(nq)[None, :]).astype(np.uint64)
        err = float(np.abs(nz - pr.normal4(seed ^ pr.K_NOISE, ctr)).max())
        assert err <= TOL, f"step {k}: max|noise_gpu - ref64| = {err:.3e}"
        worst = max(worst, err)
        ks.append(k)
    assert len(ks) >= 5 and ks == list(range(ks[0], ks[0] + len(ks))), ks       # consecutive replays: consecutive stream positions
    print(f"B={B} H={H} D={D}: steps {ks}, max|noise_gpu - ref64| = {worst:.3e}")
