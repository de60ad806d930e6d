"""The oracle's restatement of the self-attention block (oracle/unet.py: linear_attention_block, and unet_forward on a state dict that carries the
blocks) pinned against the vectors the REAL reference produced (tests/golden/attention.npz), and the block-level cases of tests/attn_ref.py shown
to tell deliberately wrong variants of the block apart.  No GPU."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import attn_ref as ar
from helpers import t, load_npz
from mpd_public_amd import synthetic as syn
from oracle import diffusion as odiff, unet as ounet

GOLDEN = Path(__file__).parent / "golden"
# (H, D, unet_input_dim, dim_mults) of make_golden_attention.py::CASES
CASES = ((64, 4, 32, (1, 2, 4, 8)), (64, 14, 32, (1, 2, 4)), (24, 6, 32, (1, 2, 4)), (40, 2, 32, (1, 2, 4, 8)), (128, 4, 32, (1, 2, 4)),
         (64, 4, 64, (1, 2, 4)))


def case_tag(H, D, uid, mults):
    return f"H{H}_D{D}_w{uid}_m{''.join(str(m) for m in mults)}"


@functools.lru_cache(maxsize=None)
def golden():
    return load_npz(GOLDEN / "attention.npz")


def attn_sd(D, uid, mults, dt=torch.float32):
    return {k: v.to(dt) for k, v in syn.synth_state_dict(ounet.unet_param_shapes(D, uid, mults, self_attention=True)).items()}


def test_param_shapes_with_self_attention_match_the_reference_layout():
    ref = []
    for line in (GOLDEN / "state_dict_keys_attention.txt").read_text().splitlines():
        cfg, key, *shape = line.split()
        if key.startswith("model."):
            ref.append((key[len("model."):], tuple(int(s) for s in shape[0].split("x")) if shape else ()))
    got = ounet.unet_param_shapes(4, 32, (1, 2, 4, 8), self_attention=True)
    assert len(ref) == 236 and got == dict(ref)
    plain = ounet.unet_param_shapes(4, 32, (1, 2, 4, 8))
    assert len(plain) == 196 and len(got) - len(plain) == 40 and all(got[k] == v for k, v in plain.items())   # the default is what it was
    assert [k for k in got if k in plain] == list(plain)


@pytest.mark.parametrize("case", CASES, ids=[case_tag(*c) for c in CASES])
def test_unet_forward_with_attention_matches_reference_golden(case):
    H, D, uid, mults = case
    tag, g = case_tag(*case), golden()
    sd32, sd64 = attn_sd(D, uid, mults), attn_sd(D, uid, mults, torch.float64)
    x = t(f"attn_x_{tag}", (3, H, D))
    ts = [(f"t{tt}", torch.full((3,), tt, dtype=torch.long)) for tt in (0, 12, 24)]
    if case == CASES[0]:
        ts.append(("mixed", torch.tensor([3, 24, 0])))
    for name, tt in ts:
        y32 = ounet.unet_forward(sd32, x, tt).numpy()
        y64 = ounet.unet_forward(sd64, x.double(), tt).numpy()
        e64 = np.abs(y64 - g[f"{tag}_{name}_f64"]).max()
        print(f"{tag} {name}: max|oracle32 - ref32| = {np.abs(y32 - g[f'{tag}_{name}_f32']).max():.3e}   max|oracle64 - ref64| = {e64:.3e}")
        # the same ATen operations in the same order as the reference's modules: the same bits
        np.testing.assert_array_equal(y32, g[f"{tag}_{name}_f32"])
        # fp64: the oracle builds the sinusoidal frequencies in fp32 (the reference's fp64 run builds them in fp64), nothing else differs.
        # Largest difference measured over the six cases and four timestep forms: FP64_MEASURED; the bound is 4 x that
        assert e64 <= 4 * FP64_MEASURED, (tag, name, e64)


FP64_MEASURED = 7e-8


def test_a_plain_state_dict_runs_without_the_blocks():
    """unet_forward on a state dict without attention keys is the network it always was; the attention keys change the result"""
    H, D, uid, mults = CASES[0]
    sd = attn_sd(D, uid, mults)
    plain = {k: v for k, v in sd.items() if ".fn." not in k}
    assert set(plain) == set(ounet.unet_param_shapes(D, uid, mults))
    x, tt = t("attn_x_" + case_tag(*CASES[0]), (3, H, D)), torch.full((3,), 12, dtype=torch.long)
    effect = float((ounet.unet_forward(sd, x, tt) - ounet.unet_forward(plain, x, tt)).abs().max())
    assert effect >= 0.05, effect


def test_chain_with_attention_matches_reference_golden():
    """oracle.diffusion.run_inference takes the network as a state dict: the attention network needs nothing further"""
    g = golden()
    H, D, uid, mults = CASES[0]
    T, n0, B = 25, 5, 4
    noise = t("attn_chain_noise", (T + n0 + 1, B, H, D))
    hc = {0: t("attn_chain_hc0", (D,), "uniform", 0.6), H - 1: t("attn_chain_hc1", (D,), "uniform", 0.6)}
    c32 = odiff.run_inference(attn_sd(D, uid, mults), hc, noise, T, n_diffusion_steps_without_noise=n0, noise_std=0.5).numpy()
    err = np.abs(c32 - g["chain_f32"]).reshape(c32.shape[0], -1).max(1)
    print(f"chain fp32: max|oracle - ref| per row {err}")
    np.testing.assert_array_equal(c32, g["chain_f32"])   # the same ATen operations in the same order, all 31 rows
    c64 = odiff.run_inference(attn_sd(D, uid, mults, torch.float64), {k: v.double() for k, v in hc.items()}, noise.double(), T,
                              n_diffusion_steps_without_noise=n0, noise_std=0.5, dtype=torch.float64).numpy()
    e64 = np.abs(c64[-1] - g["chain_final_f64"]).max()
    e32 = np.abs(g["chain_f32"][-1].astype(np.float64) - g["chain_final_f64"]).max()
    print(f"chain fp64: final row max|oracle64 - ref64| = {e64:.3e}   (the reference's own max|f32 - f64| there = {e32:.3e})")
    # measured 1.8e-7 (the fp32 sinusoidal frequencies again, through 30 steps; the reference's own fp32 chain is 3.4e-6 away); bound 4 x that
    assert e64 <= 4 * 1.8e-7, (e64, e32)


# ------------------------------------------------------------------------------------ the block-level cases (tests/attn_ref.py)
def small_batch(shape):
    return tuple(range(min(3, max(ar.SHAPES[shape]))))


def test_variant_none_is_the_oracle_block_bit_for_bit():
    for case in ar.CASES[::7]:
        shape, regime = case
        sd, x = ar.block_params(shape[0], regime), ar.block_input(shape, regime, small_batch(shape))
        assert torch.equal(ar.block_variant(sd, x, shape[1]), ounet.linear_attention_block(sd, ar.P, x)), ar.case_id(case)
        sd64 = ar.to_dtype(sd, torch.float64)
        assert torch.equal(ar.block_variant(sd64, x.double(), shape[1]), ounet.linear_attention_block(sd64, ar.P, x.double()))


def test_case_table_covers_every_row_in_the_plain_regime_and_the_refusals_are_refused():
    from mpd_public_amd import _lib
    assert {s for s, r in ar.CASES if r == "plain"} == set(ar.SHAPES) and set(ar.REGIME_SHAPES) <= set(ar.SHAPES)
    assert {r for _, r in ar.CASES} == set(ar.REGIMES)
    lib = _lib.load()
    dummy = 16   # never dereferenced: the refusal comes before any launch
    for C, L, Lv in ar.REFUSED:
        assert lib.mpdx_attention_block(dummy, dummy, dummy, dummy, dummy, dummy, 1, L, Lv, C, None) == -1, (C, L, Lv)
        assert b"self-attention block" in lib.mpdx_last_error()
    for bad in (dict(B=0), dict(Lv=0), dict(Lv=9)):
        kw = dict(B=1, L=8, Lv=8, C=256)
        kw.update(bad)
        assert lib.mpdx_attention_block(dummy, dummy, dummy, dummy, dummy, dummy, kw["B"], kw["L"], kw["Lv"], kw["C"], None) == -1, bad
    assert lib.mpdx_attention_block(None, dummy, dummy, dummy, dummy, dummy, 1, 8, 8, 256, None) == -1


@pytest.mark.parametrize("variant", ar.VARIANTS)
def test_block_cases_tell_a_wrong_variant_apart(variant):
    """A restatement with ONE deliberate mistake, evaluated in fp32, must miss the bound of the GPU test (K e_ref + 2^-23 max|y|, from the
    reference alone) or be non-finite on at least one case of the table: the inputs can fail."""
    hits = []
    for case in ar.CASES:
        shape, regime = case
        if variant == "all_positions" and shape[1] == shape[2]:
            continue
        bs = small_batch(shape)
        y64, e_ref, bound = ar.reference(shape, regime, bs)
        y = ar.block_variant(ar.block_params(shape[0], regime), ar.block_input(shape, regime, bs), shape[1], variant)
        err = float((y.double() - y64).abs().max())
        if not np.isfinite(err) or err > bound:
            hits.append((ar.case_id(case), err, bound))
    print(f"{variant}: separated on {len(hits)} cases; first {hits[:3]}")
    assert hits, variant
