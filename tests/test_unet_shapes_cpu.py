"""CPU companions of tests/test_gpu_unet_shapes.py, on the case table of tests/shapes_ref.py: what mpdx_unet_create builds for every row (parameter
table, fused programs) and what it refuses, the oracle itself against the real reference's TemporalUnet on dim_mults the two shipped options do not
cover (tests/golden/unet_shapes.npz), and proof that the GPU cases can fail: three dataflow mistakes a kernel selected by layer shape could make in a
foreign network - half an identity residual over a concatenation, the neighbouring block's time-bias row, a residual taken from blocks.0's output -
each restated in the float32 oracle, miss regime_ref's forward bound by orders of magnitude."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import regime_ref as rr
import shapes_ref as S
from helpers import load_npz
from oracle import unet as ounet


@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _create(lib, H, W, mults, D=4):
    from mpd_public_amd import _lib
    cfg = _lib.UnetCfg(D, H, W, len(mults), (C.c_int32 * _lib.MAX_LEVELS)(*mults), 32)
    h = C.c_void_p()
    return lib.mpdx_unet_create(C.byref(cfg), C.byref(h)), h


# ---------------------------------------------------------------------------------------------- what the library builds
@pytest.mark.parametrize("name", [c[0] for c in S.CASES])
def test_row_is_created_with_the_reference_parameter_table_and_pinned_programs(lib, name):
    _, H, W, mults, D = S.ROWS[name]
    rc, h = _create(lib, H, W, mults, D)
    assert rc == 0, (name, lib.mpdx_last_error())
    got = {}
    for i in range(lib.mpdx_unet_num_params(h)):
        n, s, nd = C.c_char_p(), (C.c_int32 * 3)(), C.c_int32()
        assert lib.mpdx_unet_param_info(h, i, C.byref(n), C.byref(s), C.byref(nd)) == 0
        got[n.value.decode()] = tuple(s[: nd.value])
    want = ounet.unet_param_shapes(D, W, mults)
    assert got == want and list(got) != [] and {k: tuple(v.shape) for k, v in S.state_dict(name).items()} == want
    progs = []
    while lib.mpdx_unet_fused_program(h, len(progs)) != -2:
        progs.append(lib.mpdx_unet_fused_program(h, len(progs)))
    assert progs == S.PROGRAMS[name], (name, progs)
    assert lib.mpdx_train_flat_floats(h) > 0          # the training entry points accept the handle
    row = lib.mpdx_unet_timetab_floats(h, 1)
    assert row == sum(v[0] for k, v in want.items() if k.endswith("cond_mlp.1.bias")) and row <= 4608   # csrc/train.hpp kTimeBwdMaxRow (five: 2944)
    lib.mpdx_unet_destroy(h)


def test_python_module_tree_matches_the_oracle_for_every_row():
    import mpd_public_amd as m
    for name, H, W, mults, D in S.CASES:
        net = m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=W, dim_mults=mults)
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == ounet.unet_param_shapes(D, W, mults), name
        net.load_state_dict(S.state_dict(name), strict=True)


@pytest.mark.parametrize("H,W,mults,word", S.REFUSED)
def test_refusals_name_the_layer(lib, H, W, mults, word):
    import mpd_public_amd as m
    rc, _ = _create(lib, H, W, mults)
    msg = lib.mpdx_last_error().decode()
    assert rc < 0 and msg.startswith("layer ") and word in msg, (mults, rc, msg)
    with pytest.raises(RuntimeError, match="layer "):
        m.TemporalUnet(n_support_points=H, state_dim=4, unet_input_dim=W, dim_mults=mults)


def test_halving_rows_are_refused_for_the_identity_residual(lib):
    """(1,2,1) and (1,4,2): ups.0.0 reads 2 x 32 (2 x 64) channels and writes 64 (128), so the reference builds it without residual_conv and adds the
    WHOLE concatenation.  Every layer here names one residual slot of C_out channels: refused at create, by the C ABI and by the Python constructor."""
    import mpd_public_amd as m
    for name, H, W, mults, D in S.ORACLE_ONLY:
        assert "ups.0.0.residual_conv.weight" not in S.state_dict(name) and S.state_dict(name)["ups.0.0.blocks.0.block.0.weight"].shape[:2] == (W * mults[1],) * 2
        rc, _ = _create(lib, H, W, mults, D)
        assert rc < 0 and b"ups.0.0" in lib.mpdx_last_error() and b"identity residual over a concatenation" in lib.mpdx_last_error()
        with pytest.raises(RuntimeError, match="identity residual over a concatenation"):
            m.TemporalUnet(n_support_points=H, state_dim=D, unet_input_dim=W, dim_mults=mults)


# ---------------------------------------------------------------------------------------------- the oracle against the real reference
@pytest.mark.parametrize("name", S.GOLDEN_ROWS)
def test_oracle_reproduces_the_reference_on_other_multipliers(golden_dir, name):
    """tests/golden/make_golden.py --only unet_shapes: the reference's own TemporalUnet, B = 2, t = 0 and 37"""
    g = load_npz(golden_dir / "unet_shapes.npz")
    for tv in S.GOLDEN_T:
        y = ounet.unet_forward(S.state_dict(name), S.x_in(name, 2), S.tvec(2, tv)).numpy()
        ref = g[f"{name}_t{tv}"]
        assert ref.shape == y.shape and float(np.abs(ref).max()) > 0.1
        np.testing.assert_allclose(y, ref, rtol=0, atol=2e-6, err_msg=f"{name} t={tv}")


# ---------------------------------------------------------------------------------------------- the checks have teeth
def _wrong_rtb(at, kind):
    """oracle.unet.residual_temporal_block with ONE dataflow mistake in the block `at`:
      half-residual   an identity residual over a concatenation keeps its first half only (the rest reads as zero)
      neighbour-time  the time bias comes from the next block's cond_mlp (the row behind this block's in the time table)
      output-residual the identity residual is blocks.0's output (+ time bias), not the block's input"""
    def block(sd, p, x, temb):
        if p != at:
            return _RTB(sd, p, x, temb)
        q = p
        if kind == "neighbour-time":
            q = p[:-1] + "1" if p.endswith(".0") else "mid_block2"
            assert sd[q + ".cond_mlp.1.bias"].shape == sd[p + ".cond_mlp.1.bias"].shape
        tb = F.linear(F.mish(temb), sd[q + ".cond_mlp.1.weight"], sd[q + ".cond_mlp.1.bias"])
        h0 = ounet.conv1d_block(sd, p + ".blocks.0", x) + tb[:, :, None]
        h = ounet.conv1d_block(sd, p + ".blocks.1", h0)
        if (p + ".residual_conv.weight") in sd:
            res = F.conv1d(x, sd[p + ".residual_conv.weight"], sd[p + ".residual_conv.bias"])
        else:
            res = x
        if kind == "half-residual":
            assert (p + ".residual_conv.weight") not in sd
            res = torch.cat((x[:, : x.shape[1] // 2], torch.zeros_like(x[:, x.shape[1] // 2:])), dim=1)
        if kind == "output-residual":
            assert (p + ".residual_conv.weight") not in sd
            res = h0
        return h + res
    return block


_RTB = ounet.residual_temporal_block


def _misses(name, at, kind, B=3):
    """(missed the forward bound?, ratio) of the float32 oracle with the mistake, against the float64 oracle of the row"""
    sd, x, tv = S.state_dict(name), S.x_in(name, B), S.tvec(B)
    ref = rr.forward_ref(sd, x, tv)
    ounet.residual_temporal_block = _wrong_rtb(at, kind) if kind else _RTB
    try:
        with rr.one_thread():
            y = ounet.unet_forward(sd, x, tv)
    finally:
        ounet.residual_temporal_block = _RTB
    ratio, err, e_ref, floor = rr.forward_ratio(y, ref)
    print(f"{name} {at} {kind}: err {err:.3e} e_ref {e_ref:.3e} floor {floor:.3e} ratio {ratio:.3g}")
    return not err <= rr.K * e_ref + floor, ratio, err


@pytest.mark.parametrize("name", [c[0] for c in S.ORACLE_ONLY])
def test_half_an_identity_residual_over_a_concatenation_is_caught(name):
    """what build_model's `res = src1` would have computed for the halving rows: far outside the bound (about 5e-6)"""
    missed, ratio, err = _misses(name, "ups.0.0", "half-residual")
    assert missed and err > 1e-2, (ratio, err)
    assert not _misses(name, "ups.0.0", None)[0]


@pytest.mark.parametrize("name,at", [("four-256", "downs.3.0"), ("four-128", "downs.3.0"), ("five", "mid_block1"), ("rep-first", "downs.1.0")])
def test_time_bias_of_the_neighbouring_block_is_caught(name, at):
    """four-256: the seven-layer window starts at downs.3.0.blocks.0, whose time-bias row the run must take from downs.3.0, not from the block the
    standard network's window starts behind"""
    missed, ratio, err = _misses(name, at, "neighbour-time")
    assert missed and ratio > 100, (ratio, err)


@pytest.mark.parametrize("name,at", [("rep-first", "downs.1.0"), ("rep-last", "downs.2.0"), ("four-256", "downs.3.0"), ("five", "downs.4.0")])
def test_residual_from_the_block_output_is_caught(name, at):
    """an identity residual on the FIRST block of a level (repeated multipliers): the pair kernels and the run's tile-major hand-over have only met a
    residual_conv there; a residual read from blocks.0's output slot instead of the level's input misses the bound"""
    missed, ratio, err = _misses(name, at, "output-residual")
    assert missed and ratio > 100, (ratio, err)


def test_rows_meet_their_own_bound_in_float32_and_e_ref_is_what_the_bounds_assume():
    """the unmodified float32 oracle is inside the bound by construction (ratio <= 1); e_ref of these rows under `plain` is of the order 1e-6, so the
    forward bound K e_ref + 2^-23 max|y64| comes to a few 1e-6"""
    for name in ("two", "rep-first", "four-128"):
        sd, x, tv = S.state_dict(name), S.x_in(name, 3), S.tvec(3)
        ref = rr.forward_ref(sd, x, tv)
        assert 1e-7 < ref["e_ref"] < 5e-6 and 0.5 < ref["ymax"] < 5.0, (name, ref["e_ref"], ref["ymax"])
        assert rr.K * ref["e_ref"] + 2.0 ** -23 * ref["ymax"] < 2e-5
