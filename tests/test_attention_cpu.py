"""TemporalUnet(self_attention=True), host side (no GPU: a handle is host-side metadata): the reference's module tree and state-dict layout,
the parameter table of libmpdx, the appended mpdx_unet_cfg member, and the refusals of the training step."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
MULTS = (1, 2, 4, 8)


def _net(self_attention=True, **kw):
    import mpd_public_amd as m
    args = dict(n_support_points=64, state_dim=4, unet_input_dim=32, dim_mults=MULTS)
    args.update(kw)
    return m.TemporalUnet(self_attention=self_attention, **args)


def _reference_layout():
    """(name, shape) of the reference network's 236 tensors, in the reference's state_dict() order (state_dict_keys_attention.txt)"""
    out = []
    for line in (GOLDEN / "state_dict_keys_attention.txt").read_text().splitlines():
        cfg, key, *shape = line.split()
        if key.startswith("model."):
            out.append((key[len("model."):], tuple(int(s) for s in shape[0].split("x")) if shape else ()))
    return out


def test_state_dict_has_the_reference_names_shapes_and_order():
    ref = _reference_layout()
    assert len(ref) == 236
    got = [(k, tuple(v.shape)) for k, v in _net().state_dict().items()]
    assert got == ref, [p for p in zip(got, ref) if p[0] != p[1]][:3]
    attn = [k for k, _ in got if ".fn." in k]
    assert len(attn) == 40 and {k.rsplit(".fn.", 1)[0].split(".fn")[0] for k in attn} == {f"downs.{i}.2" for i in range(4)} | {"mid_attn"} | {f"ups.{j}.2" for j in range(3)}
    # attention off: the slots are nn.Identity, the layout the plain network always had
    plain = _net(False)
    assert len(plain.state_dict()) == 196 and isinstance(plain.mid_attn, torch.nn.Identity) and isinstance(plain.downs[0][2], torch.nn.Identity)


def test_whole_checkpoint_layout_matches_the_reference():
    import mpd_public_amd as m
    want = {}
    for line in (GOLDEN / "state_dict_keys_attention.txt").read_text().splitlines():
        cfg, key, *shape = line.split()
        want[key] = tuple(int(s) for s in shape[0].split("x")) if shape else ()
    dm = m.GaussianDiffusionModel(model=_net(), n_diffusion_steps=25, predict_epsilon=True)
    assert {k: tuple(v.shape) for k, v in dm.state_dict().items()} == want


def test_native_parameter_table_agrees():
    from mpd_public_amd import _lib
    lib = _lib.load()
    net = _net()
    h = net._handle()
    assert lib.mpdx_unet_num_params(h) == 236
    name, shape, ndim = C.c_char_p(), (C.c_int32 * 3)(), C.c_int32()
    got = {}
    for i in range(236):
        assert lib.mpdx_unet_param_info(h, i, C.byref(name), shape, C.byref(ndim)) == 0
        got[name.value.decode()] = tuple(shape[k] for k in range(ndim.value))
    assert got == dict(_reference_layout())
    plain = _net(False)   # (kept alive: the module owns its handle)
    assert lib.mpdx_unet_num_params(plain._handle()) == 196   # the default model is what it was
    # the other shapes of the golden cases build too (zero-padded containers, 128 positions, 64 base channels)
    for kw in (dict(n_support_points=24, state_dim=6, dim_mults=(1, 2, 4)), dict(n_support_points=40, state_dim=2),
               dict(n_support_points=128, dim_mults=(1, 2, 4)), dict(unet_input_dim=64, dim_mults=(1, 2, 4)), dict(n_support_points=96, state_dim=14)):
        n = _net(**kw)
        assert lib.mpdx_unet_num_params(n._handle()) == len(n.state_dict())


def test_strict_load_of_a_reference_named_state_dict_and_deepcopy():
    import copy
    from mpd_public_amd import synthetic as syn
    net = _net()
    sd = syn.synth_state_dict(dict(_reference_layout()))
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.mid_attn.fn.norm.g, sd["mid_attn.fn.norm.g"]) and torch.equal(net.ups[2][2].fn.fn.to_out.bias, sd["ups.2.2.fn.fn.to_out.bias"])
    # the LayerNorm parameters of the synthetic fixture sit around 1 and 0 like the GroupNorm ones (a 0.05 u scale would nearly switch the block off)
    g, b = sd["downs.0.2.fn.norm.g"], sd["downs.0.2.fn.norm.b"]
    assert 0.9 <= float(g.min()) and float(g.max()) <= 1.1 and float(g.std()) > 0.03 and float(b.abs().max()) <= 0.1 and float(b.std()) > 0.03
    with pytest.raises(RuntimeError):   # a plain checkpoint does not load into an attention network, nor the other way round
        net.load_state_dict({k: v for k, v in sd.items() if ".fn." not in k}, strict=True)
    with pytest.raises(RuntimeError):
        _net(False).load_state_dict(sd, strict=True)
    cp = copy.deepcopy(net)
    assert cp._h is None and cp.self_attention and len(cp.state_dict()) == 236
    assert all(torch.equal(a, b_) and a.data_ptr() != b_.data_ptr() for a, b_ in zip(cp.state_dict().values(), net.state_dict().values()))
    from mpd_public_amd import _lib
    assert _lib.load().mpdx_unet_num_params(cp._handle()) == 236   # the copy builds its own handle, with the flag


def test_cfg_struct_matches_the_c_header(tmp_path):
    """sizeof(mpdx_unet_cfg) and the offset of the appended member as a C compiler sees the header (method of test_abi_struct_sizes_match_the_c_header)."""
    from mpd_public_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on this host")
    src = tmp_path / "cfg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpdx.h"\nint main(void) { mpdx_unet_cfg c = {4, 64, 32, 4, {1, 2, 4, 8}, 32};\n'
                   'printf("%zu %zu %zu %d\\n", sizeof(mpdx_unet_cfg), offsetof(mpdx_unet_cfg, self_attention), offsetof(mpdx_unet_cfg, time_emb_dim), '
                   '(int)c.self_attention); return 0; }\n')
    exe = tmp_path / "cfg"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.UnetCfg), _lib.UnetCfg.self_attention.offset, _lib.UnetCfg.time_emb_dim.offset, 0]   # a positional initialiser of the old members leaves it 0
    assert _lib.UnetCfg(4, 64, 32, 4, (C.c_int32 * _lib.MAX_LEVELS)(1, 2, 4, 8), 32).self_attention == 0


def test_create_refuses_other_flag_values():
    from mpd_public_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.UnetCfg(4, 64, 32, 4, (C.c_int32 * _lib.MAX_LEVELS)(1, 2, 4, 8), 32, 2)
    assert lib.mpdx_unet_create(C.byref(cfg), C.byref(h)) != 0 and b"self_attention" in lib.mpdx_last_error()


def test_training_entry_points_refuse_through_the_c_abi():
    from mpd_public_amd import _lib
    lib = _lib.load()
    net = _net()   # (kept alive: the module owns its handle)
    h = net._handle()
    for size in (lambda: lib.mpdx_train_flat_floats(h), lambda: lib.mpdx_train_dgrad_pack_floats(h), lambda: lib.mpdx_train_workspace_floats(h, 8)):
        assert size() == 0
        msg = lib.mpdx_last_error().decode()
        assert "self-attention" in msg and "no backward" in msg
    off, n = C.c_size_t(), C.c_size_t()
    assert lib.mpdx_train_param_offset(h, 0, C.byref(off), C.byref(n)) != 0 and "self-attention" in lib.mpdx_last_error().decode()
    one = (C.c_float * 4)()
    p = C.cast(one, C.c_void_p)
    assert lib.mpdx_train_pack(h, p, p, None, None) != 0 and "self-attention" in lib.mpdx_last_error().decode()
    assert lib.mpdx_train_draw(h, 1, None) != 0 and "self-attention" in lib.mpdx_last_error().decode()
    assert lib.mpdx_train_loss_backward(h, p, p, p, p, p, p, p, p, p, p, None, None, None, 25, 1, 1, 0, 1.0, p, p, None) != 0
    assert "self-attention" in lib.mpdx_last_error().decode() and "no backward" in lib.mpdx_last_error().decode()
    # the plain network's sizes are untouched
    plain = _net(False)
    hp = plain._handle()
    assert lib.mpdx_train_flat_floats(hp) > 0 and lib.mpdx_train_workspace_floats(hp, 8) > 0


def test_python_training_entries_refuse_before_any_device_work():
    import mpd_public_amd as m
    from mpd_public_amd.trainer import TrainStep
    dm = m.GaussianDiffusionModel(model=_net(), n_diffusion_steps=25, predict_epsilon=True)   # on the CPU: nothing below may reach a device
    with pytest.raises(NotImplementedError, match="self-attention.*no backward"):
        TrainStep(dm)
    x = torch.zeros(2, 64, 4)
    with pytest.raises(NotImplementedError, match="self-attention.*no backward"):
        dm.loss(x, None, {})
    from mpd_public_amd.train import experiment
    with pytest.raises(NotImplementedError, match="self-attention.*no backward"):   # refused, not swallowed by **kwargs
        experiment(self_attention=True, results_dir="/nonexistent/never_created", device="cpu")
    with pytest.raises(NotImplementedError):   # the other refusal stays as it was
        _net(conditioning_type="attention")
