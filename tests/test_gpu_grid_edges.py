"""GPU tests of the grid lookup's geometry (csrc/grid_field.hpp): grids whose node counts differ along every axis, boxes that link points leave
below and above (the clamped branch of include/mpdx.h, mpdx_field), a grid with 2 nodes along y, and one block with two grid fields whose second
sdf plane does not start at offset 0 of the grid buffer.  The cases, the trajectories and the fp64 reference are tests/grid_edges_ref.py; their
conditions, and that the yardstick below rejects a wrong stride, a gradient kept along a clamped axis and a second grid read at offset 0, are
asserted without a GPU by tests/test_grid_edges_cpu.py.

The grids are made on the device from the fixed objects' occupancy (GridSDF.from_occupancy, inflate 0.003); the planes are downloaded and must equal
tests/edt_ref.py's bit for bit; the reference (tests/grid_ref.GridField inside the unchanged fp64 oracle) is built over the downloaded planes.  The
yardstick is tests/test_gpu_grid_sdf.py's, unchanged: rtol 1e-3 / atol 2e-6 at w_coll = 1e-2 on the support waypoints its ambiguity
classification (_classify, _to_supports) leaves in, under the cap CAP; the metrics flags equal the fp64 flags outside the ambiguous checked points."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid_edges_ref as ger
from helpers import product_guide

pytestmark = pytest.mark.gpu

EDGE_CASES = [(n, m) for n in ger.CASES for m in ("linear", "nearest")]


def _device_grid(spec, env_id, mode):
    """(GridSDF made on the device, GridField over its downloaded planes); the planes equal edt_ref's bit for bit"""
    import mpd_public_amd as m
    occ, sdf, grad = ger.spec_planes(spec, env_id)
    g = m.GridSDF.from_occupancy(np.array(occ), spec["origin"], spec["cell"], mode=mode, inflate=ger.INFLATE)   # (a writable copy for torch)
    assert g.shape == tuple(spec["shape"]) and g.mode == mode
    s, gr = g.node_values("cuda")
    s = s.cpu().numpy()
    assert np.array_equal(s, sdf)
    if mode == "nearest":
        gr = gr.cpu().numpy()
        assert np.array_equal(gr, grad)
    else:
        assert gr is None
    return g, ger.field_of(spec, mode, s, gr)


def _descriptor(gp, k, spec, mode):
    from mpd_public_amd import _lib
    f = gp.fields[k]
    dim = len(spec["shape"])
    assert f.kind == _lib.FIELD_GRID and gp.grids and gp.n_scenes <= 1
    assert [f.n[j] for j in range(3)] == list(spec["shape"]) + [1] * (3 - dim)
    assert f.mode == (_lib.GRID_NEAREST if mode == "nearest" else _lib.GRID_LINEAR)
    assert np.array_equal(np.array([f.origin[j] for j in range(dim)], np.float32), np.asarray(spec["origin"], np.float32))


def _compare(r, got, mask, out, cap, what):
    amb, ref = r["amb"], r["ref"]
    print(f"{what}: ambiguous support waypoints {amb.mean():.4f}, checked points {r['amb_m'].mean():.4f} (cap {cap})")
    assert amb.mean() <= cap and r["amb_m"].mean() <= cap
    assert np.abs(ref).max() > 0 and got.shape == ref.shape
    assert not got[:, 0].any() and not got[:, -1].any()
    print(f"  guide: max|diff| outside ambiguous = {np.abs(got - ref)[~amb].max():.3e}; differing unambiguous waypoints "
          f"{int((ger.outside(got, ref) & ~amb).sum())} of {int((~amb).sum())}")
    print(f"  metrics: flags differing outside ambiguous {int((mask != r['hit'])[~r['amb_m']].sum())} of {int((~r['amb_m']).sum())}")
    np.testing.assert_allclose(got[~amb], ref[~amb], rtol=1e-3, atol=ger.atol_of())
    assert (mask == r["hit"])[~r["amb_m"]].all()
    np.testing.assert_array_equal(out[:, 0], mask.sum(1))
    np.testing.assert_array_equal(out[:, 3], mask.shape[1])


@pytest.mark.parametrize("name,mode", EDGE_CASES, ids=[f"{n}-{m}" for n, m in EDGE_CASES])
def test_edge_grid_guide_and_metrics_vs_oracle(name, mode):
    c = ger.CASES[name]
    g, gf = _device_grid(c, c["env_id"], mode)
    r = ger.reference(name, [gf])
    ds = ger.with_grids(ger.base_dataset(c, "cuda"), [g])
    x = r["x"]
    pg = product_guide(ds, *ger.WEIGHTS).cuda()
    gp = pg.device_params("cuda")
    _descriptor(gp, r["ks"][0], c, mode)
    got = pg(x.cuda()).cpu().numpy()
    xu = r["og"].normalizer.unnormalize(x.double()).float()
    out, mask = ds.task.trajectory_metrics(xu.cuda(), n_check=ger.n_check_of(c["H"]), return_mask=True)
    _compare(r, got, mask.cpu().numpy(), out.cpu().numpy(), ger.CAP[ger.robot_of(c["robot_id"])], f"{name} {mode}")


def test_two_grid_fields_in_one_block():
    """a nearest grid (2537 nodes: its planes padded to a multiple of 4) in the objects slot, the workspace field, a linear grid over another box in
    the extra-objects slot and the GP prior: guide increment, then mpdx_traj_metrics_mask on the same block"""
    from mpd_public_amd import _lib
    c = ger.TWO
    made = [_device_grid(s, c["env_id"], s["mode"]) for s in c["grids"]]
    r = ger.reference("two", [gf for _, gf in made])
    ds = ger.with_grids(ger.base_dataset(c, "cuda"), [g for g, _ in made])
    x = r["x"]
    pg = product_guide(ds, *ger.WEIGHTS).cuda()
    gp = pg.device_params("cuda")
    k0, k1 = r["ks"]
    assert [gp.fields[i].kind for i in range(gp.n_fields)] == [_lib.FIELD_GRID, _lib.FIELD_WORKSPACE, _lib.FIELD_GRID] and gp.use_gp
    for k, s in zip(r["ks"], c["grids"]):
        _descriptor(gp, k, s, s["mode"])
    assert gp.fields[k0].grid_sdf_off == 0 and gp.fields[k0].grid_grad_off > 0
    assert gp.fields[k1].grid_sdf_off > 0 and gp.fields[k1].grid_grad_off == -1
    n0 = int(np.prod(c["grids"][0]["shape"]))
    assert n0 % 4 and gp.fields[k0].grid_grad_off % 4 == 0 and gp.fields[k1].grid_sdf_off >= gp.fields[k0].grid_grad_off + 4 * n0
    got = pg(x.cuda()).cpu().numpy()
    B, H, D = x.shape
    xu = r["og"].normalizer.unnormalize(x.double()).float().cuda().contiguous()
    n_check = ger.n_check_of(H)
    out = torch.empty((B, 4), dtype=torch.float32, device="cuda")
    mask = torch.empty((B, n_check), dtype=torch.uint8, device="cuda")
    lib, st = _lib.load(), _lib.current_stream()
    _lib.check(lib.mpdx_traj_metrics_mask(C.byref(gp), xu.data_ptr(), out.data_ptr(), mask.data_ptr(), n_check, B, H, D, st), "mpdx_traj_metrics_mask")
    torch.cuda.synchronize()
    _compare(r, got, mask.cpu().numpy().astype(bool), out.cpu().numpy(), ger.CAP["RobotPointMass"], "two grids")
