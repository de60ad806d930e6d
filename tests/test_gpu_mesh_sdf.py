"""GPU tests of the mesh producer (csrc/mesh_sdf.hpp: mpdx_sdf_grid_from_mesh) and of what is built on it (GridSDF.from_mesh / update_mesh,
refresh_grids, TrajectoryDataset(sdf_grid=<GridSDF>)).

The distance and the winding number are held to the float64 restatement tests/mesh_ref.py, evaluated at the same fp32 node positions on the same
fp32 vertices, within bounds that come from the number format: with U = 2^-24 * L, L the largest absolute coordinate among nodes and vertices,
  |d - d_ref| <= 16 U      (an fp32 numpy restatement needs 1.1 - 1.8 U; the rest is room for contraction and another operation order)
  |w - w_ref| <= 1e-5      (the fp32 restatement's worst is 8.3e-7 for F <= 1292)
and the sign is compared away from |w_ref - 0.5| < 0.01 only.  The gradient plane is compared bit for bit with tests/edt_ref.grad_ref of the device's
own sdf plane.  Measured on an MI355X (largest multiple of U / largest winding error per case, inflate 0 and 0.03 alike): profiles/mesh_sdf_probe.md."""
import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import edt_ref
import mesh_ref
from helpers import obstacle_hugging_trajs
from test_gpu_grid_sdf import CAP, TA, _classify, _oracle_with_grid

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TILE = 256                      # faces per LDS tile of the kernel (checked against the source below)
INFLATES = (0.0, 0.03)
D_ULPS, W_TOL, AMBIGUOUS = 16.0, 1e-5, 0.01
GUARD = 64


def _run(V32, F, grid, inflate=0.0, sign="winding", with_grad=True, with_wind=True):
    """mpdx_sdf_grid_from_mesh -> (sdf [nz, ny, nx], grad [nz, ny, nx, 4] or None, wind or None) as numpy.  Every output starts as NaN and carries GUARD
    words behind it that must stay NaN."""
    from mpd_public_amd import _lib
    lib = _lib.load()
    nx, ny, nz = grid["n"]
    nodes = nx * ny * nz
    v = torch.from_numpy(np.array(V32, dtype=np.float32)).cuda()            # (copies: the cases are read-only)
    f = torch.from_numpy(np.array(F, dtype=np.int32)).cuda()
    new = lambda words: torch.full((words + GUARD,), float("nan"), device="cuda")
    sdf = new(nodes)
    grad = new(4 * nodes) if with_grad else None
    wind = new(nodes) if with_wind and sign == "winding" else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.mpdx_sdf_grid_from_mesh(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], sdf.data_ptr(), ptr(grad), ptr(wind), C.byref((C.c_int * 3)(nx, ny, nz)),
                                           C.byref((C.c_float * 3)(*grid["origin"])), grid["cell"], inflate, {"winding": _lib.MESH_SIGN_WINDING, "none": _lib.MESH_SIGN_NONE}[sign],
                                           _lib.current_stream()), "mpdx_sdf_grid_from_mesh")
    torch.cuda.synchronize()
    shp = (nz, ny, nx)
    out = []
    for t, words, s in ((sdf, nodes, shp), (grad, 4 * nodes, shp + (4,)), (wind, nodes, shp)):
        if t is None:
            out.append(None)
            continue
        assert bool(torch.isnan(t[words:]).all()), "the guard behind an output was written"
        a = t[:words].cpu().numpy().reshape(s)
        assert not np.isnan(a).any(), "a node was not written"
        out.append(a)
    return tuple(out)


@lru_cache(maxsize=None)
def _device(name, inflate):
    """the winding-mode run of a named case, both optional outputs on: shared by the tests below, read-only"""
    c = mesh_ref.case(name)
    out = _run(c["V32"], c["F"], c["grid"], inflate)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_tile_of_the_source_is_the_tile_of_these_cases():
    text = (ROOT / "mpd_public_amd" / "csrc" / "mesh_sdf.hpp").read_text()
    assert int(re.search(r"#define\s+MPDX_MESH_TILE\s+(\d+)", text).group(1)) == TILE
    nf = {k: mesh_ref.case(k)["F"].shape[0] for k in mesh_ref.CASES}
    assert nf["box"] < TILE < nf["sphere"] and nf["many"] > 2 * TILE and nf["many"] % TILE != 0
    g = mesh_ref.GRID["n"]
    assert (g[0] * g[1] * g[2]) % 256 != 0 and g[0] % 2 == 1            # rows end inside a wave, the last workgroup is partial


# ------------------------------------------------------------------------------------------------------------------------ 1-4. distance, winding, sign
@pytest.mark.parametrize("inflate", INFLATES)
@pytest.mark.parametrize("name", list(mesh_ref.CASES))
def test_distance_winding_and_sign_vs_fp64(name, inflate):
    c = mesh_ref.case(name)
    d_ref, w_ref, U = c["d"], c["w"], 2.0 ** -24 * c["L"]
    if name == "box":       # the input reaches every branch of the closest-point test (asserted before the device result is looked at)
        outside = w_ref < 0.5
        counts = [int(((c["feature"] == k) & outside).sum()) for k in (mesh_ref.FACE, mesh_ref.EDGE, mesh_ref.VERTEX)] + [int((~outside).sum())]
        print(f"box: nodes nearest a face / an edge / a vertex / inside: {counts}")
        assert min(counts) >= 500
    amb = np.abs(w_ref - 0.5) < AMBIGUOUS
    print(f"{name}: F {c['F'].shape[0]}, nodes {d_ref.size}, L {c['L']:.4f}, closest node {d_ref.min():.1e} m, ambiguous {int(amb.sum())}")
    assert amb.sum() == 0 if name in mesh_ref.CLOSED else amb.mean() <= 0.01
    sdf, _, wind = _device(name, inflate)
    assert sdf.dtype == np.float32
    s64 = sdf.astype(np.float64)
    d_gpu = np.abs(s64 + inflate)
    e_d, e_w = np.abs(d_gpu - d_ref).max() / U, np.abs(wind - w_ref).max()
    print(f"  inflate {inflate}: max |d - d_ref| = {e_d:.2f} U, max |w - w_ref| = {e_w:.2e}")
    assert e_d <= D_ULPS
    assert e_w <= W_TOL
    inside = w_ref > 0.5
    assert ((s64 + inflate < 0) == inside)[~amb].all()
    s_ref = np.where(inside, -d_ref, d_ref) - inflate
    assert (np.abs(s64 - s_ref) <= D_ULPS * U + 2.0 ** -24 * np.abs(s_ref))[~amb].all()
    assert inside.any() and not inside.all()


def _sub_case(nf):
    """the first nf faces of the sphere's list: an open sheet"""
    c = mesh_ref.case("sphere")
    g = mesh_ref.GRID
    F = c["F"][:nf]
    P = mesh_ref.nodes(g["n"], g["origin"], g["cell"])
    d, _, _ = mesh_ref.field_at(P.reshape(-1, 3), c["V32"].astype(np.float64), F, winding=False)
    return c["V32"], F, g, d.reshape(P.shape[:-1]), float(max(np.abs(P).max(), np.abs(c["V32"]).max()))


@pytest.mark.parametrize("nf", [TILE, TILE + 1], ids=["one_tile", "one_tile_and_a_face"])
def test_unsigned_mode_at_the_tile_boundary(nf):
    V32, F, g, d_ref, L = _sub_case(nf)
    assert F.shape[0] == nf
    for inflate in INFLATES:
        sdf, grad, wind = _run(V32, F, g, inflate, sign="none")
        assert wind is None
        e = np.abs((sdf.astype(np.float64) + inflate) - d_ref).max() / (2.0 ** -24 * L)
        print(f"F {nf}, inflate {inflate}: max |d - d_ref| = {e:.2f} U")
        assert e <= D_ULPS
        assert np.array_equal(grad, edt_ref.grad_ref(sdf, g["cell"]))
    # the last face matters: it is the nearest one of some node
    d_last = mesh_ref.field_at(mesh_ref.nodes(g["n"], g["origin"], g["cell"]).reshape(-1, 3), V32.astype(np.float64), F[-1:], winding=False)[0]
    assert (d_last.reshape(d_ref.shape) == d_ref).sum() >= 5


@pytest.mark.parametrize("name", list(mesh_ref.CASES))
def test_unsigned_mode_is_the_distance(name):
    """sign='none' directly: s = d - inflate, the same d bit for bit as the winding mode takes (the winding sum shares nothing with the distance)"""
    c = mesh_ref.case(name)
    U = 2.0 ** -24 * c["L"]
    for inflate in INFLATES:
        sdf, _, _ = _run(c["V32"], c["F"], c["grid"], inflate, sign="none", with_grad=False)
        e = np.abs((sdf.astype(np.float64) + inflate) - c["d"]).max() / U
        print(f"{name} unsigned, inflate {inflate}: max |d - d_ref| = {e:.2f} U")
        assert e <= D_ULPS
        if inflate == 0.0:
            assert (sdf >= 0).all() and np.array_equal(sdf, np.abs(_device(name, 0.0)[0]))


# ------------------------------------------------------------------------------------------------------------------------ 5-6. gradient plane, determinism
@pytest.mark.parametrize("name", ["box", "open_cap", "many"])
def test_gradient_plane_bit_for_bit_and_optional_outputs(name):
    c = mesh_ref.case(name)
    for inflate in INFLATES:
        sdf, grad, _ = _device(name, inflate)
        assert grad.dtype == np.float32 and np.array_equal(grad, edt_ref.grad_ref(sdf, c["grid"]["cell"]))
        assert not grad[..., 3].any() and np.abs(grad[..., :3]).max() > 0.5
        bare, none_g, none_w = _run(c["V32"], c["F"], c["grid"], inflate, with_grad=False, with_wind=False)
        assert none_g is None and none_w is None and np.array_equal(bare, sdf)


@pytest.mark.parametrize("name", ["sphere", "many"])
def test_two_runs_give_the_same_bits(name):
    c = mesh_ref.case(name)
    first = _device(name, 0.03)
    again = _run(c["V32"], c["F"], c["grid"], 0.03)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------ 4, 7. GridSDF.from_mesh
WS = (np.array([-0.2, -0.15, 0.25]), np.array([0.2, 0.15, 0.6]))


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_from_mesh_is_the_kernel_and_orients_an_inward_mesh(mode):
    from mpd_public_amd.planning import GridSDF, grid_spec_for
    V, F = mesh_ref.mesh("two")
    cell, inflate = 0.05, 0.03
    g = GridSDF.from_mesh(V, F, WS[0], WS[1], cell, mode=mode, inflate=inflate)
    shape, origin = grid_spec_for(WS[0], WS[1], cell)
    assert g.shape == shape and g.dim == 3 and g.inflate == inflate and np.array_equal(g.origin, origin)
    assert g.mesh_info["flipped"] is False and g.mesh_info["dropped_faces"] == 0 and g.mesh_info["n_faces"] == 92
    sdf, grad = g.node_values()
    assert sdf.is_cuda and g.planes("cuda")[0].data_ptr() == g.sdf.data_ptr()                   # the planes are the tensors the grid was made on: no copy
    want = _run(V.astype(np.float32), F, dict(n=shape, origin=[float(v) for v in origin], cell=cell), inflate, with_wind=False)
    assert np.array_equal(sdf.cpu().numpy(), want[0])
    assert (grad is None and g.grad is None) if mode == "linear" else np.array_equal(grad.cpu().numpy(), want[1])
    # faces reversed and two zero-area faces added: the same planes
    h = GridSDF.from_mesh(torch.from_numpy(V), torch.from_numpy(np.concatenate([F[:, ::-1], [[0, 0, 1], [5, 9, 5]]]).astype(np.int32)), WS[0], WS[1], cell,
                          mode=mode, inflate=inflate)
    assert h.mesh_info["flipped"] is True and h.mesh_info["dropped_faces"] == 2 and h.mesh_info["signed_volume"] < 0
    for a, b in zip(g.node_values(), h.node_values()):
        assert (a is None and b is None) or torch.equal(a, b)
    with pytest.raises(RuntimeError, match="not copied"):
        g.planes("cpu")


def test_box_mesh_agrees_with_the_primitive_bake():
    """the new producer against one the project already trusts: the same box as a mesh and as a primitive, on the same grid"""
    from mpd_public_amd.planning import GridSDF, ObjectSet
    lo, hi = (np.asarray(v, np.float64) for v in mesh_ref.BOX)
    V, F = mesh_ref.box(lo, hi)
    cell = 0.05
    g = GridSDF.from_mesh(V, F, WS[0], WS[1], cell)
    z3, z1 = np.zeros((0, 3), np.float32), np.zeros((0,), np.float32)
    prim = GridSDF(None, g.origin, cell, source=ObjectSet(z3, z1, (0.5 * (lo + hi))[None].astype(np.float32), (0.5 * (hi - lo))[None].astype(np.float32)), shape=g.shape)
    a, b = g.node_values()[0].cpu().numpy().astype(np.float64), prim.node_values("cuda")[0].cpu().numpy().astype(np.float64)
    P = mesh_ref.nodes(g.shape, g.origin, cell)
    L = float(max(np.abs(P).max(), np.abs(V).max()))
    e = np.abs(a - b).max() / (2.0 ** -24 * L)
    print(f"box mesh vs primitive bake: {a.size} nodes, inside {int((b < 0).sum())}, max |difference| = {e:.2f} U (L {L:.3f})")
    assert (b < 0).sum() >= 100 and (b > 0.2).any()
    assert e <= 32.0                                                                            # each side gets one bound of 16 U


# ------------------------------------------------------------------------------------------------------------------------ 8. under the task
def _cell_mesh(ds_prim):
    """an icosphere and a box where the environment has its first two fixed spheres: the trajectories that hug those hug the mesh"""
    c = ds_prim.env.obj_fixed.sphere_centers.astype(np.float64)
    return mesh_ref.concat(mesh_ref.icosphere(2, 0.17, c[0]), mesh_ref.box(c[1] - 0.13, c[1] + 0.13))


def _metrics_follow_the_oracle(ds_prim, ds, x, n_check, tag):
    from oracle import costs as oc
    from oracle.guide import interpolate_points_v1
    og, comp, gf, k = _oracle_with_grid(ds_prim, ds)
    xu = og.normalizer.unnormalize(x.double()).float()
    xi = interpolate_points_v1(xu.double(), n_check)
    amb = _classify(comp, gf, xi, {i: 0.0 for i in range(len(comp.cost_l))}).numpy()
    hit = torch.zeros(xi.shape[:2], dtype=torch.bool)
    on_grid = None
    for i, term in enumerate(comp.cost_l):
        if isinstance(term, oc.CostCollision):
            keep, term.cutoff = term.cutoff, 0.0
            h = (term.factors(xi) > 0).any(-1)
            term.cutoff = keep
            hit |= h
            if i == k:
                on_grid = h.numpy()
    hit = hit.numpy()
    print(f"{tag}: ambiguous interpolated waypoints {amb.mean():.4f} (cap {CAP['RobotPanda']}), colliding {hit.mean():.3f}, with the mesh field {on_grid.mean():.3f}")
    assert amb.mean() <= CAP["RobotPanda"]
    assert hit.any() and not hit.all() and on_grid.any()
    out, mask = ds.task.trajectory_metrics(xu.cuda(), n_check=n_check, return_mask=True)
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    print(f"  flags differing outside ambiguous: {int((mask != hit)[~amb].sum())}; inside: {int((mask != hit)[amb].sum())} of {int(amb.sum())}")
    assert (mask == hit)[~amb].all()
    np.testing.assert_array_equal(out[:, 0], mask.sum(1))
    np.testing.assert_array_equal(out[:, 3], n_check)
    return on_grid


def test_mesh_grid_under_the_task_and_update_mesh():
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    env_id, robot_id = "EnvSpheres3D", "RobotPanda"
    ds_prim = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
    V, F = _cell_mesh(ds_prim)
    grid = m.GridSDF.from_mesh(V, F, ds_prim.task.ws_min, ds_prim.task.ws_max, cell_size=0.05)
    ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA, sdf_grid=grid)
    assert ds.task.df_collision_objects.kind == _lib.FIELD_GRID and ds.task.df_collision_objects.grid is grid
    x = obstacle_hugging_trajs(ds_prim, 7, seed=f"g/{env_id}", scale=0.9)
    first = _metrics_follow_the_oracle(ds_prim, ds, x, 128, "mesh grid")
    # the object moved: the same planes are rewritten, the task copies them again, and the metrics follow
    before = grid.node_values()[0].clone()
    ptrs = [p.data_ptr() for p in grid.planes("cuda") if p is not None]
    assert grid.update_mesh(V + np.array([0.05, 0.0, 0.0])) is grid
    assert [p.data_ptr() for p in grid.planes("cuda") if p is not None] == ptrs
    assert not torch.equal(grid.node_values()[0], before)
    ds.task.refresh_grids()
    second = _metrics_follow_the_oracle(ds_prim, ds, x, 128, "after update_mesh")
    assert (first != second).any()
    fresh = m.GridSDF.from_mesh(V + np.array([0.05, 0.0, 0.0]), F, ds_prim.task.ws_min, ds_prim.task.ws_max, cell_size=0.05)
    assert torch.equal(fresh.node_values()[0], grid.node_values()[0])
    with pytest.raises(ValueError, match="vertices"):
        grid.update_mesh(V[:-1])
