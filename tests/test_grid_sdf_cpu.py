"""CPU checks of the grid signed-distance field (MPDX_FIELD_GRID): descriptor packing, ABI struct sizes against the C header, the torch_robotics
adapter, host-side validation of the launchers through the C ABI (no launch), and the fp64 reference lookup (tests/grid_ref.py) itself."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from grid_ref import GridField

ROOT = Path(__file__).resolve().parent.parent


def _toy_grid(dim=2, mode="linear", n=(9, 7, 5), cell=0.25, with_grad=None):
    from mpd_public_amd.planning import GridSDF
    shape = tuple(reversed(n[:dim]))
    g = torch.Generator().manual_seed(3)
    sdf = torch.rand(shape, generator=g)
    grad = torch.rand(shape + (dim,), generator=g) if (with_grad if with_grad is not None else mode == "nearest") else None
    return GridSDF(sdf, np.full(dim, -1.0, np.float32) + 0.01, cell, mode=mode, grad=grad)


def _grid_guide_params(dim=2, mode="linear", device="cpu"):
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    from mpd_public_amd.guides import build_device_params
    from mpd_public_amd.planning import CollisionField
    ds = m.TrajectoryDataset("EnvSimple2D" if dim == 2 else "EnvSpheres3D", "RobotPointMass" if dim == 2 else "RobotPanda")
    grid = _toy_grid(dim, mode)
    fields = [CollisionField(_lib.FIELD_GRID, grid=grid, name="objects"), ds.task.df_collision_ws_boundaries, ds.task.df_collision_extra_objects]
    costs = [m.CostCollision(ds.robot, 64, field=f) for f in fields]
    gp, prims = build_device_params(ds.robot, dim, 0.05, None, None, costs, [1.0] * 3, True, 128, True, 1.0, device)
    return gp, prims, grid, ds


@pytest.mark.parametrize("dim,mode", [(2, "linear"), (2, "nearest"), (3, "linear"), (3, "nearest")])
def test_grid_field_packs_into_guide_params(dim, mode):
    from mpd_public_amd import _lib
    gp, prims, grid, ds = _grid_guide_params(dim, mode)
    f = gp.fields[0]
    nodes = grid.n_nodes
    assert [gp.fields[i].kind for i in range(gp.n_fields)] == [_lib.FIELD_GRID, _lib.FIELD_WORKSPACE, _lib.FIELD_OBJECTS]
    assert f.mode == (_lib.GRID_NEAREST if mode == "nearest" else _lib.GRID_LINEAR)
    assert list(f.n) == list(grid.shape) + [1] * (3 - dim) and nodes == int(np.prod(list(f.n)))
    assert f.cell == pytest.approx(0.25) and list(f.origin)[:dim] == pytest.approx([-0.99] * dim)
    assert f.grid_sdf_off == 0
    assert gp.grids and gp.grids == gp.grids_tensor.data_ptr()
    if mode == "nearest":
        assert f.grid_grad_off >= nodes and f.grid_grad_off % 4 == 0
        assert gp.n_grid_floats >= f.grid_grad_off + 4 * nodes
        g4 = gp.grids_tensor[f.grid_grad_off: f.grid_grad_off + 4 * nodes].reshape(-1, 4)
        assert torch.equal(g4[:, :dim], grid.grad.reshape(-1, dim)) and not g4[:, dim:].any()
    else:
        assert f.grid_grad_off == -1 and gp.n_grid_floats >= nodes
    assert torch.equal(gp.grids_tensor[:nodes], grid.sdf.reshape(-1))
    # the grid is NOT part of the primitive table every kernel stages in LDS: only the extra objects are
    extra = ds.env.obj_extra
    assert gp.n_prim_floats == 4 * len(extra.sphere_radii) + 6 * len(extra.box_centers)
    assert gp.fields[2].n_spheres == len(extra.sphere_radii)


def test_grid_sdf_descriptor_validation():
    from mpd_public_amd.planning import GridSDF
    with pytest.raises(ValueError, match="nearest"):
        GridSDF(torch.zeros(4, 4), [0, 0], 0.1, mode="nearest")
    with pytest.raises(ValueError, match="mode"):
        GridSDF(torch.zeros(4, 4), [0, 0], 0.1, mode="cubic")
    with pytest.raises(ValueError, match="cell"):
        GridSDF(torch.zeros(4, 4), [0, 0], 0.0)
    with pytest.raises(ValueError):
        GridSDF(torch.zeros(4, 4), [0, 0, 0], 0.1)
    g = GridSDF(torch.zeros(5, 4, 3), [0, 0, 0], 0.1, grad=torch.zeros(5, 4, 3, 3), mode="nearest")
    assert g.shape == (3, 4, 5) and g.dim == 3 and g.n_nodes == 60


def test_abi_struct_sizes_match_the_c_header(tmp_path):
    """ctypes mirrors of mpdx_field / mpdx_guide_params have the size and the member offsets a C compiler gives the header's structs."""
    from mpd_public_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on this host")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpdx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mpdx_field), '
                   'sizeof(mpdx_guide_params), offsetof(mpdx_field, grid_sdf_off), offsetof(mpdx_field, mode), offsetof(mpdx_guide_params, fields), '
                   'offsetof(mpdx_guide_params, prims), offsetof(mpdx_guide_params, grids)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_lib.Field), C.sizeof(_lib.GuideParams), _lib.Field.grid_sdf_off.offset, _lib.Field.mode.offset, _lib.GuideParams.fields.offset,
            _lib.GuideParams.prims.offset, _lib.GuideParams.grids.offset]
    assert got == want
    # every integer constant of the header that _lib mirrors (name without the prefix) has the header's value; the grid ones exist
    import re
    defs = {k: int(v) for k, v in re.findall(r"#define MPDX_(\w+)\s+\(?(-?\d+)\)?", (ROOT / "include" / "mpdx.h").read_text())}
    assert {"FIELD_GRID", "GRID_LINEAR", "GRID_NEAREST"} <= set(defs) and defs["FIELD_GRID"] == 3 and (defs["GRID_LINEAR"], defs["GRID_NEAREST"]) == (0, 1)
    mirrored = [k for k in defs if hasattr(_lib, k)]
    assert len(mirrored) >= 8 and all(getattr(_lib, k) == defs[k] for k in mirrored), [k for k in mirrored if getattr(_lib, k) != defs[k]]


# ---------------------------------------------------------------------------------------------------------------- the grid module
def test_planning_re_exports_the_grid_module_names():
    import mpd_public_amd as m
    from mpd_public_amd import grid_sdf, planning
    for name in ("GridSDF", "grid_spec_for", "GRID_MODES", "MESH_SIGNS", "_check_mesh", "_mesh_vertices", "_occupancy_bytes"):
        assert getattr(planning, name) is getattr(grid_sdf, name), name
    assert m.GridSDF is grid_sdf.GridSDF


@pytest.mark.parametrize("env_id,robot_id", [("EnvSimple2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")])
def test_for_primitives_is_the_dict_form_of_the_task(env_id, robot_id):
    import mpd_public_amd as m
    from mpd_public_amd.grid_sdf import GridSDF
    spec = dict(cell_size=0.03, mode="nearest", padding=0.25)
    task = m.TrajectoryDataset(env_id, robot_id, sdf_grid=spec).task
    want = task.df_collision_objects.grid
    got = GridSDF.for_primitives(task.env.obj_fixed, task.ws_min, task.ws_max, spec["cell_size"], mode=spec["mode"], padding=spec["padding"])
    assert got.sdf is None and want.sdf is None and got.dim == task.env.dim
    assert got.shape == want.shape and got.origin.tobytes() == want.origin.tobytes() and got.origin.dtype == want.origin.dtype
    assert got.cell == want.cell and got.mode == want.mode == "nearest" and got.source is want.source is task.env.obj_fixed
    # ... and of the defaults (mode 'linear', padding 0.3)
    dflt, plain = m.TrajectoryDataset(env_id, robot_id, sdf_grid=dict(cell_size=0.03)).task.df_collision_objects.grid, GridSDF.for_primitives(
        task.env.obj_fixed, task.ws_min, task.ws_max, 0.03)
    assert plain.shape == dflt.shape and plain.origin.tobytes() == dflt.origin.tobytes() and plain.mode == dflt.mode == "linear"


def test_the_grid_module_does_not_import_planning():
    """In a fresh interpreter.  The package's __init__ imports planning itself (it exports PlanningTask), so the child gives the package a bare stand-in
    with the package's path: what `import mpd_public_amd.grid_sdf` then loads is what grid_sdf and its own imports ask for."""
    import sys
    code = ("import sys, types\n"
            "pkg = types.ModuleType('mpd_public_amd'); pkg.__path__ = [sys.argv[1]]; sys.modules['mpd_public_amd'] = pkg\n"
            "import mpd_public_amd.grid_sdf as g\n"
            "assert g.GridSDF.__module__ == 'mpd_public_amd.grid_sdf' and callable(g.grid_spec_for)\n"
            "print(' '.join(sorted(k for k in sys.modules if k.startswith('mpd_public_amd.'))))\n")
    out = subprocess.run([sys.executable, "-c", code, str(ROOT / "mpd_public_amd")], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    loaded = out.stdout.split()
    assert "mpd_public_amd.grid_sdf" in loaded and "mpd_public_amd.planning" not in loaded, loaded


# ---------------------------------------------------------------------------------------------------------------- adapter
def _grid_map_sdf(dim=2, n=(6, 5, 4)):
    shape = n[:dim]
    g = torch.Generator().manual_seed(5)
    return NS(sdf_tensor=torch.rand(shape, generator=g), grad_sdf_tensor=torch.rand(tuple(shape) + (dim,), generator=g),
              limits=torch.tensor([[-1.0] * dim, [-1.0 + 0.5 * (v - 1) for v in shape]]), cell_size=0.5)


def _tr_task(fields):
    env = NS(name="EnvStandIn", dim=2, limits=torch.tensor([[-1.0, -1.0], [1.0, 1.0]]), obj_fixed_list=[NS(fields=fields, pos=None, ori=None)],
             obj_extra_list=None)
    robot = NS(name="RobotPointMass", q_dim=2, link_margins_for_object_collision_checking=[0.01])
    return NS(env=env, robot=robot, obstacle_cutoff_margin=0.05)


def test_adapter_accepts_a_grid_map_sdf_and_refuses_an_incomplete_one():
    from mpd_public_amd import _lib
    from mpd_public_amd.planning import task_from_torch_robotics
    gm = _grid_map_sdf()
    t = task_from_torch_robotics(_tr_task([gm]))
    kinds = [c.kind for c in t.get_collision_fields()]
    assert kinds == [_lib.FIELD_GRID, _lib.FIELD_WORKSPACE, _lib.FIELD_OBJECTS]
    g = t.df_collision_objects.grid
    assert g.mode == "nearest" and g.shape == (6, 5) and g.cell == 0.5 and list(g.origin) == [-1.0, -1.0]
    # [ix, iy] of the source -> [iy, ix] planes (x fastest)
    assert torch.equal(g.sdf, gm.sdf_tensor.t()) and torch.equal(g.grad, gm.grad_sdf_tensor.permute(1, 0, 2))
    # the incomplete surface (what tests/test_adapter_cpu.py feeds) is still refused with the primitive message
    with pytest.raises(NotImplementedError, match="primitive"):
        task_from_torch_robotics(_tr_task([NS(grid=np.zeros((4, 4)))]))
    part = _grid_map_sdf()
    del part.grad_sdf_tensor
    with pytest.raises(NotImplementedError, match="primitive"):
        task_from_torch_robotics(_tr_task([part]))
    # one grid per objects list, not mixed with primitives
    sph = NS(centers=torch.zeros(1, 2), radii=torch.tensor([0.1]))
    with pytest.raises(NotImplementedError, match="mixed"):
        task_from_torch_robotics(_tr_task([_grid_map_sdf(), sph]))


def test_sdf_grid_none_keeps_the_primitive_fields():
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    for env_id, robot_id in (("EnvSimple2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")):
        base = m.TrajectoryDataset(env_id, robot_id).task
        none = m.TrajectoryDataset(env_id, robot_id, sdf_grid=None).task
        kinds = [f.kind for f in base.get_collision_fields()]
        assert kinds == [f.kind for f in none.get_collision_fields()] and _lib.FIELD_GRID not in kinds
        grid = m.TrajectoryDataset(env_id, robot_id, sdf_grid=dict(cell_size=0.02, mode="nearest")).task
        gk = [f.kind for f in grid.get_collision_fields()]
        assert gk == [(_lib.FIELD_GRID if f is base.df_collision_objects else f.kind) for f in base.get_collision_fields()]
        g = grid.df_collision_objects.grid
        assert g.sdf is None and g.mode == "nearest" and g.source.prim_floats()[0].tolist() == base.env.obj_fixed.prim_floats()[0].tolist()
        # grid box = workspace limits grown by the padding; origin a further 0.37 cell down
        np.testing.assert_allclose(g.origin, np.asarray(base.ws_min) - 0.3 - 0.37 * 0.02, atol=1e-6)
        last = g.origin + (np.asarray(g.shape) - 1) * 0.02
        assert (last >= np.asarray(base.ws_max) + 0.3 - 1e-6).all() and (last < np.asarray(base.ws_max) + 0.3 + 0.02).all()
    with pytest.raises(ValueError):
        m.TrajectoryDataset("EnvSimple2D", "RobotPointMass", sdf_grid=dict(mode="linear"))


# ---------------------------------------------------------------------------------------------------------------- launcher validation
@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    try:
        build.build(verbose=False)
        return _lib.load()
    except _lib.LibraryUnavailable as e:   # pragma: no cover
        pytest.skip(f"libmpdx.so does not load on this host: {e}")


def _bad_descriptors():
    """(what, mutation of a VALID grid parameter block) - each must be refused on the host, before any launch"""
    def grids_null(gp): gp.grids = None
    def one_node(gp): gp.fields[0].n[1] = 1
    def cell_zero(gp): gp.fields[0].cell = 0.0
    def cell_negative(gp): gp.fields[0].cell = -0.25
    def nearest_without_gradient(gp): gp.fields[0].mode, gp.fields[0].grid_grad_off = 1, -1
    def sdf_beyond(gp): gp.fields[0].grid_sdf_off = gp.n_grid_floats - 3
    def sdf_negative(gp): gp.fields[0].grid_sdf_off = -4
    def grad_beyond(gp): gp.fields[0].mode, gp.fields[0].grid_grad_off = 1, gp.n_grid_floats - 8
    def buffer_too_small(gp): gp.n_grid_floats = 10
    def bad_mode(gp): gp.fields[0].mode = 7
    return [(f.__name__, f) for f in (grids_null, one_node, cell_zero, cell_negative, nearest_without_gradient, sdf_beyond, sdf_negative, grad_beyond,
                                      buffer_too_small, bad_mode)]


@pytest.mark.parametrize("what,mutate", _bad_descriptors())
def test_launchers_refuse_malformed_grid_fields_without_launching(lib, what, mutate):
    gp, prims, grid, ds = _grid_guide_params(2, "linear")
    mutate(gp)
    # host buffers stand in for the device pointers: a refused call never reaches a launch, so nothing dereferences them
    x = (C.c_float * (2 * 64 * 4))()
    out = (C.c_float * (2 * 64 * 4))()
    flag = (C.c_uint32 * 1)()
    a = lambda b: C.cast(b, C.c_void_p)
    rc = lib.mpdx_guide_step(C.byref(gp), a(x), a(out), None, None, a(flag), None, 2, 2, 64, 4, None)
    assert rc == -1, (what, rc)
    msg = lib.mpdx_last_error().decode()
    assert "grid" in msg, (what, msg)
    rc = lib.mpdx_traj_metrics_mask(C.byref(gp), a(x), a(out), None, 64, 2, 64, 4, None)
    assert rc == -1 and "grid" in lib.mpdx_last_error().decode(), (what, rc)


def test_planner_entry_points_refuse_grid_fields_on_the_host(lib):
    from mpd_public_amd import _lib
    gp, prims, grid, ds = _grid_guide_params(2, "linear")
    gp.use_gp, gp.dt, gp.sigma_gp = 1, 5.0 / 64, 1.0
    buf = (C.c_float * 4096)()
    a = lambda b: C.cast(b, C.c_void_p)
    o = _lib.GpmpOpts(1.0, 10.0, 0.1, 1e-6, 1e6, 1.0, 1)
    assert lib.mpdx_gpmp_step(C.byref(gp), C.byref(o), a(buf), a(buf), a(buf), 1, 64, 4, 1, None) == -1
    assert "grid fields: guide and metrics only" in lib.mpdx_last_error().decode()
    r = _lib.RrtOpts()
    r.step, r.max_nodes, r.max_iters, r.max_connect_steps, r.n_edge_checks = 0.1, 64, 16, 4, 4
    assert lib.mpdx_rrt_connect(C.byref(gp), C.byref(r), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), 1, None) == -1
    assert "grid fields: guide and metrics only" in lib.mpdx_last_error().decode()
    assert lib.mpdx_rrt_paths(C.byref(gp), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), None, 1, 64, 64, 0.1, 4, 1, None) == -1
    assert "grid fields: guide and metrics only" in lib.mpdx_last_error().decode()


def test_bake_entry_point_validates_on_the_host(lib):
    gp, prims, grid, ds = _grid_guide_params(2, "linear")
    buf = (C.c_float * 64)()
    a = lambda b: C.cast(b, C.c_void_p)
    n, org = (C.c_int * 3)(4, 4, 1), (C.c_float * 3)(0, 0, 0)
    assert lib.mpdx_sdf_grid_bake(C.byref(gp), 0, a(buf), None, C.byref(n), C.byref(org), 0.1, None) == -1      # field 0 is the grid, not OBJECTS
    assert "OBJECTS" in lib.mpdx_last_error().decode()
    assert lib.mpdx_sdf_grid_bake(C.byref(gp), 2, a(buf), None, C.byref(n), C.byref(org), 0.0, None) == -1      # cell
    assert lib.mpdx_sdf_grid_bake(C.byref(gp), 2, a(buf), None, C.byref((C.c_int * 3)(4, 1, 1)), C.byref(org), 0.1, None) == -1   # one node along y
    assert lib.mpdx_sdf_grid_bake(C.byref(gp), 9, a(buf), None, C.byref(n), C.byref(org), 0.1, None) == -1      # no such field


# ---------------------------------------------------------------------------------------------------------------- the fp64 reference itself
@pytest.mark.parametrize("dim", [2, 3])
def test_reference_linear_lookup_reproduces_an_affine_function_and_its_gradient(dim):
    n, cell, origin = (9, 7, 5)[:dim], 0.25, np.array([-1.0, -0.5, 0.25], np.float32)[:dim]
    coef = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)[:dim]
    proto = GridField(torch.zeros(tuple(reversed(n))), origin, cell)
    nodes = (proto.node_positions() * coef).sum(-1) + 0.75            # exactly representable in fp32 (dyadic numbers)
    gf = GridField(nodes, origin, cell)
    g = torch.Generator().manual_seed(1)
    hi = torch.tensor([(v - 1) * cell for v in n], dtype=torch.float64)
    p = (torch.tensor(origin, dtype=torch.float64) + torch.rand((200, dim), generator=g, dtype=torch.float64) * hi).requires_grad_(True)
    val = gf.sdf(p)
    want = (p.detach() * coef).sum(-1) + 0.75
    assert (val.detach() - want).abs().max() < 1e-13
    grad = torch.autograd.grad(val.sum(), p)[0]
    assert (grad - coef).abs().max() < 1e-11
    # outside the box the point is clamped: value of the clamped point, zero gradient along the clamped axis
    q = p.detach().clone()
    q[:, 0] = float(origin[0]) - 0.3
    q.requires_grad_(True)
    vq = gf.sdf(q)
    qc = q.detach().clone()
    qc[:, 0] = float(origin[0])
    assert (vq.detach() - ((qc * coef).sum(-1) + 0.75)).abs().max() < 1e-13
    gq = torch.autograd.grad(vq.sum(), q)[0]
    assert not gq[:, 0].any() and (gq[:, 1:] - coef[1:]).abs().max() < 1e-11


def test_reference_linear_gradient_equals_finite_differences_away_from_faces():
    g = torch.Generator().manual_seed(2)
    gf = GridField(torch.rand((6, 7, 8), generator=g), [-1.0, -1.0, 0.0], 0.2)
    p = torch.tensor([-1.0, -1.0, 0.0], dtype=torch.float64) + torch.rand((300, 3), generator=g, dtype=torch.float64) * torch.tensor([1.4, 1.2, 1.0])
    p = p[gf.discontinuity_distance(p) > 1e-2].requires_grad_(True)
    assert p.shape[0] > 100
    grad = torch.autograd.grad(gf.sdf(p).sum(), p)[0]
    h = 1e-6
    for j in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[j] = h
        fd = (gf.sdf(p.detach() + e) - gf.sdf(p.detach() - e)) / (2 * h)
        assert (fd - grad[:, j]).abs().max() < 1e-8


def test_reference_nearest_lookup_returns_node_values_and_stored_gradients():
    g = torch.Generator().manual_seed(4)
    sdf, grad = torch.rand((5, 6), generator=g), torch.rand((5, 6, 4), generator=g)
    gf = GridField(sdf, [0.0, 0.0], 0.5, mode="nearest", grad=grad)
    pos = gf.node_positions()                                          # [5, 6, 2]
    p = (pos + 0.2 * (torch.rand(pos.shape, generator=g, dtype=torch.float64) - 0.5)).requires_grad_(True)   # within 0.1 < cell / 2 of its node
    val = gf.sdf(p)
    assert torch.equal(val.detach(), sdf.double())
    gr = torch.autograd.grad((val * 2.0).sum(), p)[0]
    assert torch.equal(gr, 2.0 * grad[..., :2].double())
    # half-way points round to the EVEN node (torch.round), beyond the box the edge node answers
    q = torch.tensor([[0.25, 0.0], [0.75, 0.0], [-3.0, 9.0]], dtype=torch.float64)
    assert torch.equal(gf.node_index(q), torch.tensor([0, 2, 4 * 6 + 0]))
    assert gf.discontinuity_distance(q)[:2].max() < 1e-12 and gf.discontinuity_distance(q)[2] == 0.5
