"""CPU checks of the occupancy transform (csrc/edt.hpp): the brute-force reference (tests/edt_ref.py) against scipy's exact transform, the three
symbols of the C ABI, every host-side refusal of the launchers through the C ABI (host buffers stand in for device pointers: nothing is launched,
the method of tests/test_grid_sdf_cpu.py), and the refusals of the Python surface."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import edt_ref

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("mpdx_sdf_grid_edt_ws_bytes", "mpdx_sdf_grid_from_occupancy", "mpdx_occupancy_from_points")


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_d2_equals_scipy():
    """3 % random occupancy from ONE generator seeded 0, drawn for the three shapes in this order; the recorded maxima pin the draw"""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for shape, max_d2 in [((9, 13, 17), 21), ((1, 33, 65), 74), ((5, 7, 70), 25)]:
        occ = rng.random(shape) < 0.03
        assert occ.any() and not occ.all()
        want = np.where(occ, ndi.distance_transform_edt(occ), ndi.distance_transform_edt(~occ))
        want = np.rint(want ** 2).astype(np.int32)
        got = edt_ref.d2_ref(occ)
        print(f"{shape}: occupied {int(occ.sum())}, max d2 {int(got.max())}")
        assert got.dtype == np.int32 and np.array_equal(got, want), shape
        assert int(got.max()) == max_d2, shape


def test_reference_formulas_on_a_hand_case():
    occ = np.zeros((1, 3, 4), np.uint8)
    occ[0, 1, 1] = 1
    d2 = edt_ref.d2_ref(occ)
    assert d2[0].tolist() == [[2, 1, 2, 5], [1, 1, 1, 4], [2, 1, 2, 5]]
    s = edt_ref.sdf_ref(d2, occ, 0.5, 0.25)
    assert s.dtype == np.float32
    assert s[0, 1, 0] == 0.5 * 0.5 - 0.25 and s[0, 1, 1] == -(0.5 * 0.5) - 0.25 and s[0, 1, 3] == 0.5 * 1.5 - 0.25     # face at half a cell
    g = edt_ref.grad_ref(s, 0.5)
    assert g.shape == (1, 3, 4, 4) and not g[..., 2:].any()
    assert g[0, 1, 0, 0] == (s[0, 1, 1] - s[0, 1, 0]) * np.float32(2.0) and g[0, 1, 2, 0] == (s[0, 1, 3] - s[0, 1, 1]) * np.float32(1.0)
    # no node of the other side: the sentinel
    assert (edt_ref.d2_ref(np.zeros((2, 3, 4))) == 81).all() and (edt_ref.d2_ref(np.ones((1, 3, 4))) == 64).all()
    # voxelisation: half to even, dropped (not clamped) outside, non-finite dropped, z ignored in 2-D
    pts = np.array([[0.25, 0.0, 9.0], [0.75, 0.5, np.nan], [-0.3, 0.0, 0.0], [np.nan, 0.0, 0.0], [np.inf, 0.5, 0.0], [1.74, 1.0, 0.0]], np.float32)
    v = edt_ref.voxelise_ref(pts, (1, 3, 4), [0.0, 0.0, 0.0], 0.5)
    assert sorted(zip(*[a.tolist() for a in np.nonzero(v[0])])) == [(0, 0), (1, 2), (2, 3)]


# ---------------------------------------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_three_symbols_are_declared_exported_and_bound(lib):
    from mpd_public_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mpdx.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert re.search(rf" T {name}\b", out), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert lib.mpdx_sdf_grid_edt_ws_bytes.restype is C.c_size_t
    n3 = lambda *v: C.byref((C.c_int * 3)(*v))
    assert lib.mpdx_sdf_grid_edt_ws_bytes(n3(17, 13, 9)) == 2 * 4 * 17 * 13 * 9
    assert lib.mpdx_sdf_grid_edt_ws_bytes(n3(65, 33, 1)) == 2 * 4 * 65 * 33
    assert lib.mpdx_sdf_grid_edt_ws_bytes(n3(4096, 4096, 32)) == 2 * 4 * (1 << 29)
    assert lib.mpdx_sdf_grid_edt_ws_bytes(None) == 0 and "n is null" in lib.mpdx_last_error().decode()
    for bad in ((1, 4, 4), (4, 1, 1), (4097, 2, 2), (4, 4, 0), (4, 4, 4097), (4096, 4096, 33)):
        assert lib.mpdx_sdf_grid_edt_ws_bytes(n3(*bad)) == 0, bad
        assert "n" in lib.mpdx_last_error().decode()


def _transform_args():
    """a VALID call of mpdx_sdf_grid_from_occupancy on host buffers (never made: every test below breaks one argument first)"""
    n = (4, 3, 2)
    nodes = 24
    grad = (C.c_float * (4 * nodes + 8))()
    g0 = C.addressof(grad)
    g0 += (-g0) % 16
    b = dict(occ=(C.c_uint8 * nodes)(), sdf=(C.c_float * nodes)(), grad=grad, d2=(C.c_int32 * nodes)(), ws=(C.c_int32 * (2 * nodes))())
    a = lambda x: C.cast(x, C.c_void_p)
    kw = dict(occ=a(b["occ"]), sdf_out=a(b["sdf"]), grad_out=C.c_void_p(g0), d2_out=a(b["d2"]), n=n, cell=0.1, inflate=0.0, ws=a(b["ws"]), ws_bytes=8 * nodes)
    return kw, b


def _transform(lib, kw):
    rc = lib.mpdx_sdf_grid_from_occupancy(kw["occ"], kw["sdf_out"], kw["grad_out"], kw["d2_out"], C.byref((C.c_int * 3)(*kw["n"])), kw["cell"], kw["inflate"],
                                          kw["ws"], kw["ws_bytes"], None)
    return rc, lib.mpdx_last_error().decode()


TRANSFORM_REFUSALS = [
    ("occ null", dict(occ=None), "occ"),
    ("sdf_out null", dict(sdf_out=None), "sdf_out"),
    ("ws null", dict(ws=None), "ws"),
    ("one node along x", dict(n=(1, 3, 2)), "n[0]"),
    ("one node along y", dict(n=(4, 1, 1)), "n[1]"),
    ("too many along x", dict(n=(4097, 3, 2)), "n[0]"),
    ("too many along y", dict(n=(4, 4097, 2)), "n[1]"),
    ("too many along z", dict(n=(4, 3, 4097)), "n[2]"),
    ("zero along z", dict(n=(4, 3, 0)), "n[2]"),
    ("negative along z", dict(n=(4, 3, -1)), "n[2]"),
    ("more than 2^29 nodes", dict(n=(4096, 4096, 33)), "nodes"),
    ("cell zero", dict(cell=0.0), "cell"),
    ("cell negative", dict(cell=-0.1), "cell"),
    ("cell inf", dict(cell=float("inf")), "cell"),
    ("cell nan", dict(cell=float("nan")), "cell"),
    ("inflate negative", dict(inflate=-1e-3), "inflate"),
    ("inflate inf", dict(inflate=float("inf")), "inflate"),
    ("inflate nan", dict(inflate=float("nan")), "inflate"),
    ("grad_out misaligned", "misalign", "grad_out"),
    ("ws_bytes short", dict(ws_bytes=8 * 24 - 1), "ws_bytes"),
    ("ws_bytes zero", dict(ws_bytes=0), "ws_bytes"),
]


@pytest.mark.parametrize("what,change,needle", TRANSFORM_REFUSALS, ids=[r[0].replace(" ", "_") for r in TRANSFORM_REFUSALS])
def test_transform_refuses_on_the_host_without_launching(lib, what, change, needle):
    kw, bufs = _transform_args()
    if change == "misalign":
        kw["grad_out"] = C.c_void_p(kw["grad_out"].value + 4)
    else:
        kw.update(change)
    for k in ("sdf", "d2", "ws"):
        C.memset(bufs[k], 0x5A, C.sizeof(bufs[k]))
    before = {k: bytes(bufs[k]) for k in ("sdf", "grad", "d2", "ws")}
    rc, msg = _transform(lib, kw)
    assert rc == -1 and needle in msg, (what, rc, msg)
    assert {k: bytes(bufs[k]) for k in before} == before, what     # nothing ran


def test_transform_takes_null_optional_outputs_as_far_as_the_host_checks_go(lib):
    """grad_out and d2_out may be null: with them null the NEXT refusal in line answers, not a null-pointer one"""
    kw, _ = _transform_args()
    kw.update(grad_out=None, d2_out=None, ws_bytes=0)
    rc, msg = _transform(lib, kw)
    assert rc == -1 and "ws_bytes" in msg


def _voxel(lib, points, n_points, occ, n=(4, 3, 2), origin=(0.0, 0.0, 0.0), cell=0.1, origin_null=False):
    org = None if origin_null else C.byref((C.c_float * 3)(*origin))
    rc = lib.mpdx_occupancy_from_points(points, n_points, occ, C.byref((C.c_int * 3)(*n)), org, cell, None)
    return rc, lib.mpdx_last_error().decode()


def test_voxelise_refuses_on_the_host_without_launching(lib):
    pts = (C.c_float * 12)()
    occ = (C.c_uint8 * 24)()
    p, o = C.cast(pts, C.c_void_p), C.cast(occ, C.c_void_p)
    for what, kw, needle in [("n_points negative", dict(points=p, n_points=-1, occ=o), "n_points"),
                             ("points null", dict(points=None, n_points=4, occ=o), "points"),
                             ("occ null", dict(points=p, n_points=4, occ=None), "occ"),
                             ("origin null", dict(points=p, n_points=4, occ=o, origin_null=True), "origin"),
                             ("one node along y", dict(points=p, n_points=4, occ=o, n=(4, 1, 1)), "n[1]"),
                             ("too many along x", dict(points=p, n_points=4, occ=o, n=(4097, 3, 2)), "n[0]"),
                             ("zero along z", dict(points=p, n_points=4, occ=o, n=(4, 3, 0)), "n[2]"),
                             ("more than 2^29 nodes", dict(points=p, n_points=4, occ=o, n=(4096, 4096, 33)), "nodes"),
                             ("cell zero", dict(points=p, n_points=4, occ=o, cell=0.0), "cell"),
                             ("cell nan", dict(points=p, n_points=4, occ=o, cell=float("nan")), "cell")]:
        rc, msg = _voxel(lib, **kw)
        assert rc == -1 and needle in msg, (what, rc, msg)
    assert not any(occ)
    # no points: a successful no-op (with or without a points pointer), nothing is launched
    assert _voxel(lib, None, 0, o)[0] == 0 and _voxel(lib, p, 0, o)[0] == 0
    assert not any(occ)


# ---------------------------------------------------------------------------------------------------------------- Python surface
def test_python_refusals():
    import mpd_public_amd as m
    from mpd_public_amd.planning import GridSDF
    occ = np.zeros((5, 6), bool)
    occ[2, 3] = True
    # no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GridSDF.from_occupancy(occ, [0.0, 0.0], 0.1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GridSDF.from_points(np.zeros((3, 3), np.float32), [-1, -1], [1, 1], 0.1, device="cpu")
    # malformed inputs, refused before any device is touched
    with pytest.raises(ValueError, match="occupancy"):
        GridSDF.from_occupancy(np.zeros(5, bool), [0.0], 0.1, device="cpu")
    with pytest.raises(ValueError, match="bool or uint8"):
        GridSDF.from_occupancy(np.zeros((5, 6), np.float32), [0.0, 0.0], 0.1, device="cpu")
    # a grid that was not made from an occupancy map has none to update
    plain = GridSDF(torch.zeros(5, 6), [0.0, 0.0], 0.1)
    with pytest.raises(ValueError, match="from_occupancy"):
        plain.update_occupancy(occ=occ)
    assert plain.occupancy() is None and plain.inflate == 0.0
    # a RobotChain keeps refusing any grid, a GridSDF instance included
    chain = m.RobotChain.panda()
    g3 = GridSDF(torch.zeros(4, 4, 4), [0.0, 0.0, 0.0], 0.1)
    with pytest.raises(ValueError, match="no signed-distance grid"):
        m.TrajectoryDataset("EnvSpheres3D", chain, sdf_grid=g3)
    env = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda").env
    with pytest.raises(ValueError, match="no signed-distance grid"):
        m.PlanningTask(env, chain, sdf_grid=g3)
    assert "GridSDF" in m.__all__ and m.GridSDF is GridSDF


def test_update_occupancy_refuses_another_shape():
    """the planes are re-used, so the shape is fixed: checked on a grid whose device state is stood in for by host tensors (nothing is launched)"""
    from mpd_public_amd.planning import GridSDF
    g = GridSDF(torch.zeros(5, 6), [0.0, 0.0], 0.1)
    g._occ = torch.zeros(30, dtype=torch.uint8)
    with pytest.raises(ValueError, match="shape"):
        g.update_occupancy(occ=np.zeros((6, 5), bool))
    with pytest.raises(ValueError, match="shape"):
        g.update_occupancy(occ=np.zeros((2, 5, 6), bool))
    with pytest.raises(ValueError, match="occ, points or both"):
        g.update_occupancy()
    assert not g._occ.any()


def test_task_and_dataset_take_a_grid_instance_and_keep_the_dict_form():
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    from mpd_public_amd.planning import GridSDF
    g2 = GridSDF(torch.zeros(5, 6), [-1.0, -1.0], 0.4)
    ds = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass", sdf_grid=g2)
    assert ds.task.df_collision_objects.kind == _lib.FIELD_GRID and ds.task.df_collision_objects.grid is g2 and ds.task.sdf_grid is g2
    kinds = [f.kind for f in ds.task.get_collision_fields()]
    base = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass")
    assert kinds == [(_lib.FIELD_GRID if f is base.task.df_collision_objects else f.kind) for f in base.task.get_collision_fields()]
    with pytest.raises(ValueError, match="3-D GridSDF"):
        m.TrajectoryDataset("EnvSimple2D", "RobotPointMass", sdf_grid=GridSDF(torch.zeros(4, 4, 4), [0.0, 0.0, 0.0], 0.1))
    d = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass", sdf_grid=dict(cell_size=0.02, mode="nearest")).task
    assert d.sdf_grid == dict(cell_size=0.02, mode="nearest") and d.df_collision_objects.grid.sdf is None
    with pytest.raises(ValueError):
        m.TrajectoryDataset("EnvSimple2D", "RobotPointMass", sdf_grid=dict(cell_size=0.02, inflate=0.1))
    import inspect
    from mpd_public_amd import inference
    sig = inspect.signature(inference.experiment)
    assert sig.parameters["sdf_grid"].default is None and sig.parameters["sdf_grid_cell_size"].default is None
    # refresh_grids exists on the guide and the task and is a no-op before anything was compiled
    from helpers import product_guide
    product_guide(ds).refresh_grids()
    ds.task.refresh_grids()
