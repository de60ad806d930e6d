"""CPU tests of the tool-axis constraint (planning.CostToolAxis; the tool members of mpdx_guide_params): the argument checks, the packing into the
appended members, the C header against the ctypes mirror, and that the fp64 reference of tests/tool_ref.py can fail - two wrong fp32 variants of
itself miss the yardstick the GPU test holds the kernel to."""
import ctypes as C
import math
import pathlib
import shutil
import subprocess

import numpy as np
import pytest
import torch

from chain_ref import chain_trajs, description, mismatch_fraction, probe_configs, product_robot
import tool_ref as tr

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _r3():
    return product_robot("R3")


# ---------------------------------------------------------------------------------------------------------------- 1. argument checks
def test_cost_tool_axis_argument_checks():
    import mpd_public_amd as m
    rob = _r3()
    c = m.CostToolAxis(rob, 64)
    assert c.frame == 3 and c.max_tilt == 0.1 and np.allclose(c.axis, [0, 0, 1]) and np.allclose(c.world_axis, [0, 0, 1])
    c = m.CostToolAxis(rob, 64, frame=2, axis=(0.1, 0.2, 1), world_axis=(0, 3, 4), max_tilt=0.5)
    assert c.frame == 2 and c.axis.dtype == np.float64 and abs(np.linalg.norm(c.axis) - 1) < 1e-15 and np.allclose(c.world_axis, [0, 0.6, 0.8], atol=1e-15)
    assert c.cos_min == math.cos(0.5)
    for bad in [dict(axis=(0, 0, 0)), dict(world_axis=(0, 0, 0)), dict(axis=(float("nan"), 0, 1)), dict(world_axis=(0, float("inf"), 1)), dict(axis=(1, 0)),
                dict(frame=0), dict(frame=4), dict(frame=-1), dict(frame=1.5), dict(max_tilt=-0.01), dict(max_tilt=math.pi + 0.01), dict(max_tilt=float("nan"))]:
        with pytest.raises(ValueError):
            m.CostToolAxis(rob, 64, **bad)
    m.CostToolAxis(rob, 64, max_tilt=0.0), m.CostToolAxis(rob, 64, max_tilt=math.pi), m.CostToolAxis(rob, 64, frame=1)
    for other in (m.make_robot("RobotPanda"), m.make_robot("RobotPointMass"), m.make_robot("RobotPointMass3D")):
        with pytest.raises(ValueError, match=r"RobotChain\.panda\(\)"):
            m.CostToolAxis(other, 64)


# ---------------------------------------------------------------------------------------------------------------- 2. packing
def _build(rob, costs, weights):
    from mpd_public_amd.guides import build_device_params
    lo, hi = rob.limits()
    return build_device_params(rob, 3, 0.05, lo, hi, costs, weights, True, 128, True, 1.0, "cpu")[0]


def _tool_members(gp):
    return (gp.tool_frame, tuple(gp.tool_axis), tuple(gp.tool_world), gp.tool_cos_min, gp.tool_weight)


def test_build_device_params_packs_the_tool_members():
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    rob = _r3()
    task = m.PlanningTask(m.make_env("EnvSpheres3D"), rob)
    coll = [m.CostCollision(rob, 64, field=f) for f in task.get_collision_fields()]
    gpc = m.CostGPTrajectory(rob, 64, 5.0 / 64)
    tool = m.CostToolAxis(rob, 64, frame=2, axis=(0.1, 0.2, 1), world_axis=(0.2, -0.3, 1), max_tilt=0.7)
    assert len(coll) == _lib.MAX_FIELDS      # a chain with pairs and extra objects uses every field slot: the term has members of its own
    base = _build(rob, coll + [gpc], [1e-2] * 4 + [1e-7])
    assert _tool_members(base) == (0, (0.0,) * 3, (0.0,) * 3, 0.0, 0.0)
    full = _build(rob, coll + [tool, gpc], [1e-2] * 4 + [3e-2, 1e-7])
    assert full.tool_frame == 2 and full.tool_cos_min == np.float32(math.cos(0.7)) and full.tool_weight == np.float32(3e-2)
    assert np.array_equal(np.array(full.tool_axis), tr.unit((0.1, 0.2, 1)).astype(np.float32))
    assert np.array_equal(np.array(full.tool_world), tr.unit((0.2, -0.3, 1)).astype(np.float32))
    assert abs(np.linalg.norm(np.array(full.tool_axis, np.float64)) - 1) < 1e-6
    # everything else is what it is without the term
    assert full.n_fields == base.n_fields == 4 and np.array_equal(full.table_host, base.table_host) and full.n_prim_floats == base.n_prim_floats
    assert all(bytes(full.fields[i]) == bytes(base.fields[i]) for i in range(_lib.MAX_FIELDS))
    assert (full.use_gp, full.gp_weight, full.dt) == (base.use_gp, base.gp_weight, base.dt) and full.n_chain_floats == base.n_chain_floats
    # the term alone, and with the GP term: valid composites without a field
    alone = _build(rob, [tool], [1e-2])
    assert alone.n_fields == 0 and alone.use_gp == 0 and alone.tool_frame == 2 and alone.tool_weight == np.float32(1e-2)
    with_gp = _build(rob, [tool, gpc], [1e-2, 1e-7])
    assert with_gp.n_fields == 0 and with_gp.use_gp == 1 and with_gp.tool_frame == 2
    # one term only; unknown types are still refused
    with pytest.raises(NotImplementedError):
        _build(rob, [tool, m.CostToolAxis(rob, 64)], [1e-2, 1e-2])
    with pytest.raises(NotImplementedError):
        _build(rob, [tool, object()], [1e-2, 1e-2])
    with pytest.raises(NotImplementedError):
        _build(rob, [gpc, gpc], [1e-7, 1e-7])


def test_with_scenes_keeps_the_tool_term():
    import mpd_public_amd as m
    from scene_ref import N_PER_CONTEXT, scene_object_sets
    ds = m.TrajectoryDataset("EnvSpheres3D", _r3(), tensor_args={"device": "cpu", "dtype": torch.float32})
    pg, tool = tr.product_guide_tool(ds, 3, 0.7, "full")
    sets = scene_object_sets(3)
    g = pg.with_scenes(m.PlanningScenes(ds.task, [sets[2], sets[1]]), [1, 0], N_PER_CONTEXT)
    gp = g.device_params("cpu")
    assert gp.n_scenes == 2 and gp.tool_frame == 3 and gp.tool_cos_min == np.float32(math.cos(0.7)) and gp.n_fields == 4


# ---------------------------------------------------------------------------------------------------------------- 3. ABI
PARENT_OFFSETS = {"chain": 608, "n_chain_floats": 616}    # of the commit before the tool members existed (sizeof 624)
TOOL_MEMBERS = ["tool_frame", "tool_axis", "tool_world", "tool_cos_min", "tool_weight"]


def test_tool_members_in_the_c_header_match_the_ctypes_mirror(tmp_path):
    from mpd_public_amd import _lib
    G = _lib.GuideParams
    assert [n for n, _ in G._fields_][-len(TOOL_MEMBERS):] == TOOL_MEMBERS           # appended at the end, behind n_chain_floats
    assert [n for n, _ in G._fields_][-len(TOOL_MEMBERS) - 1] == "n_chain_floats"
    assert {k: getattr(G, k).offset for k in PARENT_OFFSETS} == PARENT_OFFSETS
    assert "tool_frame" not in [n for n, _ in _lib.Field._fields_]
    assert "mpdx_traj_tool_metrics" in _lib.SIGNATURES
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on this host")
    names = ["chain", "n_chain_floats"] + TOOL_MEMBERS
    src = tmp_path / "tool_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpdx.h"\nint main(void) { printf("%zu' + " %zu" * len(names) + '\\n", sizeof(mpdx_guide_params), '
                   + ", ".join(f"offsetof(mpdx_guide_params, {n})" for n in names) + "); return 0; }\n")
    exe = tmp_path / "tool_sizes"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(G)] + [getattr(G, n).offset for n in names]
    assert got[1:3] == [PARENT_OFFSETS["chain"], PARENT_OFFSETS["n_chain_floats"]]


# ---------------------------------------------------------------------------------------------------------------- 4. the reference can fail
def _r3_reference(frame):
    """R3, H = 64, the inputs and the tool term of tests/test_gpu_tool_axis.py (tool term alone): (dataset, description, x, fp64 increment)."""
    import mpd_public_amd as m
    desc = description("R3")
    ds = m.TrajectoryDataset("EnvSpheres3D", _r3(), n_support_points=64, tensor_args={"device": "cpu", "dtype": torch.float32})
    x = chain_trajs(3, 3, 64, "chain/R3/64/0", probes=probe_configs("R3", ds))
    og, _ = tr.oracle_guide_tool(ds, desc, tr.ToolAxisRef(desc, frame, tr.MAX_TILT["R3", 64, frame]), "alone")
    return ds, desc, x, og(x.double()).numpy()


@pytest.mark.parametrize("frame,wrong", [(2, "above_frame"), (3, "prismatic_as_revolute"), (2, "prismatic_as_revolute")])
def test_the_reference_can_fail(frame, wrong):
    """fp32 with the stated gradient written by hand agrees with the fp64 autograd reference under the GPU test's yardstick (fewer than 0.5 % of the
    waypoints left out); the same fp32 code with one mistake - the gradient also on the joints above the frame, or prismatic joints treated as
    revolute - misses it (more than 1 % of the waypoints left out)."""
    ds, desc, x, ref = _r3_reference(frame)
    assert np.abs(ref).max() > 0

    def frac(variant):
        og, _ = tr.oracle_guide_tool(ds, desc, tr.ToolAxisRef(desc, frame, tr.MAX_TILT["R3", 64, frame], dtype=torch.float32, wrong=variant), "alone")
        return mismatch_fraction(og(x.float()).numpy(), ref, tr.W_TOOL)[0]

    good, bad = frac("analytic"), frac(wrong)
    print(f"R3 frame {frame}: stated gradient in fp32 leaves out {100 * good:.3f} % of the waypoints, '{wrong}' {100 * bad:.1f} %")
    assert good < 0.005
    assert bad > 0.01
