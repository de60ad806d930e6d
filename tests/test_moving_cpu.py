"""CPU checks of moving obstacles (time-indexed translation tracks; include/mpdx.h, csrc/motion.hpp): the layout of the new members against the C
header, the host-side refusals through the C ABI (host buffers stand in for device pointers, nothing is launched), the refusals of the Python
surface, the fp64 reference (tests/moving_ref.py) held to account, and the reference-only conditions of every GPU case of
tests/test_gpu_moving.py."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import guide_ref as gr
import moving_ref as mr

ROOT = Path(__file__).resolve().parent.parent
H = 64


def _lib_or_skip():
    from mpd_public_amd import build, _lib
    try:
        build.build(verbose=False)
        return _lib.load()
    except _lib.LibraryUnavailable as e:   # pragma: no cover
        pytest.skip(f"libmpdx.so does not load on this host: {e}")


# ---------------------------------------------------------------------------------------------------------------- layout
def test_track_members_match_the_c_header(tmp_path):
    """The track members of mpdx_field share the words of a grid field's plane offsets (anonymous unions): the header and the ctypes mirror agree on
    their offsets, and neither mpdx_field nor mpdx_guide_params changes its size or the offset of any member it had."""
    from mpd_public_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on this host")
    names_f = ["track_len", "track_off", "grid_sdf_off", "grid_grad_off", "n", "mode"]
    names_g = ["fields", "prims", "grids", "n_scenes", "chain", "tool_weight"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpdx.h"\nint main(void) { printf("%zu %zu' + " %zu" * (len(names_f) + len(names_g))
                   + '\\n", sizeof(mpdx_field), sizeof(mpdx_guide_params), ' + ", ".join(f"offsetof(mpdx_field, {n})" for n in names_f) + ", "
                   + ", ".join(f"offsetof(mpdx_guide_params, {n})" for n in names_g) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F, G = _lib.Field, _lib.GuideParams
    assert got == [C.sizeof(F), C.sizeof(G)] + [getattr(F, n).offset for n in names_f] + [getattr(G, n).offset for n in names_g]
    assert F.track_len.offset == F.grid_sdf_off.offset and F.track_off.offset == F.grid_grad_off.offset == F.track_len.offset + 4
    assert F.track_len.size == F.track_off.size == 4
    assert (C.sizeof(F), C.sizeof(G)) == (88, 656)          # what they were before the members existed
    f = F()
    f.track_len, f.track_off = 64, 24
    assert (f.grid_sdf_off, f.grid_grad_off) == (64, 24)    # one word each, two names


def _valid_block(h=H):
    """A well-formed 2-D point-mass block over HOST memory: field 0 static objects (3 spheres, 1 box), field 1 the workspace, field 2 a moving
    sphere whose track lies behind the tables at a multiple of 4."""
    from mpd_public_amd import _lib
    gp = _lib.GuideParams()
    gp.robot, gp.q_dim, gp.ws_dim, gp.interpolate, gp.n_interp, gp.n_fields = _lib.ROBOT_POINTMASS, 2, 2, 1, 128, 3
    f = gp.fields[0]
    f.kind, f.weight, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 1.0, 0, 3, 12, 1      # floats 0 .. 18
    gp.fields[1].kind = _lib.FIELD_WORKSPACE
    for j in range(2):
        gp.fields[1].ws_min[j], gp.fields[1].ws_max[j] = -1.0, 1.0
    f = gp.fields[2]
    f.kind, f.weight, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 1.0, 18, 1, 22, 0     # floats 18 .. 22
    keep = [(C.c_float * (24 + 4 * 128 + 8))()]
    gp.prims, gp.n_prim_floats = C.addressof(keep[0]), 24 + 4 * h
    gp.fields[2].track_len, gp.fields[2].track_off = h, 24
    gp._keep = keep
    return gp


def _call_all(lib, gp, h=H):
    """Every entry point that takes a guide block with tracks, with host buffers: (name, rc, message)."""
    from mpd_public_amd import _lib
    x = (C.c_float * (4 * 128 * 4))()
    out = (C.c_float * (4 * 128 * 4))()
    flag = (C.c_uint32 * 4)()
    ms = C.c_float()
    a = lambda b: C.cast(b, C.c_void_p)
    res = []
    call = lambda name, rc: res.append((name, rc, (lib.mpdx_last_error() or b"").decode()))
    call("mpdx_guide_step", lib.mpdx_guide_step(C.byref(gp), a(x), a(out), None, None, a(flag), None, 4, 4, h, 4, None))
    call("mpdx_guide_step_scaled", lib.mpdx_guide_step_scaled(C.byref(gp), a(x), a(out), None, None, a(flag), None, 4, 4, h, 4, 0.5, None))
    call("mpdx_guide_time", lib.mpdx_guide_time(C.byref(gp), a(x), a(out), a(flag), 4, 4, h, 4, 1, None, C.byref(ms)))
    call("mpdx_guide_variant", lib.mpdx_guide_variant(C.byref(gp), 4, h, 4))
    call("mpdx_traj_metrics", lib.mpdx_traj_metrics(C.byref(gp), a(x), a(out), 64, 4, h, 4, None))
    call("mpdx_traj_metrics_mask", lib.mpdx_traj_metrics_mask(C.byref(gp), a(x), a(out), None, 64, 4, h, 4, None))
    cfg = _lib.UnetCfg(4, h, 32, 3, (C.c_int32 * _lib.MAX_LEVELS)(1, 2, 4), 32)
    hdl = C.c_void_p()
    assert lib.mpdx_unet_create(C.byref(cfg), C.byref(hdl)) == 0
    try:
        coefs = (_lib.StepCoefs * 2)()
        call("mpdx_plan", lib.mpdx_plan(hdl, a(x), a(x), 2, coefs, 0, a(x), None, None, None, None, 4, a(x), C.byref(gp), 1, 3, a(flag), 4, 0, 0, None))
    finally:
        lib.mpdx_unet_destroy(hdl)
    return res


def test_zero_initialised_and_valid_blocks_pass_every_check():
    """All-zero track members: as before the members existed.  Seen without a launch through mpdx_guide_variant, which runs every host check of a
    block and launches nothing - for a block of zeros, for the valid block with its track, and for the same block with the track members zeroed."""
    from mpd_public_amd import _lib
    lib = _lib_or_skip()
    zero = _lib.GuideParams()
    assert lib.mpdx_guide_variant(C.byref(zero), 4, H, 0) == 0, lib.mpdx_last_error()
    gp = _valid_block()
    assert lib.mpdx_guide_variant(C.byref(gp), 4, H, 4) == 0, lib.mpdx_last_error()
    gp.fields[2].track_len = gp.fields[2].track_off = 0
    assert lib.mpdx_guide_variant(C.byref(gp), 4, H, 4) == 0, lib.mpdx_last_error()
    # a track offset without a length is no track
    gp.fields[2].track_off = 3
    assert lib.mpdx_guide_variant(C.byref(gp), 4, H, 4) == 0, lib.mpdx_last_error()


def _refusals():
    from mpd_public_amd import _lib
    out = []

    def case(name, member, fn):
        gp = _valid_block()
        fn(gp)
        out.append((name, member, gp))

    def set_len(f, v):
        return lambda gp: setattr(gp.fields[f], "track_len", v)

    def set_off(f, v):
        return lambda gp: setattr(gp.fields[f], "track_off", v)
    case("track_len is neither 0 nor H", "track_len", set_len(2, H - 1))
    case("track_len negative", "track_len", set_len(2, -H))
    case("a workspace field with a track", "track_len", lambda gp: (set_len(1, H)(gp), set_off(1, 24)(gp)))

    def self_field(gp):      # a fourth field, the self-collision one, with a track
        gp.n_fields, gp.fields[3].kind = 4, _lib.FIELD_SELF
        set_len(3, H)(gp), set_off(3, 24)(gp)
    case("a self-collision field with a track", "track_len", self_field)
    case("track_off negative", "track_off", set_off(2, -4))
    case("track_off not a multiple of 4", "track_off", set_off(2, 26))
    case("the track ends beyond n_prim_floats", "track_off", set_off(2, 28))
    case("n_prim_floats too small for the track", "track_off", lambda gp: setattr(gp, "n_prim_floats", 24 + 4 * H - 1))
    case("the track overlaps the static field's box table", "track_off", set_off(2, 16))
    case("the track overlaps its own field's sphere table", "track_off", set_off(2, 20))

    def second_track(gp):     # field 0 moves too, on rows that overlap field 2's
        gp.n_prim_floats = 24 + 8 * H
        gp.fields[0].track_len, gp.fields[0].track_off = H, 24 + 4 * H - 4
    case("two tracks overlap", "track_off", second_track)

    def scenes(gp):
        gp.n_scenes, gp.scene_stride, gp.scene_n_per_ctx = 2, 28, 2
    case("tracks with several scenes", "track_len", scenes)
    case("tracks with a chain robot", "track_len", lambda gp: setattr(gp, "robot", _lib.ROBOT_CHAIN))
    return out


def test_track_refusals_through_the_c_abi():
    lib = _lib_or_skip()
    cases = _refusals()
    assert len(cases) == 13
    for what, member, gp in cases:
        for name, rc, msg in _call_all(lib, gp):
            assert rc == -1 and member in msg, (what, name, rc, msg)
    # two tracks side by side are fine (the refusal above is the overlap, not the second track)
    gp = _valid_block()
    gp.n_prim_floats = 24 + 8 * H
    gp.fields[0].track_len, gp.fields[0].track_off = H, 24 + 4 * H
    assert lib.mpdx_guide_variant(C.byref(gp), 4, H, 4) == 0, lib.mpdx_last_error()
    # ... and so is a track next to a grid field (checked on members only: the grid's own checks pass on a well-formed descriptor)
    from mpd_public_amd import _lib
    gp = _valid_block()
    g = gp.fields[1]
    g.kind, g.grid_sdf_off, g.grid_grad_off, g.cell, g.mode = _lib.FIELD_GRID, 0, -1, 0.25, _lib.GRID_LINEAR
    g.n[0], g.n[1], g.n[2] = 4, 4, 1
    planes = (C.c_float * 16)()
    gp.grids, gp.n_grid_floats = C.addressof(planes), 16
    assert lib.mpdx_guide_variant(C.byref(gp), 4, H, 4) == 0, lib.mpdx_last_error()


def test_a_track_is_checked_against_the_horizon_of_the_launch():
    """the same block is taken at H = 64 and refused at every other horizon, by every entry point"""
    lib = _lib_or_skip()
    gp = _valid_block(64)
    for name, rc, msg in _call_all(lib, gp, h=32):
        assert rc == -1 and "track_len" in msg and "32" in msg, (name, rc, msg)


def test_planners_and_bake_refuse_any_track():
    from mpd_public_amd import _lib
    lib = _lib_or_skip()
    gp = _valid_block()
    gp.use_gp, gp.dt, gp.sigma_gp = 1, 0.1, 1.0
    buf = (C.c_float * 4096)()
    a = lambda b: C.cast(b, C.c_void_p)
    o = _lib.GpmpOpts(1.0, 10.0, 0.1, 1e-6, 1e6, 1.0, 1)
    assert lib.mpdx_gpmp_step(C.byref(gp), C.byref(o), a(buf), a(buf), a(buf), 1, H, 4, 1, None) == -1
    assert "track_len" in lib.mpdx_last_error().decode()
    r = _lib.RrtOpts()
    r.step, r.max_nodes, r.max_iters, r.max_connect_steps, r.n_edge_checks = 0.1, 64, 16, 4, 4
    assert lib.mpdx_rrt_connect(C.byref(gp), C.byref(r), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), 1, None) == -1
    assert "track_len" in lib.mpdx_last_error().decode()
    assert lib.mpdx_rrt_paths(C.byref(gp), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), None, 1, 64, H, 0.1, 4, 1, None) == -1
    assert "track_len" in lib.mpdx_last_error().decode()
    n, org = (C.c_int * 3)(8, 8, 1), (C.c_float * 3)(-1.0, -1.0, 0.0)
    assert lib.mpdx_sdf_grid_bake(C.byref(gp), 0, a(buf), None, C.byref(n), C.byref(org), 0.25, None) == -1
    assert "track_len" in lib.mpdx_last_error().decode()


def test_panda_dense_variant_falls_back_when_the_track_no_longer_fits():
    """guide_takes_dense: the dense variant where its layout fits 80 KB.  A Panda block at B = 512 whose static tables leave less room than a track needs
    is dense without the track and takes the table variant with it (mpdx_guide_variant: the launcher's own rule, no launch)."""
    from mpd_public_amd import _lib
    lib = _lib_or_skip()
    gp = _lib.GuideParams()
    gp.robot, gp.q_dim, gp.ws_dim, gp.interpolate, gp.n_interp, gp.n_fields = _lib.ROBOT_PANDA, 7, 3, 1, 128, 2
    n_static = 360      # spheres of the static field: 1440 floats; the dense layout at H = 64, N = 128 leaves room for about 1620
    f = gp.fields[0]
    f.kind, f.weight, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 1.0, 0, n_static, 4 * n_static, 0
    f = gp.fields[1]
    f.kind, f.weight, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 1.0, 4 * n_static, 1, 4 * n_static + 4, 0
    keep = (C.c_float * (4 * n_static + 4 + 4 * H))()
    gp.prims, gp.n_prim_floats = C.addressof(keep), 4 * n_static + 4
    assert lib.mpdx_guide_variant(C.byref(gp), 512, H, 14) == 1, lib.mpdx_last_error()
    gp.n_prim_floats = 4 * n_static + 4 + 4 * H
    gp.fields[1].track_len, gp.fields[1].track_off = H, 4 * n_static + 4
    assert lib.mpdx_guide_variant(C.byref(gp), 512, H, 14) == 0, lib.mpdx_last_error()
    # a small table stays dense with its track
    f = gp.fields[0]
    f.n_spheres, f.box_off = 15, 60
    gp.fields[1].sphere_off, gp.fields[1].box_off = 60, 64
    gp.n_prim_floats, gp.fields[1].track_off = 64 + 4 * H, 64
    assert lib.mpdx_guide_variant(C.byref(gp), 512, H, 14) == 1, lib.mpdx_last_error()


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_object_set_track_and_packing():
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    from mpd_public_amd.guides import build_device_params
    from mpd_public_amd.planning import ObjectSet, PlanningTask
    o = mr.moving_set(2, H, track=None)
    assert o.track is None and ObjectSet.empty().track is None
    lin = o.with_linear_motion((0.0, -0.5), (0.25, 0.5), H)
    assert lin.track.shape == (H, 2) and lin.track.dtype == np.float32 and o.track is None
    np.testing.assert_allclose(lin.track[0], (0.0, -0.5))
    np.testing.assert_allclose(lin.track[-1], (0.25, 0.5))
    np.testing.assert_allclose(np.diff(lin.track, axis=0), np.tile(np.float32([0.25, 1.0]) / (H - 1), (H - 1, 1)), atol=1e-6)    # constant velocity
    rows = lin.track_rows(H)
    assert rows.shape == (H, 4) and not rows[:, 2:].any()
    ds = mr.dataset("pm2-H64")
    task = ds.task
    assert [f.name for f in task.get_collision_fields()] == ["objects", "workspace", "extra_objects", "moving_objects"]
    assert task.get_collision_fields_moving_objects() == [task.df_collision_moving_objects] and task.has_tracks
    costs = [m.CostCollision(ds.robot, H, field=f) for f in task.get_collision_fields()]
    gp, prims = build_device_params(ds.robot, 2, 0.05, None, None, costs, [1.0] * 4, True, 128, True, 1.0, "cpu")
    f = gp.fields[3]
    assert [gp.fields[i].track_len for i in range(4)] == [0, 0, 0, H] and f.track_off % 4 == 0 and f.track_off + 4 * H == gp.n_prim_floats
    assert f.track_off >= f.box_off + 6 * f.n_boxes and (f.n_spheres, f.n_boxes) == (2, 1)
    got = gp.table_host[f.track_off: f.track_off + 4 * H].reshape(H, 4)
    np.testing.assert_array_equal(got[:, :2], mr.bend_track(H, 2))
    assert not got[:, 2:].any()
    # the tables in front of the track are those of the static task
    static = mr.dataset("pm2-H64", track=None)
    gs, _ = build_device_params(static.robot, 2, 0.05, None, None, [m.CostCollision(static.robot, H, field=f) for f in static.task.get_collision_fields()],
                                [1.0] * 4, True, 128, True, 1.0, "cpu")
    assert [(gs.fields[i].track_len, gs.fields[i].track_off) for i in range(4)] == [(0, 0)] * 4
    np.testing.assert_array_equal(gs.table_host[: gs.n_prim_floats], gp.table_host[: gs.n_prim_floats])
    assert _lib.MAX_FIELDS == 4
    # the default task is untouched
    base = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass").task
    assert not base.has_tracks and [f.name for f in base.get_collision_fields()] == ["objects", "workspace", "extra_objects"]
    assert isinstance(PlanningTask(base.env, base.robot, moving_objects=lin), PlanningTask)


def test_python_surface_refusals():
    """every refusal is a ValueError that says why, raised before any device work (there is no device here)"""
    import mpd_public_amd as m
    from mpd_public_amd import generate_trajectories as gt
    from mpd_public_amd.guides import build_device_params
    from mpd_public_amd.planning import GridSDF, ObjectSet, PlanningScenes, PlanningTask, RobotChain, make_env
    ds = mr.dataset("pm2-H64")
    task = ds.task
    mv = mr.moving_set(2, H)
    # a track of another length than the horizon
    costs = [m.CostCollision(ds.robot, 32, field=f) for f in task.get_collision_fields()]
    with pytest.raises(ValueError, match="n_support_points"):
        build_device_params(ds.robot, 2, 0.05, None, None, costs, [1.0] * 4, True, 128, True, 1.0, "cpu")
    with pytest.raises(ValueError, match="n_support_points"):
        task.trajectory_metrics(torch.zeros(2, 32, 4))
    with pytest.raises(ValueError, match="track"):
        ObjectSet(mv.sphere_centers, mv.sphere_radii, mv.box_centers, mv.box_half, np.zeros((H, 5), np.float32)).track_rows(H)
    # a moving set without a track; more fields than the kernels take
    with pytest.raises(ValueError, match="no track"):
        PlanningTask(ds.env, ds.robot, moving_objects=mr.moving_set(2, H, track=None))
    panda = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda")
    with pytest.raises(ValueError, match="self, objects, workspace, extra_objects, moving_objects"):
        PlanningTask(panda.env, panda.robot, moving_objects=mr.moving_set(3, H))
    assert PlanningTask(panda.env, panda.robot, use_extra_objects=False, moving_objects=mr.moving_set(3, H)).has_tracks
    # scenes
    with pytest.raises(ValueError, match="scene"):
        PlanningScenes(task, [ds.env.obj_extra, ds.env.obj_extra])
    plain = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass").task
    with pytest.raises(ValueError, match="track"):
        PlanningScenes(plain, [plain.env.obj_extra, mv])
    # a chain robot
    chain = RobotChain.panda()
    with pytest.raises(ValueError, match="RobotChain"):
        PlanningTask(make_env("EnvSpheres3D"), chain, use_extra_objects=False, moving_objects=mr.moving_set(3, H))
    fld = PlanningTask(panda.env, panda.robot, use_extra_objects=False, moving_objects=mr.moving_set(3, H)).df_collision_moving_objects
    with pytest.raises(ValueError, match="RobotChain"):
        build_device_params(chain, 3, 0.05, None, None, [m.CostCollision(chain, H, field=fld)], [1.0], True, 128, True, 1.0, "cpu")
    # the baseline planners
    q = torch.zeros(3, 2)
    with pytest.raises(ValueError, match="edges_free"):
        gt.edges_free(task, q, q)
    with pytest.raises(ValueError, match="RRTConnectBatch"):
        gt.RRTConnectBatch(task, q[0], q[1], 3)
    with pytest.raises(ValueError, match="GPMP2"):
        gt.GPMP2(ds, 5.0 / H)
    with pytest.raises(ValueError, match="moving obstacle"):
        task._params("cpu")
    # a grid of a moving set
    with pytest.raises(ValueError, match="does not move"):
        GridSDF.for_primitives(mv, task.ws_min, task.ws_max, 0.05)
    env = mr.gr.cover_env(2)
    env.obj_fixed = mr.moving_set(2, H)
    with pytest.raises(ValueError, match="does not move"):
        PlanningTask(env, ds.robot, sdf_grid=dict(cell_size=0.05))
    assert PlanningTask(env, ds.robot).has_tracks       # ... while as primitives a fixed set may move
    # experiment's option
    from mpd_public_amd.inference import _moving_sphere_set
    s = _moving_sphere_set(((0.0, -0.8), (0.0, 0.8), 0.2), "EnvSimple2D")
    assert s.track.shape == (64, 2) and s.sphere_radii.tolist() == pytest.approx([0.2])
    np.testing.assert_allclose(s.sphere_centers[0, :2] + s.track[-1], (0.0, 0.8), atol=1e-6)
    for bad in (((0.0, 0.0, 0.0), (0.0, 0.8), 0.2), ((0.0, 0.0), (0.0, 0.8), -1.0), (1.0, 2.0)):
        with pytest.raises(ValueError, match="moving_sphere"):
            _moving_sphere_set(bad, "EnvSimple2D")


def test_refresh_grids_reaches_every_block_of_a_task_with_a_track():
    """A track next to a grid field: the task keeps one metrics block per horizon (and one of its static fields), each with a grid buffer of its own
    where the planes are concatenated (nearest mode: sdf + gradient plane).  After the planes were rewritten in place - what GridSDF.update_occupancy /
    update_mesh do - task.refresh_grids() copies them again into EVERY block; without it the blocks keep the old planes."""
    import mpd_public_amd as m
    from mpd_public_amd import _lib
    from mpd_public_amd.planning import GridSDF, PlanningTask
    g = torch.Generator().manual_seed(11)
    grid = GridSDF(torch.rand((7, 9), generator=g), np.float32([-1.0, -1.0]), 0.25, mode="nearest", grad=torch.rand((7, 9, 2), generator=g))
    base = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass")
    task = PlanningTask(base.env, base.robot, sdf_grid=grid, moving_objects=mr.moving_set(2, H))
    assert task.has_tracks and task.df_collision_objects.kind == _lib.FIELD_GRID
    blocks = [task._params("cpu", H), task._params("cpu", static_only=True)]
    other = PlanningTask(base.env, base.robot, sdf_grid=grid, moving_objects=mr.moving_set(2, 32))
    blocks.append(other._params("cpu", 32))
    sdf_p, grad_p = grid.planes("cpu")
    n = sdf_p.numel()
    for gp in blocks:
        k = [i for i in range(gp.n_fields) if gp.fields[i].kind == _lib.FIELD_GRID][0]
        assert gp.grids_tensor.data_ptr() != sdf_p.data_ptr()                  # a concatenation: the block's own buffer
        assert torch.equal(gp.grids_tensor[gp.fields[k].grid_sdf_off: gp.fields[k].grid_sdf_off + n], sdf_p)
    assert len(task._gp_by_h) == 2 and getattr(task, "_gp", None) is None
    old = sdf_p.clone()
    sdf_p.add_(1.0)                                                            # the planes rewritten in place (a new perception frame)
    grad_p.mul_(-1.0)
    for gp in blocks:
        k = [i for i in range(gp.n_fields) if gp.fields[i].kind == _lib.FIELD_GRID][0]
        assert torch.equal(gp.grids_tensor[gp.fields[k].grid_sdf_off: gp.fields[k].grid_sdf_off + n], old)      # stale until refreshed
    task.refresh_grids()
    other.refresh_grids()
    for gp in blocks:
        k = [i for i in range(gp.n_fields) if gp.fields[i].kind == _lib.FIELD_GRID][0]
        f = gp.fields[k]
        assert torch.equal(gp.grids_tensor[f.grid_sdf_off: f.grid_sdf_off + n], sdf_p)
        assert torch.equal(gp.grids_tensor[f.grid_grad_off: f.grid_grad_off + grad_p.numel()], grad_p)
    # a new track array is a new block; the cache is bounded
    task.df_collision_moving_objects.objects.track = mr.bend_track(H, 2, amp=0.1)
    gp2 = task._params("cpu", H)
    assert gp2 is not blocks[0] and len(task._gp_by_h) == 3
    t_off = [gp2.fields[i].track_off for i in range(gp2.n_fields) if gp2.fields[i].kind == _lib.FIELD_OBJECTS and gp2.fields[i].track_len][0]
    np.testing.assert_array_equal(gp2.table_host[t_off: t_off + 4 * H].reshape(H, 4)[:, :2], mr.bend_track(H, 2, amp=0.1))
    for k in range(12):
        task.df_collision_moving_objects.objects.track = mr.bend_track(H, 2, amp=0.01 * (k + 1))
        task._params("cpu", H)
    assert len(task._gp_by_h) <= 8


def test_a_non_finite_track_is_refused_before_it_reaches_a_block():
    """The kernels cannot fault on a NaN track entry, but what a box then reports is not defined (include/mpdx.h): the Python side refuses it."""
    import mpd_public_amd as m
    from mpd_public_amd.guides import build_device_params
    from mpd_public_amd.planning import PlanningTask
    base = m.TrajectoryDataset("EnvSimple2D", "RobotPointMass")
    for bad in (float("nan"), float("inf")):
        mv = mr.moving_set(2, H)
        mv.track[H // 2, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            mv.track_rows(H)
        task = PlanningTask(base.env, base.robot, moving_objects=mv)
        with pytest.raises(ValueError, match="non-finite"):
            build_device_params(base.robot, 2, 0.05, None, None, [m.CostCollision(base.robot, H, field=f) for f in task.get_collision_fields()], [1.0] * 4,
                                True, 128, True, 1.0, "cpu")
        with pytest.raises(ValueError, match="non-finite"):
            task.trajectory_metrics(torch.zeros(2, H, 4))


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def _static_oracle(name, shift=None):
    """fp64 oracle of the case's task with the moving set static (its centres shifted by `shift`)"""
    ds = mr.dataset(name, track=None)
    if shift is not None:
        o = ds.task.df_collision_moving_objects.objects
        s = np.zeros(3, np.float32)
        s[: len(shift)] = shift
        o.sphere_centers, o.box_centers = o.sphere_centers + s, o.box_centers + s
    og, _, _ = mr.oracle(ds, n_interp=mr.CASES[name]["n_interp"])
    return og


@pytest.mark.parametrize("name", ["pm2-H64", "pm2-H64-nointerp", "pm3-H24", "panda-H64"])
def test_reference_zero_and_constant_tracks(name):
    c = mr.CASES[name]
    dim = gr.ROBOTS[c["robot_id"]][1]
    x = mr.trajs(name).double()
    static = _static_oracle(name)(x).numpy()
    assert np.abs(static).max() > 0
    og0, _, _ = mr.oracle(mr.dataset(name, track="zero"), n_interp=c["n_interp"])
    np.testing.assert_array_equal(og0(x).numpy(), static)                  # p - 0 = p: exactly
    const = np.float32([0.0625, -0.125, 0.03125][:dim])                    # (dyadic: centre + shift is exact in fp32 for none of the centres - hence the bound)
    ogc, _, _ = mr.oracle(mr.dataset(name, track=np.tile(const, (c["H"], 1))), n_interp=c["n_interp"])
    shifted = _static_oracle(name, const)(x).numpy()
    got = ogc(x).numpy()
    print(f"{name}: constant track against shifted centres, max|diff| = {np.abs(got - shifted).max():.3e}")
    # fp64 rounding of (p - o) - c against p - (c + o) with c + o rounded to fp32 first: 6e-8 in the position, through a unit gradient times w = 1e-2
    np.testing.assert_allclose(got, shifted, rtol=0, atol=1e-8)
    assert np.abs(got - static).max() > 1e-6                                # the shift does matter on these trajectories


@pytest.mark.parametrize("name", list(mr.CASES))
def test_wrong_interpolation_is_detected_on_the_case_inputs(name):
    """the mutant offsets by the NEAREST support's row instead of interpolating: the yardstick of the GPU test rejects it on the case's own inputs
    (interpolation off: the points are the supports and the mutant is the reference - nothing to detect, asserted equal)"""
    c = mr.case(name)
    cs = mr.CASES[name]
    ref = c["og"](c["x"].double()).numpy()
    ogm, _, _ = mr.oracle(c["ds"], n_interp=cs["n_interp"], nearest=True, grid_field=c["comp"].cost_l[c["k_grid"]].field if cs["grid"] else None)
    mut = ogm(c["x"].double()).numpy()
    if cs["n_interp"] is None:
        np.testing.assert_array_equal(mut, ref)
        return
    assert gr.rejected(mut, ref, c["amb"], mr.WEIGHTS[0]), name
    assert not gr.rejected(ref, ref, c["amb"], mr.WEIGHTS[0])


@pytest.mark.parametrize("name", list(mr.CASES))
def test_gpu_case_conditions_from_the_reference_alone(name):
    """the caps are conditions, not measurements: the share of ambiguous support waypoints (decided on the shifted points, DELTA = 1e-5) stays within
    the cap of the case, the trajectories reach active hinges of the moving field, and max|x| is not within 1e-3 of the normaliser's range test"""
    c = mr.case(name)
    share, amax = float(c["amb"].mean()), float(c["x"].abs().max())
    print(f"{name}: B = {c['x'].shape[0]}, ambiguous share {100 * share:.2f} % (cap {100 * mr.cap_of(name):.0f} %), active moving-field hinges on "
          f"{c['hinges']} of {c['xi'].shape[0] * c['xi'].shape[1]} points, max|x| = {amax:.4f}")
    assert c["x"].shape[0] == mr.B == 4
    assert share <= mr.cap_of(name)
    assert c["hinges"] > 0
    assert abs(amax - 1.0) > 1e-3


@pytest.mark.parametrize("name,n_check", [("pm2-H64", 64), ("pm2-H64", 256), ("panda-H64", 64), ("panda-H64", 256)] +
                         [(n, k) for n in ("pm2-H64-grid", "panda-H64-grid", "pm3-H24-grid") for k in (64, 256)])
def test_metrics_case_conditions(name, n_check):
    """the metrics comparison presupposes decided points of both kinds, few points in the 1e-5 band, and points that the moving field ALONE decides"""
    from oracle.guide import interpolate_points_v1
    c = mr.case(name)
    xu = c["og"].normalizer.unnormalize(c["x"].double()).float()
    xi = interpolate_points_v1(xu.double(), n_check)
    hit, band = mr.metrics_reference(c["comp"], xi)
    grid = c["comp"].cost_l[c["k_grid"]].field if mr.CASES[name]["grid"] else None
    ogs, comps, _ = mr.oracle(mr.dataset(name, track=None), n_interp=128, grid_field=grid)
    hit_static, _ = mr.metrics_reference(comps, xi)
    print(f"{name} n_check {n_check}: {int(hit.sum())} of {hit.size} collide, {int(band.sum())} in the band, {int((hit != hit_static).sum())} differ from the static set")
    assert band.mean() <= 0.01 and (hit & ~band).any() and (~hit & ~band).any()
    assert (hit != hit_static)[~band].any()


def test_crossing_expectations():
    """the hand-built crossing of tests/test_gpu_moving.py, from the reference alone: static the sphere leaves the line free; on its track it is met at
    mid-time; parked on the line it blocks it; on a track that leaves first nothing is hit.  No flag within 1e-5 of its margin."""
    from oracle.guide import interpolate_points_v1
    flags = {}
    for kind in ("static", "crossing", "parked", "leaving"):
        ds = mr.crossing_dataset(kind)
        x = mr.crossing_traj(ds)
        og, comp, _ = mr.oracle(ds)
        xu = og.normalizer.unnormalize(x.double()).float()
        hit, band = mr.metrics_reference(comp, interpolate_points_v1(xu.double(), 256))
        assert not band.any(), kind
        flags[kind] = hit[0]
    assert not flags["static"].any() and not flags["leaving"].any()
    assert flags["parked"].any() and flags["crossing"].any()
    idx = np.nonzero(flags["crossing"])[0]
    assert idx.min() > 64 and idx.max() < 192 and (np.diff(idx) == 1).all()      # one contiguous run around mid-time
