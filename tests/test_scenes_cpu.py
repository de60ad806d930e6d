"""CPU checks of the scene batches (several obstacle scenes in one launch, include/mpdx.h): the blocked primitive table, the ABI struct against the C
header, the launchers' refusals through the C ABI (no launch), PlanningScenes' host-side validation, the slicing of plan_contexts, and the oracle's own
fp32-against-fp64 error on the inputs of the GPU oracle cases (tests/test_gpu_scenes.py)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import obstacle_hugging_trajs, product_guide
from scene_ref import N_PER_CONTEXT, SCENE_OF_CONTEXT, mismatch_fraction, oracle_increment, scene_object_sets

ROOT = Path(__file__).resolve().parent.parent


def _scenes(env_id="EnvDense2D", robot_id="RobotPointMass", fixed=False, **task_kw):
    import mpd_public_amd as m
    ds = m.TrajectoryDataset(env_id, robot_id)
    if task_kw:
        ds.task = m.PlanningTask(ds.env, ds.robot, obstacle_cutoff_margin=ds.task.obstacle_cutoff_margin, **task_kw)
    sets = scene_object_sets(ds.env.dim)
    fixed_sets = None
    if fixed:   # scene s keeps the first 4 + 3 s fixed spheres of the environment
        o = ds.env.obj_fixed
        fixed_sets = [m.ObjectSet(o.sphere_centers[:4 + 3 * s], o.sphere_radii[:4 + 3 * s], o.box_centers[:s], o.box_half[:s]) for s in range(3)]
    return ds, m.PlanningScenes(ds.task, sets, fixed_objects=fixed_sets), sets, fixed_sets


def _table_of(gp):
    return np.asarray(gp.table_host), np.asarray(gp.table_host).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- table packing
@pytest.mark.parametrize("env_id,robot_id", [("EnvDense2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")])
def test_scene_table_packing(env_id, robot_id):
    """Scenes A (nothing), B (3 spheres), C (5 spheres + 2 boxes): per-scene header counts, the same offsets in every block, capacity = the maximum,
    stride a multiple of 4, unused capacity zero; the fixed field's table once, in the shared tail."""
    from mpd_public_amd import _lib
    ds, scenes, sets, _ = _scenes(env_id, robot_id)
    gp = scenes._params("cpu")
    tab, hdr = _table_of(gp)
    kinds = [gp.fields[i].kind for i in range(gp.n_fields)]
    fx, ex = kinds.index(_lib.FIELD_OBJECTS), len(kinds) - 1     # get_collision_fields(): [self,] objects, workspace, extra objects
    assert kinds[ex] == _lib.FIELD_OBJECTS and fx != ex
    S, stride = gp.n_scenes, gp.scene_stride
    assert S == 3 and stride % 4 == 0 and stride >= _lib.SCENE_HEADER_WORDS + 4 * 5 + 6 * 2
    f = gp.fields[ex]
    assert (f.n_spheres, f.n_boxes) == (5, 2)                                  # capacity = the largest scene
    assert f.sphere_off == _lib.SCENE_HEADER_WORDS and f.box_off == f.sphere_off + 4 * 5 and f.box_off + 6 * 2 <= stride
    for s, o in enumerate(sets):
        b0 = s * stride
        sp, bx = o.prim_floats()
        assert hdr[b0 + ex] == sp.size // 4 and hdr[b0 + _lib.MAX_FIELDS + ex] == bx.size // 6, s     # the scene's own counts
        assert np.array_equal(tab[b0 + f.sphere_off: b0 + f.sphere_off + sp.size], sp)
        assert np.array_equal(tab[b0 + f.box_off: b0 + f.box_off + bx.size], bx)
        assert not tab[b0 + f.sphere_off + sp.size: b0 + f.box_off].any() and not tab[b0 + f.box_off + bx.size: b0 + stride].any()
    # the fixed field: once, behind the last block (offsets >= stride address the shared tail of the staged image)
    g = gp.fields[fx]
    fsp, fbx = ds.env.obj_fixed.prim_floats()
    assert g.sphere_off == stride and g.box_off == stride + fsp.size and (g.n_spheres, g.n_boxes) == (fsp.size // 4, fbx.size // 6)
    assert gp.n_prim_floats == S * stride + fsp.size + fbx.size
    tail = tab[S * stride: gp.n_prim_floats]
    assert np.array_equal(tail, np.concatenate([fsp, fbx]))
    for s in range(S):   # a shared field's header entry is its capacity in every scene
        assert hdr[s * stride + fx] == g.n_spheres and hdr[s * stride + _lib.MAX_FIELDS + fx] == g.n_boxes
    assert gp.scene_of_ctx is None and gp.scene_n_per_ctx == 0    # bound per call


def test_scene_table_repeats_fixed_field_only_with_fixed_objects():
    from mpd_public_amd import _lib
    ds, scenes, sets, fixed_sets = _scenes(fixed=True)
    gp = scenes._params("cpu")
    tab, hdr = _table_of(gp)
    stride = gp.scene_stride
    fx, ex = 0, 2
    g, f = gp.fields[fx], gp.fields[ex]
    assert (g.n_spheres, g.n_boxes) == (10, 2) and (f.n_spheres, f.n_boxes) == (5, 2)
    assert g.sphere_off < stride and g.box_off < stride and f.sphere_off < stride       # both per scene now
    assert gp.n_prim_floats == 3 * stride                                                 # no shared tail
    spans = sorted([(g.sphere_off, 40), (g.box_off, 12), (f.sphere_off, 20), (f.box_off, 12)])
    assert spans[0][0] == _lib.SCENE_HEADER_WORDS and all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])) and sum(spans[-1]) <= stride
    for s in range(3):
        sp, bx = fixed_sets[s].prim_floats()
        assert hdr[s * stride + fx] == 4 + 3 * s and hdr[s * stride + _lib.MAX_FIELDS + fx] == s
        assert np.array_equal(tab[s * stride + g.sphere_off: s * stride + g.sphere_off + sp.size], sp)
        assert np.array_equal(tab[s * stride + g.box_off: s * stride + g.box_off + bx.size], bx)
    # without fixed_objects the same task stores the fixed table once
    gp1 = _scenes()[1]._params("cpu")
    assert gp1.n_prim_floats > 3 * gp1.scene_stride and gp1.fields[fx].sphere_off == gp1.scene_stride


def test_grid_task_keeps_its_grid_and_varies_the_extras():
    """A task whose fixed field is a signed-distance grid: the grid is shared (global memory), only the extras are blocked."""
    from mpd_public_amd import _lib
    from mpd_public_amd.planning import GridSDF
    ds, _, sets, _ = _scenes()
    import mpd_public_amd as m
    ds.env.grid_fixed = GridSDF(torch.rand(9, 9), [-1.2, -1.2], 0.3)
    task = m.PlanningTask(ds.env, ds.robot)
    scenes = m.PlanningScenes(task, sets)
    gp = scenes._params("cpu")
    assert [gp.fields[i].kind for i in range(gp.n_fields)] == [_lib.FIELD_GRID, _lib.FIELD_WORKSPACE, _lib.FIELD_OBJECTS]
    assert gp.n_scenes == 3 and gp.n_prim_floats == 3 * gp.scene_stride and gp.n_grid_floats >= 81
    with pytest.raises(ValueError, match="grid"):
        m.PlanningScenes(task, sets, fixed_objects=sets)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_scene_members_match_the_c_header(tmp_path):
    from mpd_public_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on this host")
    names = ["n_scenes", "scene_stride", "scene_of_ctx", "scene_n_per_ctx", "n_grid_floats", "grids"]
    src = tmp_path / "scene_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpdx.h"\nint main(void) { printf("%zu", sizeof(mpdx_guide_params));\n'
                   + "".join(f'printf(" %zu", offsetof(mpdx_guide_params, {n}));\n' for n in names)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "scene_sizes"
    subprocess.run([cc, "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_lib.GuideParams)] + [getattr(_lib.GuideParams, n).offset for n in names]
    assert got == want
    # the two scene constants of the header (name without the prefix, as _lib mirrors them)
    import re
    defs = {k: int(v) for k, v in re.findall(r"#define MPDX_(\w+)\s+(\d+)", (ROOT / "include" / "mpdx.h").read_text())}
    assert (defs["SCENE_HEADER_WORDS"], defs["SCENE_MAX_STAGED_FLOATS"]) == (_lib.SCENE_HEADER_WORDS, _lib.SCENE_MAX_STAGED_FLOATS)
    assert _lib.SCENE_HEADER_WORDS == 2 * _lib.MAX_FIELDS
    # appended: every member that existed before keeps its offset (the scene members sit behind n_grid_floats)
    assert _lib.GuideParams.n_scenes.offset > _lib.GuideParams.n_grid_floats.offset


def _lib_or_skip():
    from mpd_public_amd import build, _lib
    try:
        build.build(verbose=False)
        return _lib.load()
    except _lib.LibraryUnavailable as e:   # pragma: no cover
        pytest.skip(f"libmpdx.so does not load on this host: {e}")


def _valid_block():
    """A well-formed two-scene point-mass block over HOST memory (the launchers check it before anything touches the pointers)."""
    from mpd_public_amd import _lib
    gp = _lib.GuideParams()
    gp.robot, gp.q_dim, gp.ws_dim, gp.interpolate, gp.n_interp, gp.n_fields = _lib.ROBOT_POINTMASS, 2, 2, 1, 128, 1
    f = gp.fields[0]
    f.kind, f.weight, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 1.0, 8, 3, 20, 1     # 8 + 12 + 6 = 26 -> stride 28
    keep = [(C.c_float * 64)(), (C.c_int32 * 4)()]
    gp.prims, gp.n_prim_floats = C.addressof(keep[0]), 56
    gp.n_scenes, gp.scene_stride, gp.scene_of_ctx, gp.scene_n_per_ctx = 2, 28, C.addressof(keep[1]), 2
    gp._keep = keep
    return gp


def _refusals():
    from mpd_public_amd import _lib
    out = []

    def case(name, **members):
        gp = _valid_block()
        for k, v in members.items():
            setattr(gp, k, v)
        out.append((name, gp))
    case("null table", scene_of_ctx=None)
    case("n_per_ctx zero", scene_n_per_ctx=0)
    case("n_per_ctx negative", scene_n_per_ctx=-2)
    case("stride not a multiple of 4", scene_stride=26)
    case("stride smaller than header plus tables", scene_stride=24)     # the box table (20 .. 26) straddles the block end
    case("stride smaller than the header", scene_stride=4)
    case("blocks beyond the table", n_prim_floats=55)
    case("blocks far beyond the table", n_scenes=1 << 20)
    gp = _valid_block()      # a block that exceeds the LDS table budget
    gp.scene_stride, gp.n_prim_floats = _lib.SCENE_MAX_STAGED_FLOATS + 4, 2 * (_lib.SCENE_MAX_STAGED_FLOATS + 4)
    out.append(("block over the LDS budget", gp))
    gp = _valid_block()      # ... or whose shared tail pushes the staged image over it
    gp.n_prim_floats = 56 + _lib.SCENE_MAX_STAGED_FLOATS
    out.append(("block + tail over the LDS budget", gp))
    return out


def _call_all(lib, gp):
    """Every entry point that takes scenes, with host buffers: (name, rc, message)."""
    from mpd_public_amd import _lib
    x = (C.c_float * (4 * 64 * 4))()
    out = (C.c_float * (4 * 64 * 4))()
    flag = (C.c_uint32 * 2)()
    ms = C.c_float()
    a = lambda b: C.cast(b, C.c_void_p)
    res = []
    call = lambda name, rc: res.append((name, rc, (lib.mpdx_last_error() or b"").decode()))
    call("mpdx_guide_step", lib.mpdx_guide_step(C.byref(gp), a(x), a(out), None, None, a(flag), None, 2, 4, 64, 4, None))
    call("mpdx_guide_step_scaled", lib.mpdx_guide_step_scaled(C.byref(gp), a(x), a(out), None, None, a(flag), None, 2, 4, 64, 4, 0.5, None))
    call("mpdx_guide_time", lib.mpdx_guide_time(C.byref(gp), a(x), a(out), a(flag), 2, 4, 64, 4, 1, None, C.byref(ms)))
    call("mpdx_traj_metrics", lib.mpdx_traj_metrics(C.byref(gp), a(x), a(out), 64, 4, 64, 4, None))
    call("mpdx_traj_metrics_mask", lib.mpdx_traj_metrics_mask(C.byref(gp), a(x), a(out), None, 64, 4, 64, 4, None))
    cfg = _lib.UnetCfg(4, 64, 32, 3, (C.c_int32 * _lib.MAX_LEVELS)(1, 2, 4), 32)
    hdl = C.c_void_p()
    assert lib.mpdx_unet_create(C.byref(cfg), C.byref(hdl)) == 0
    try:
        coefs = (_lib.StepCoefs * 2)()
        call("mpdx_plan", lib.mpdx_plan(hdl, a(x), a(x), 2, coefs, 0, a(x), None, None, None, None, 4, a(x), C.byref(gp), 1, 3, a(flag), 2, 0, 0, None))
    finally:
        lib.mpdx_unet_destroy(hdl)
    return res


def test_scene_refusals_through_the_c_abi():
    lib = _lib_or_skip()
    for what, gp in _refusals():
        for name, rc, msg in _call_all(lib, gp):
            assert rc == -1 and "scene" in msg, (what, name, rc, msg)


def test_zero_block_and_one_scene_take_the_existing_path():
    """n_scenes = 0 (a zero-initialised tail) and n_scenes = 1 are one scene: the scene members are not even looked at.  Seen without a launch: a
    block whose scene members would all be refused, with a robot id no kernel exists for, gets as far as the robot dispatch (the launchers' last
    check), while the same block with n_scenes = 2 is refused for its scene members first."""
    lib = _lib_or_skip()
    for n_scenes in (0, 1, 2):
        gp = _valid_block()
        gp.robot = 7
        gp.n_scenes, gp.scene_stride, gp.scene_of_ctx, gp.scene_n_per_ctx = n_scenes, 3, None, -1
        for name, rc, msg in _call_all(lib, gp):
            if name in ("mpdx_plan", "mpdx_guide_time"):     # (these reach the robot dispatch only through a launch sequence)
                assert (rc == -1 and "scene" in msg) == (n_scenes == 2), (n_scenes, name, rc, msg)
                continue
            assert rc == -1, (n_scenes, name, rc, msg)
            assert ("scene" in msg) == (n_scenes == 2) and ("unsupported robot" in msg) == (n_scenes != 2), (n_scenes, name, msg)


def test_planners_and_bake_refuse_scenes():
    from mpd_public_amd import _lib
    lib = _lib_or_skip()
    gp = _valid_block()
    gp.use_gp, gp.dt, gp.sigma_gp = 1, 0.1, 1.0
    buf = (C.c_float * 4096)()
    a = lambda b: C.cast(b, C.c_void_p)
    o = _lib.GpmpOpts(1.0, 10.0, 0.1, 1e-6, 1e6, 1.0, 1)
    assert lib.mpdx_gpmp_step(C.byref(gp), C.byref(o), a(buf), a(buf), a(buf), 1, 64, 4, 1, None) == -1
    assert "planners take one scene" in lib.mpdx_last_error().decode()
    r = _lib.RrtOpts()
    r.step, r.max_nodes, r.max_iters, r.max_connect_steps, r.n_edge_checks = 0.1, 64, 16, 4, 4
    assert lib.mpdx_rrt_connect(C.byref(gp), C.byref(r), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), 1, None) == -1
    assert "planners take one scene" in lib.mpdx_last_error().decode()
    assert lib.mpdx_rrt_paths(C.byref(gp), a(buf), a(buf), a(buf), a(buf), a(buf), a(buf), None, 1, 64, 64, 0.1, 4, 1, None) == -1
    assert "planners take one scene" in lib.mpdx_last_error().decode()
    n, org = (C.c_int * 3)(8, 8, 1), (C.c_float * 3)(-1.0, -1.0, 0.0)
    assert lib.mpdx_sdf_grid_bake(C.byref(gp), 0, a(buf), None, C.byref(n), C.byref(org), 0.25, None) == -1
    assert "one scene only" in lib.mpdx_last_error().decode()


def test_gpmp_step_refuses_unsupported_horizons_without_launching():
    """mpdx_gpmp_step's shape limits, each refused on the host (-1) with the offending value in mpdx_last_error: fewer than two free supports,
    fewer interpolated points than supports or more than 8 per support (the support-window arithmetic), and a Panda horizon whose
    block-tridiagonal system does not fit 160 KB of LDS."""
    from mpd_public_amd import _lib
    lib = _lib_or_skip()
    buf = (C.c_float * (128 * 14))()
    a = lambda b: C.cast(b, C.c_void_p)
    o = _lib.GpmpOpts(2e-2, 10.0, 0.2, 1e-7, 1e7, 1.0, 1)

    def block(n_interp, panda=False):
        gp = _valid_block()
        gp.n_scenes, gp.n_interp = 1, n_interp
        gp.use_gp, gp.dt, gp.sigma_gp = 1, 5.0 / 64, 1.0
        if panda:
            gp.robot, gp.q_dim, gp.ws_dim = _lib.ROBOT_PANDA, 7, 3
        return gp
    for gp, H, D, want in ((block(8), 3, 4, "H=3"), (block(23), 24, 4, "n_interp 23 unsupported for H=24"), (block(193), 24, 4, "n_interp 193 unsupported for H=24"),
                           (block(128, panda=True), 80, 14, "LDS (H=80, 128 points)")):
        assert lib.mpdx_gpmp_step(C.byref(gp), C.byref(o), a(buf), a(buf), a(buf), 1, H, D, 1, None) == -1, want
        assert want in lib.mpdx_last_error().decode(), (want, lib.mpdx_last_error().decode())


# ---------------------------------------------------------------------------------------------------------------- PlanningScenes / guide / plan_contexts
def test_planning_scenes_validation():
    import mpd_public_amd as m
    ds, scenes, sets, _ = _scenes()
    z = m.ObjectSet.empty()
    with pytest.raises(ValueError, match="wrong dimension"):      # a 3-D sphere in a 2-D workspace
        m.PlanningScenes(ds.task, [m.ObjectSet(np.array([[0.1, 0.2, 0.3]], np.float32), np.array([0.1], np.float32), z.box_centers, z.box_half)])
    with pytest.raises(ValueError, match=r"\[n, 3\]"):            # rows not padded to 3-D
        m.PlanningScenes(ds.task, [m.ObjectSet(np.zeros((2, 2), np.float32), np.full(2, 0.1, np.float32), z.box_centers, z.box_half)])
    with pytest.raises(ValueError, match="positive"):
        m.PlanningScenes(ds.task, [m.ObjectSet(np.zeros((1, 3), np.float32), np.zeros(1, np.float32), z.box_centers, z.box_half)])
    with pytest.raises(ValueError, match="at least one scene"):
        m.PlanningScenes(ds.task, [])
    with pytest.raises(ValueError, match="fixed object sets"):
        m.PlanningScenes(ds.task, sets, fixed_objects=sets[:2])
    with pytest.raises(ValueError, match="use_extra_objects"):
        m.PlanningScenes(m.PlanningTask(ds.env, ds.robot, use_extra_objects=False), sets)
    big = m.ObjectSet(np.zeros((4000, 3), np.float32), np.full(4000, 0.1, np.float32), z.box_centers, z.box_half)
    with pytest.raises(ValueError, match="stage at most"):
        m.PlanningScenes(ds.task, [big])
    grid_task = m.PlanningTask(ds.env, ds.robot, sdf_grid=dict(cell_size=0.05))
    m.PlanningScenes(grid_task, sets)                             # per-scene extras next to a grid: fine
    with pytest.raises(ValueError, match="grid"):
        m.PlanningScenes(grid_task, sets, fixed_objects=sets)
    # the assignment: range-checked on the host, one entry per context
    assert scenes.check_assignment(torch.tensor(SCENE_OF_CONTEXT), 8, 2) == SCENE_OF_CONTEXT
    for bad, n in (([0, 3, 1, 2], 8), ([0, -1, 1, 2], 8), ([0, 1, 2], 8), ([0, 1, 2, 0, 1], 8), ([0, 1, 2, 0], 9)):
        with pytest.raises(ValueError):
            scenes.check_assignment(bad, n, 2)
    with pytest.raises(ValueError):
        scenes.check_assignment(SCENE_OF_CONTEXT, 8, 0)
    x = torch.zeros(8, 64, 4)
    with pytest.raises(RuntimeError, match="GPU"):                # no CPU fallback
        scenes.trajectory_metrics(x, SCENE_OF_CONTEXT, 2)


def test_guide_with_scenes_binding():
    import mpd_public_amd as m
    from helpers import toy_cost
    ds, scenes, sets, _ = _scenes()
    pg = product_guide(ds)
    g = pg.with_scenes(scenes, SCENE_OF_CONTEXT, N_PER_CONTEXT)
    assert g is not pg and g.cost is pg.cost and g._n_per_context == 2 and pg._scenes is None
    assert (g.clip_grad, g.interpolate_trajectories_for_collision, g.num_interpolated_points_for_collision) == (True, True, 128)
    gp = g.device_params("cpu")
    assert gp.n_scenes == 3 and gp.scene_n_per_ctx == 2 and gp.scene_of_ctx == g._scene_table.data_ptr()
    assert g._scene_table.tolist() == SCENE_OF_CONTEXT and g._scene_table.dtype == torch.int32
    assert pg.device_params("cpu").n_scenes == 0                   # the guide it came from stays a single-scene guide
    g.check_batch(8, 2)
    with pytest.raises(ValueError, match="batch of 6"):
        g.check_batch(6)
    with pytest.raises(ValueError, match="n_per_context"):
        g.check_batch(8, 4)
    with pytest.raises(ValueError):
        pg.with_scenes(scenes, [0, 3], 2)                          # scene 3 of 3
    with pytest.raises(ValueError, match="another task"):
        pg.with_scenes(m.PlanningScenes(m.PlanningTask(ds.env, ds.robot), sets), [0], 2)
    with pytest.raises(NotImplementedError, match="autograd"):    # a foreign (autograd) cost has its obstacles inside the callable
        m.GuideManagerTrajectoriesWithVelocity(ds, toy_cost).with_scenes(scenes, [0], 2)


def test_plan_contexts_slices_the_assignment_per_chunk_and_rank():
    from mpd_public_amd.parallel import plan_contexts
    ds, scenes, _, _ = _scenes()
    pg = product_guide(ds)
    Cn, n = 7, 2
    soc = [2, 0, 2, 1, 1, 0, 2]
    start, goal = torch.zeros(Cn, 4), torch.ones(Cn, 4)
    seen = []

    def planner(hc, B, npc, guide=None, **kw):
        seen.append((B, npc, list(guide._scene_of_context), guide._n_per_context, guide._scenes is scenes))
        return torch.zeros(B, 64, 4)
    got = []
    for rank in range(2):
        seen.clear()
        x, (lo, hi) = plan_contexts(None, start, goal, n, rank=rank, world_size=2, max_batch=4, planner=planner, horizon=64, guide=pg, scenes=scenes,
                                    scene_of_context=soc)
        assert x.shape[0] == (hi - lo) * n
        assert all(s[1] == n and s[3] == n and s[4] and s[0] == len(s[2]) * n for s in seen)
        got.append([v for s in seen for v in s[2]])
        assert max(len(s[2]) for s in seen) <= 2                   # max_batch 4 = two contexts per chunk
    assert got == [soc[:4], soc[4:]]
    assert pg._scenes is None
    passed = []
    plan_contexts(None, start, goal, n, planner=lambda hc, B, npc, guide=None, **kw: passed.append(guide) or torch.zeros(B, 64, 4), horizon=64, guide=pg)
    assert passed == [pg]                                          # scenes=None: the guide passes through as it is
    with pytest.raises(ValueError):
        plan_contexts(None, start, goal, n, planner=planner, horizon=64, guide=pg, scenes=scenes, scene_of_context=soc[:-1])
    with pytest.raises(ValueError):
        plan_contexts(None, start, goal, n, planner=planner, horizon=64, guide=pg, scenes=scenes)
    with pytest.raises(ValueError):
        plan_contexts(None, start, goal, n, planner=planner, horizon=64, scenes=scenes, scene_of_context=soc)
    with pytest.raises(ValueError):
        plan_contexts(None, start, goal, n, planner=planner, horizon=64, guide=pg, scene_of_context=soc)


# ---------------------------------------------------------------------------------------------------------------- the oracle on the GPU cases' inputs
@pytest.mark.parametrize("env_id,robot_id", [("EnvDense2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPanda")])
def test_oracle_fp32_stays_inside_the_guide_tolerance_on_the_scene_inputs(env_id, robot_id):
    """The GPU oracle cases (tests/test_gpu_scenes.py) hold the kernel to 1e-3 rel / 2e-6 abs on >= 99 % of the waypoints against fp64 autograd.
    That cap must leave room for fp32 itself: the fp32 oracle against the fp64 oracle on the same inputs, scene by scene, stays inside it."""
    ds, scenes, _, _ = _scenes(env_id, robot_id)
    x = obstacle_hugging_trajs(ds, len(SCENE_OF_CONTEXT) * N_PER_CONTEXT, seed=f"scenes/{env_id}")
    r64 = oracle_increment(ds, scenes, SCENE_OF_CONTEXT, N_PER_CONTEXT, x, torch.float64)
    r32 = oracle_increment(ds, scenes, SCENE_OF_CONTEXT, N_PER_CONTEXT, x, torch.float32)
    frac, bad = mismatch_fraction(r32.numpy(), r64.numpy())
    print(f"fp32 oracle vs fp64 oracle: {bad.sum()} of {bad.size} waypoints outside 1e-3 rel / 2e-6 abs ({100 * frac:.2f} %)")
    assert r64.abs().max() > 0 and frac < 0.01
    # the scenes matter on these inputs: evaluating everything against scene A gives another increment
    rA = oracle_increment(ds, scenes, [0] * len(SCENE_OF_CONTEXT), N_PER_CONTEXT, x, torch.float64)
    assert mismatch_fraction(rA.numpy(), r64.numpy())[0] > 0.01
