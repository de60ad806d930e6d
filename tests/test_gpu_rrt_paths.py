"""rrt_path_kernel (mpdx_rrt_paths: path extraction + greedy shortcutting + arc-length resampling in one launch) against its float64 restatement
tests/paths_ref.py, on HAND-BUILT trees of a handful of nodes: which nodes, in which order; the 1024-node cap and its straight-line fallback;
the supports and velocities at H = 2 ... 1024 within the bound derived in paths_ref (a few float32 roundings of the arc length, not a chosen
number); the shortcut decisions on paths whose every examined edge clears the obstacle margin by 1e-3 (established on the CPU in
tests/test_paths_ref_cpu.py, so none may be cut short here); the Panda's sphere and pair split at 12 / 8 / 2 / 1 parts.  Each launch holds 5 - 8
problems with DIFFERENT trees; the output buffers carry a sentinel-filled guard behind the last problem.

Last: the full pipeline at its defaults on the trees of the search's reference, and the host restatements RRTConnectBatch.paths / shortcut_path."""
import ctypes as C

import numpy as np
import pytest
import torch

import paths_ref as pr
import rrt_ref
from helpers import paths_case, rrt_problem, single_thread

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, -12345.0
_DS = {}


def _gpu_dataset(cpu_ds):
    import mpd_public_amd as m
    key = (cpu_ds.env.name, "RobotPointMass3D" if (cpu_ds.robot.name, cpu_ds.robot.q_dim) == ("RobotPointMass", 3) else cpu_ds.robot.name)
    if key not in _DS:
        _DS[key] = m.TrajectoryDataset(*key, tensor_args={"device": "cuda", "dtype": torch.float32})
    return _DS[key]


def _launch(ds, p, with_len=True):
    """one mpdx_rrt_paths launch on the problem's trees -> (trajs [n, H, 2q], path_len [n] or None) as numpy; the guards are checked here"""
    from mpd_public_amd import _lib
    n, H, q, M = p.n, p.H, p.start.shape[1], p.max_nodes
    assert p.nodes.shape == (n, 2, M, q) and p.parent.shape == (n, 2, M) and p.link.shape == (n, 2)
    assert int(p.parent.max()) < M and int(p.link.max()) < M and int(p.parent.min()) >= -1, "indices the kernel follows stay inside the trees"
    f = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda")     # noqa: E731
    i = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.int32, device="cuda")       # noqa: E731
    start, goal, nodes, parent, link = f(p.start), f(p.goal), f(p.nodes), i(p.parent), i(p.link)
    out = torch.full((n * H * 2 * q + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out[n * H * 2 * q:] = SENTINEL
    plen = torch.full((n + GUARD,), -77, dtype=torch.int32, device="cuda")
    gp = ds.task._params(torch.device("cuda"))
    _lib.check(_lib.load().mpdx_rrt_paths(C.byref(gp), start.data_ptr(), goal.data_ptr(), nodes.data_ptr(), parent.data_ptr(), link.data_ptr(),
                                          out.data_ptr(), plen.data_ptr() if with_len else None, n, M, H, float(np.float32(p.dt)), int(p.n_edge_checks),
                                          int(p.rounds), _lib.current_stream()), "mpdx_rrt_paths")
    torch.cuda.synchronize()
    out, plen = out.cpu(), plen.cpu()
    assert bool((out[n * H * 2 * q:] == SENTINEL).all()), "trajs_out was written behind its last problem"
    assert bool((plen[n:] == -77).all()) and (with_len or bool((plen == -77).all())), "path_len was written behind its last problem"
    return out[: n * H * 2 * q].reshape(n, H, 2 * q).numpy(), (plen[:n].numpy() if with_len else None)


def _judge(name, p, trajs, plen):
    with single_thread():
        rep = pr.compare(trajs, plen, p)
    print(f"PATHS_EDGES {name}: {p.n} problems, path_len {None if plen is None else plen.tolist()}, {rep.edge_checks} edge decisions verified, "
          f"{len(rep.cut_short)} cut short, worst error / bound: positions {rep.pos_frac:.3f}, velocities {rep.vel_frac:.3f}")
    assert rep.mismatches == [], rep.mismatches
    return rep


# path_len the cases are built for (None: judged by compare() alone)
EXPECTED_LEN = {"extract": [2, 11, 11, 14, 2, 2, 3, 2], "path_cap": [1024, 2, 1024, 2, 2, 1024],
                **{f"shortcut_c{c}_r{r}": [2, 4, 4, 3, 4, 2] for c in (24, 32, 256) for r in (1, 3)}, "shortcut_c2_r3": [2] * 6,
                **{f"panda_c{c}": [5, 5, 5, 4, 2, 3] for c in (16, 32, 100, 200)}}


@pytest.mark.parametrize("name", list(pr.CASES))
def test_rrt_path_kernel_equals_its_float64_restatement(name):
    cpu_ds, p = paths_case(name)
    ds = _gpu_dataset(cpu_ds)
    trajs, plen = _launch(ds, p)
    rep = _judge(name, p, trajs, plen)
    assert rep.cut_short == [] and rep.compared == p.n, "hand-built cases: no edge is ambiguous (tests/test_paths_ref_cpu.py)"
    if name in EXPECTED_LEN:
        assert plen.tolist() == EXPECTED_LEN[name]
    if name.startswith("resample_"):
        q = p.start.shape[1]
        assert plen.tolist() == [len(v) for v in pr._resample_paths(q, p.H, 1.0 if q < 7 else 2.0)], "rounds = 0: every node stays"
        assert np.array_equal(trajs[3, :, : p.start.shape[1]], np.tile(p.start[3].astype(np.float32), (p.H, 1))) and not trajs[3, :, p.start.shape[1]:].any()
    if name == "path_cap":      # the 1024-node chains are resampled as arcs, the 1025-node chains as their chords
        q = 2
        for b, m in enumerate(plen.tolist()):
            mid = 0.5 * (p.start[b] + p.goal[b])
            off = float(np.linalg.norm(trajs[b, :, :q].astype(np.float64) - mid, axis=-1).min())
            assert (off > 0.3) == (m == 1024) and (off < 0.05) == (m == 2), (b, m, off)
    if name in ("extract", "shortcut_c24_r3", "resample_q7_H64"):      # path_len = NULL: the same trajectories, bit for bit
        again, none = _launch(ds, p, with_len=False)
        assert none is None and np.array_equal(again, trajs)


def test_more_rounds_change_nothing_after_the_first():
    """`rounds` 1 and 3 give the same output on every shortcut case: one round of "jump to the last visible node" leaves a fixed point
    (paths_ref's docstring has the argument; tests/test_paths_ref_cpu.py checks it on random visibility tables)"""
    for c in (24, 256):
        cpu_ds, p1 = paths_case(f"shortcut_c{c}_r1")
        _, p3 = paths_case(f"shortcut_c{c}_r3")
        ds = _gpu_dataset(cpu_ds)
        (t1, l1), (t3, l3) = _launch(ds, p1), _launch(ds, p3)
        assert np.array_equal(t1, t3) and np.array_equal(l1, l3)
    cpu_ds, p0 = paths_case("shortcut_c24_r3")
    p0.rounds = 0
    t0, l0 = _launch(_gpu_dataset(cpu_ds), p0)
    assert l0.tolist() == [len(v) for v in pr.NARROW_PATHS[:5]] + [2]
    _judge("shortcut_c24_r0", p0, t0, l0)


@pytest.fixture(scope="module")
def search():
    """the trees of the search's reference on rrt_ref.CASES["dense"] (float64 search on the CPU, cast to float32)"""
    import mpd_public_amd as m
    case = rrt_ref.CASES["dense"]
    cpu_ds = m.TrajectoryDataset(case["env"], case["robot"], tensor_args={"device": "cpu", "dtype": torch.float32})
    rp = rrt_problem(cpu_ds, case)
    with single_thread():
        trees = rrt_ref.free_run(rp)
    return cpu_ds, case, trees, pr.case_search(trees, rp)


def test_full_pipeline_on_the_trees_of_the_search_reference(search):
    cpu_ds, case, trees, p = search
    trajs, plen = _launch(_gpu_dataset(cpu_ds), p)
    rep = _judge("search_dense", p, trajs, plen)
    assert 8 * len(rep.cut_short) <= p.n, f"problems cut short at an ambiguous edge: {rep.cut_short}"
    assert rep.edge_checks > 100 and max(rep.path_len) > 2


def test_host_restatements_equal_the_reference_on_the_same_trees(search):
    from mpd_public_amd.generate_trajectories import RRTConnectBatch, shortcut_path
    cpu_ds, case, trees, p = search
    ds = _gpu_dataset(cpu_ds)
    n = p.n
    rrt = RRTConnectBatch(ds.task, torch.tensor(case["start"], device="cuda"), torch.tensor(case["goal"], device="cuda"), n, step_size=case["step"],
                          max_nodes=case["max_nodes"], n_edge_checks=case["n_edge_checks"])
    rrt.nodes.copy_(torch.tensor(trees.nodes))
    rrt.parent.copy_(torch.tensor(trees.parent))
    rrt.link.copy_(torch.tensor(trees.link))
    rrt.done = rrt.link[:, 0] >= 0
    paths = rrt.paths()
    compared = 0
    for b in range(n):
        if int(trees.link[b, 0]) < 0:
            assert paths[b] is None
            continue
        ref = pr.extract(p.nodes[b], p.parent[b], p.link[b], p.start[b], p.goal[b])
        assert np.array_equal(paths[b].numpy().astype(np.float64), ref), b
        try:
            with single_thread():
                sc = pr.shortcut(ref, p.slack_fn, 32, 3)
        except pr.Ambiguous:
            continue
        got = shortcut_path(ds.task, paths[b], 32, 3).numpy().astype(np.float64)
        assert np.array_equal(got, sc), (b, len(got), len(sc))
        compared += 1
    assert 8 * (int((trees.link[:, 0] >= 0).sum()) - compared) <= n and compared >= n // 2
    # the object's own launch (RRTConnectBatch.trajectories) is the launch judged above
    tr, plen = rrt.trajectories(p.H, p.dt, return_path_len=True)
    with single_thread():
        rep = pr.compare(tr.cpu().numpy(), plen.cpu().numpy(), p)
    assert rep.mismatches == [] and 8 * len(rep.cut_short) <= n
