"""tests/paths_ref.py checked without a GPU: the three steps on hand-computable inputs, compare() REPORTS each of the deliberately wrong pipelines
(paths_ref.FAULTS) on the cases tests/test_gpu_rrt_paths.py runs on the device, those cases have the properties they are there for (no edge
within 1e-3 of the obstacle margin), generate_trajectories.resample_path is held to the same bound, and mpdx_rrt_paths refuses bad arguments on
the host, before any launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import paths_ref as pr
import rrt_ref
from helpers import paths_case, rrt_problem, single_thread, oracle_deciding_hinge, oracle_collision_terms

_CACHE = {}


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = paths_case(name)[1]
    return _CACHE[name]


def _search_case():
    if "search" not in _CACHE:
        import mpd_public_amd as m
        case = rrt_ref.CASES["dense"]
        ds = m.TrajectoryDataset(case["env"], case["robot"], tensor_args={"device": "cpu", "dtype": torch.float32})
        rp = rrt_problem(ds, case)
        with single_thread():
            _CACHE["search"] = pr.case_search(rrt_ref.free_run(rp), rp)
    return _CACHE["search"]


def _run(p, fault=None):
    with single_thread():
        return pr.run(p, fault)


def _compare(trajs, plen, p):
    with single_thread():
        return pr.compare(trajs, plen, p)


# ------------------------------------------------------------------------------------------------------------------- hand-computable inputs
P345 = np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 4.0]])


def test_resample_of_a_3_4_5_polyline():
    tr = pr.resample(P345, 8, 0.5)                     # total length 7: u_h = h
    assert np.allclose(tr[:, :2], [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [3, 2], [3, 3], [3, 4]], rtol=0, atol=1e-15)
    assert np.array_equal(tr[3, :2], [3.0, 0.0]), "the support that lands on the corner IS the corner"
    vel = np.array([[0, 0], [2, 0], [2, 0], [1, 1], [0, 2], [0, 2], [0, 2], [0, 0]], dtype=float)     # (x[h + 1] - x[h - 1]) / (2 * 0.5)
    assert np.allclose(tr[:, 2:], vel, rtol=0, atol=1e-14)
    tr2 = pr.resample(P345, 2, 0.1)
    assert np.array_equal(tr2, [[0, 0, 0, 0], [3, 4, 0, 0]])
    tr3 = pr.resample(P345, 3, 0.25)                   # u = 3.5: half a unit up the second segment
    assert np.allclose(tr3, [[0, 0, 0, 0], [3, 0.5, 6, 8], [3, 4, 0, 0]], rtol=0, atol=1e-14)


def test_resample_ignores_a_duplicated_node():
    dup = P345[[0, 1, 1, 1, 2]]
    assert np.allclose(pr.resample(dup, 8, 0.5), pr.resample(P345, 8, 0.5), rtol=0, atol=1e-15)
    assert np.allclose(pr.resample(P345[[0, 0, 1, 2, 2]], 8, 0.5), pr.resample(P345, 8, 0.5), rtol=0, atol=1e-15)


def test_resample_of_start_equal_goal_is_finite():
    s = np.array([0.3, -0.7, 1.1])
    for H in (2, 3, 64):
        tr = pr.resample(np.stack([s, s]), H, 1e-3)
        assert np.isfinite(tr).all() and np.array_equal(tr[:, :3], np.tile(s, (H, 1))) and not tr[:, 3:].any()


def _toy_trees():
    # tree 0: 0 (start) <- 2 <- 3, decoys 1, 4;   tree 1: 0 (goal) <- 1 <- 4, decoys 2, 3
    nodes = np.arange(2 * 5 * 2, dtype=float).reshape(2, 5, 2)
    parent = np.array([[-1, 0, 0, 2, 1], [-1, 0, 1, 2, 1]])
    return nodes, parent


def test_extract_orders_the_two_branches():
    nodes, parent = _toy_trees()
    start, goal = nodes[0, 0], nodes[1, 0]
    path = pr.extract(nodes, parent, (3, 4), start, goal)
    assert np.array_equal(path, np.stack([nodes[0, 0], nodes[0, 2], nodes[0, 3], nodes[1, 4], nodes[1, 1], nodes[1, 0]]))
    assert np.array_equal(pr.extract(nodes, parent, (0, 0), start, goal), np.stack([start, goal]))
    line = np.stack([start + 100, goal + 100])       # the fallback takes start / goal, not the roots
    for link in ((-1, -1), (3, -1), (-1, 4), (-2, 4)):
        assert np.array_equal(pr.extract(nodes, parent, link, start + 100, goal + 100), line)
    assert len(pr.extract(nodes, parent, (3, 4), start, goal, max_path=6)) == 6
    assert np.array_equal(pr.extract(nodes, parent, (3, 4), start + 100, goal + 100, max_path=5), line)
    assert len(pr.extract(nodes, parent, (3, 0), start, goal, max_path=4)) == 4
    assert np.array_equal(pr.extract(nodes, parent, (3, 4), start, goal, max_path=2), np.stack([start, goal]))


def _pair_slack(vis):
    """edges between the nodes [i] of a path on a line, judged by a table: 2 checks hand the function the two end points"""
    return lambda q: np.full(len(q), -1.0 if vis[int(q[0, 0]), int(q[-1, 0])] else 1.0)


def test_shortcut_jumps_to_the_last_visible_node():
    path = np.arange(6, dtype=float)[:, None]
    vis = np.zeros((6, 6), dtype=bool)
    vis[0, 2] = vis[0, 4] = vis[4, 5] = vis[2, 5] = True
    log = []
    assert pr.shortcut(path, _pair_slack(vis), 2, 3, log=log)[:, 0].tolist() == [0, 4, 5]
    assert [(i, j) for i, j, _ in log[:2]] == [(0, 5), (0, 4)]
    assert pr.shortcut(path, _pair_slack(vis), 2, 1, fault="first_visible")[:, 0].tolist() == [0, 2, 5]
    assert pr.shortcut(path, _pair_slack(vis), 2, 0)[:, 0].tolist() == list(range(6))
    assert pr.shortcut(path, _pair_slack(np.zeros((6, 6), dtype=bool)), 2, 3)[:, 0].tolist() == list(range(6))     # sees nothing: the next node
    assert pr.shortcut(path, _pair_slack(np.ones((6, 6), dtype=bool)), 2, 3)[:, 0].tolist() == [0, 5]
    with pytest.raises(pr.Ambiguous):
        pr.shortcut(path, lambda q: np.full(len(q), 0.5 * pr.EDGE_EPS), 2, 1)


def test_edge_checks_include_both_end_points():
    seen = []
    pr.edge_slack(np.array([0.0]), np.array([1.0]), lambda q: (seen.append(q[:, 0].copy()), np.zeros(len(q)))[1], 5)
    assert np.array_equal(seen[0], [0.0, 0.25, 0.5, 0.75, 1.0])


def test_one_round_of_last_visible_leaves_a_fixed_point():
    """why `one_round` is in EQUIVALENT_FAULTS: on 300 random visibility tables the second round removes nothing (the argument is in
    paths_ref's docstring) - while the rule `first_visible` does need its rounds"""
    rng = np.random.default_rng(0)
    differs = 0
    for _ in range(300):
        m = int(rng.integers(3, 14))
        vis = rng.uniform(size=(m, m)) < rng.uniform(0.1, 0.9)
        path = np.arange(m, dtype=float)[:, None]
        one = pr.shortcut(path, _pair_slack(vis), 2, 1)
        vis2 = vis[np.ix_(one[:, 0].astype(int), one[:, 0].astype(int))]
        again = pr.shortcut(np.arange(len(one), dtype=float)[:, None], _pair_slack(vis2), 2, 1)
        assert len(again) == len(one)
        f1 = pr.shortcut(path, _pair_slack(vis), 2, 1, fault="first_visible")
        v1 = vis[np.ix_(f1[:, 0].astype(int), f1[:, 0].astype(int))]
        differs += len(pr.shortcut(np.arange(len(f1), dtype=float)[:, None], _pair_slack(v1), 2, 1, fault="first_visible")) < len(f1)
    assert differs > 30


# ------------------------------------------------------------------------------------------------------------------- compare() and the faults
@pytest.mark.parametrize("name", list(pr.CASES))
def test_compare_accepts_the_reference_itself(name):
    p = _case(name)
    trajs, plen = _run(p)
    rep = _compare(trajs, plen, p)
    assert rep.mismatches == [] and rep.cut_short == [] and rep.compared == p.n
    assert rep.pos_frac < 0.5 and rep.vel_frac < 0.5, "the float32 cast of the reference lies well inside the bound"
    assert _compare(trajs, None, p).mismatches == []


# (fault, case): a case of the GPU test on which the fault changes the output
MUTANTS = [("first_visible", "shortcut_c24_r3"), ("first_visible", "shortcut_c24_r1"), ("w_over_n", "shortcut_c2_r3"),
           ("searchsorted_left_unclamped", "resample_q2_H64_dt0"), ("searchsorted_left_unclamped", "resample_q7_H3"),
           ("forward_difference", "resample_q2_H3_dt1"), ("forward_difference", "resample_q7_H1024_lds"),
           ("end_velocity_nonzero", "resample_q2_H2_dt0"), ("end_velocity_nonzero", "resample_q3_H64"),
           ("tree1_reversed", "extract"), ("tree1_reversed", "path_cap"), ("link_node_twice", "extract"), ("link_node_twice", "path_cap"),
           ("ends_interpolated", "resample_q2_H64_dt0")]


@pytest.mark.parametrize("fault,name", MUTANTS)
def test_compare_reports_a_wrong_pipeline(fault, name):
    assert fault in pr.FAULTS
    p = _case(name)
    rep = _compare(*_run(p, fault), p)
    print(fault, name, rep.mismatches)
    assert rep.mismatches and rep.cut_short == []


def test_every_fault_has_a_mutant_and_the_equivalent_one_has_none():
    assert sorted({m[0] for m in MUTANTS}) == sorted(pr.FAULTS)
    assert sorted(pr.FAULTS + pr.EQUIVALENT_FAULTS) == sorted(["first_visible", "one_round", "w_over_n", "searchsorted_left_unclamped", "forward_difference",
                                                              "end_velocity_nonzero", "tree1_reversed", "link_node_twice", "ends_interpolated"])
    for name in pr.HAND_BUILT_SHORTCUT:      # `one_round`: the same output, bit for bit, on every case that shortcuts
        p = _case(name)
        a, b = _run(p), _run(p, "one_round")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


def test_link_node_twice_shows_in_path_len_only():
    """a duplicated node adds a segment of length zero: the trajectories stay, so compare() must look at path_len"""
    p = _case("extract")
    trajs, plen = _run(p, "link_node_twice")
    assert _compare(trajs, None, p).mismatches == [] and len(_compare(trajs, plen, p).mismatches) >= 4


# ------------------------------------------------------------------------------------------------------------------- conditions on the cases
@pytest.mark.parametrize("name", pr.HAND_BUILT_SHORTCUT)
def test_hand_built_edges_are_clear_of_the_margin(name):
    p = _case(name)
    worst, edges = math.inf, 0
    with single_thread():
        for b in range(p.n):
            log = []
            pr.solve(p, b, None, log)
            edges += len(log)
            worst = min([worst] + [abs(s) for _, _, s in log])
    assert edges > 0 and worst >= 1e-3, (name, worst)


def test_shortcut_cases_have_the_properties_they_are_there_for():
    def lens(name, fault=None):
        return _run(_case(name), fault)[1].tolist()
    full = [len(v) for v in pr.NARROW_PATHS]
    assert lens("shortcut_c24_r3") == [2, 4, 4, 3, 4, 2] == lens("shortcut_c24_r1") == lens("shortcut_c256_r3") == lens("shortcut_c32_r3")
    assert full[1] == full[2] == 4, "paths 1 and 2: nothing can be removed"
    assert lens("shortcut_c24_r1", "first_visible")[3] == 4, "path 3: first visible and last visible differ within one round"
    assert lens("shortcut_c24_r3", "first_visible")[0] == 3, "path 0: first visible has not converged after three rounds"
    assert lens("shortcut_c2_r3") == [2] * 6, "two checks see the end points only: the chord through the wall is accepted"
    p = _case("shortcut_c24_r3")
    assert float(p.slack_fn(0.5 * (p.start[1] + p.goal[1])[None])[0]) > 0.03, "... and it does cross the wall"
    for c in (16, 32, 100, 200):
        assert lens(f"panda_c{c}") == [5, 5, 5, 4, 2, 3], c
    p = _case("panda_c32")
    assert pr.edge_slack(p.start[0], p.goal[0], p.slack_fn, 32) > 0.1, "the straight line start -> goal collides"


def test_panda_edges_are_decided_by_link_spheres_of_several_parts_and_by_a_self_collision_pair():
    ds, p = paths_case("panda_c32")
    terms = oracle_collision_terms(ds)
    kinds = set()
    with single_thread():
        for b in (0, 5):
            path = pr.extract(p.nodes[b], p.parent[b], p.link[b], p.start[b], p.goal[b])
            log = []
            pr.shortcut(path, p.slack_fn, 32, 1, log=log)
            w = (np.arange(32) / 31)[:, None]
            for i, j, s in log:
                v, kind, idx = oracle_deciding_hinge(ds, (1 - w) * path[i] + w * path[j], terms)
                assert abs(v - s) < 1e-12
                kinds.add((kind, idx))
    print(sorted(kinds))
    assert ("self", 0) in kinds and len({idx % 8 for kind, idx in kinds if kind == "objects"}) >= 3


def test_search_trees_cut_short_at_most_one_problem_in_eight():
    p = _search_case()
    trajs, plen = _run(p)
    rep = _compare(trajs, plen, p)
    assert rep.mismatches == [] and 8 * len(rep.cut_short) <= p.n, rep.cut_short
    assert int((p.link[:, 0] >= 0).sum()) >= p.n // 2 and rep.edge_checks > 100 and max(rep.path_len) > 2


# ------------------------------------------------------------------------------------------------------------------- the host restatement
@pytest.mark.parametrize("name", [k for k in pr.CASES if k.startswith("resample_")] + ["path_cap", "shortcut_c24_r3"])
def test_host_resample_path_is_within_the_bound(name):
    from mpd_public_amd.generate_trajectories import resample_path
    p = _case(name)
    q = p.start.shape[1]
    worst = [0.0, 0.0]
    for b in range(p.n):
        path, ref = pr.solve(p, b)
        got = resample_path(torch.tensor(path, dtype=torch.float32), p.H, p.dt).numpy().astype(np.float64)
        pos_tol, vel_tol = pr.tolerances(path, ref, p.dt)
        assert np.isfinite(got).all(), (name, b)
        assert np.array_equal(got[0, :q], path[0]) and np.array_equal(got[-1, :q], path[-1]) and not got[0, q:].any() and not got[-1, q:].any()
        pe, ve = np.abs(got[:, :q] - ref[:, :q]).max(), (np.abs(got[:, q:] - ref[:, q:]) / np.where(vel_tol > 0, vel_tol, 1.0)).max()
        if pos_tol == 0:
            assert pe == 0 and not got[:, q:].any()
            continue
        worst = [max(worst[0], pe / pos_tol), max(worst[1], ve)]
        assert pe <= pos_tol and ve <= 1.0, (name, b, pe / pos_tol, ve)
    print(name, "worst fraction of the bound: positions %.3f, velocities %.3f" % tuple(worst))


# ------------------------------------------------------------------------------------------------------------------- refusals, on the host
@pytest.fixture(scope="module")
def lib():
    from mpd_public_amd import build, _lib
    try:
        build.build(verbose=False)
        return _lib.load()
    except _lib.LibraryUnavailable as e:   # pragma: no cover
        pytest.skip(f"libmpdx.so does not load on this host: {e}")


OK_ARGS = dict(n=1, max_nodes=64, H=64, dt=0.1, n_edge_checks=4, rounds=1)
REFUSALS = [("H", 1, "H 1,"), ("H", 1025, "H 1025,"), ("dt", 0.0, "dt 0,"), ("n_edge_checks", 1, "n_edge_checks 1,"), ("n_edge_checks", 257, "n_edge_checks 257,"),
            ("rounds", -1, "rounds -1"), ("max_nodes", 1, "max_nodes 1,"), ("n", 0, "n 0"), ("max_nodes", 20000, "20000 nodes x 7 dims need")]


@pytest.mark.parametrize("robot", ["RobotPointMass", "RobotPanda"])
def test_rrt_paths_refuses_bad_arguments_before_any_launch(lib, robot):
    import mpd_public_amd as m
    ds = m.TrajectoryDataset("EnvSimple2D" if robot == "RobotPointMass" else "EnvSpheres3D", robot)
    gp = ds.task._params("cpu")
    # host buffers stand in for the device pointers: a refused call never reaches a launch, so nothing dereferences them
    buf = (C.c_float * 64)()
    a = C.cast(buf, C.c_void_p)

    def call(ptrs=(a,) * 7, **kw):
        v = dict(OK_ARGS, **kw)
        return lib.mpdx_rrt_paths(C.byref(gp), *ptrs[:6], ptrs[6], v["n"], v["max_nodes"], v["H"], v["dt"], v["n_edge_checks"], v["rounds"], None)

    for key, value, text in REFUSALS:
        if key == "max_nodes" and value == 20000 and robot != "RobotPanda":
            continue      # (the LDS need of q_dim 7: 4 * (7168 + 7 H + 2048 + 40000 + 16 + primitives) B > 160 KB)
        assert call(**{key: value}) == -1, (key, value)
        msg = lib.mpdx_last_error().decode()
        assert msg.startswith("RRT paths:") and text in msg, (key, value, msg)
    for k in range(6):      # start, goal, nodes, parent, link, trajs_out (path_len, the 7th, may be null)
        ptrs = [a] * 7
        ptrs[k] = None
        assert call(tuple(ptrs)) == -1 and "RRT paths: null argument" in lib.mpdx_last_error().decode(), k
    assert lib.mpdx_rrt_paths(None, a, a, a, a, a, a, a, 1, 64, 64, 0.1, 4, 1, None) == -1 and "null argument" in lib.mpdx_last_error().decode()
    if robot == "RobotPanda":      # the largest max_nodes that fits is accepted by this check (not called: it would launch)
        need = lambda M: 4 * (1024 * 7 + 2 * 7 + 2048 + 2 * M + 16 + gp.n_prim_floats)   # noqa: E731
        assert need(20000) > 160 * 1024 > need(2048)
