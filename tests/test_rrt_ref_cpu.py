"""tests/rrt_ref.py checked without a GPU: the teacher-forced replay accepts the reference's own trees, REPORTS each of the deliberately wrong
searches (rrt_ref.FAULTS), and the cases tests/test_gpu_rrt_replay.py runs on the device have the properties they are there for."""
import numpy as np
import pytest
import torch

import rrt_ref
from helpers import rrt_problem, single_thread

_CACHE = {}


def _problem(name):
    if name not in _CACHE:
        import mpd_public_amd as m
        case = rrt_ref.CASES[name]
        ds = m.TrajectoryDataset(case["env"], case["robot"], tensor_args={"device": "cpu", "dtype": torch.float32})
        _CACHE[name] = rrt_problem(ds, case)
    return _CACHE[name]


def _free(name, problems=None, fault=None):
    key = (name, None if problems is None else tuple(problems), fault)
    if key not in _CACHE:
        with single_thread():
            _CACHE[key] = rrt_ref.free_run(_problem(name), fault, problems)
    return _CACHE[key]


def _compare(trees, name, problems=None):
    with single_thread():
        return rrt_ref.compare(trees, _problem(name), problems)


@pytest.mark.parametrize("name", list(rrt_ref.CASES))
def test_start_and_goal_are_clear_of_obstacles(name):
    p = _problem(name)
    assert float(np.max(p.slack_fn(np.concatenate([p.start, p.goal])))) < -0.02
    assert rrt_ref.case_seed(rrt_ref.CASES[name]) == p.seed < 2 ** 64


# (case, problems replayed): every problem of the cheap cases; of the long ones a solved problem with a tree beyond 256 nodes and a short one
SELF = [("dense", None), ("narrow", (1, 3)), ("narrow_small_budget", None), ("dense_24_checks", None), ("ties", None), ("panda", (1,)), ("pm3", None)]


@pytest.mark.parametrize("name,problems", SELF)
def test_replay_accepts_the_reference_itself(name, problems):
    trees = _free(name, problems)
    rep = _compare(trees, name, problems)
    assert rep.mismatches == [] and rep.cut_short == [] and rep.insertions == int(trees.count.sum()) - 2 * len(trees.count)
    assert sum(trees.ambiguous) == 0, "the cases were chosen free of ambiguous decisions"
    dirs = [d for d in rep.first_dirs if d is not None]
    if problems is None and name != "ties":     # (its sampling box is one point: every problem extends the same way)
        assert len(dirs) >= len(trees.count) // 2 and rrt_ref.directions_span(dirs)


# (fault, case, problems): the cheapest problems on which the fault changes the trees
MUTANTS = [("rounds9", "dense", (5,)), ("swap_counters", "dense", (5,)), ("nearest256", "narrow", (1,)), ("tie_high", "ties", (1,)),
           ("dup_reached", "dense", (5,)), ("w_over_n", "dense", (1,))]


@pytest.mark.parametrize("fault,name,problems", MUTANTS)
def test_replay_reports_a_wrong_search(fault, name, problems):
    assert fault in rrt_ref.FAULTS
    with single_thread():
        wrong = rrt_ref.free_run(_problem(name), fault, problems)
    rep = _compare(wrong, name, problems)
    print(fault, rep.mismatches)
    assert len(rep.mismatches) == len(problems) and rep.cut_short == []
    assert _compare(_free(name, problems), name, problems).mismatches == []      # ... and the same problems pass without the fault


def test_every_fault_has_a_mutant():
    assert sorted(m[0] for m in MUTANTS) == sorted(rrt_ref.FAULTS)


def test_cases_have_the_properties_the_gpu_tests_rely_on():
    narrow = _free("narrow")
    assert int((narrow.count.max(1) > 256).sum()) >= 2, "the strided part of the nearest loop needs trees beyond 256 nodes"
    cap = rrt_ref.CASES["narrow"]["max_iters"]
    unsolved = narrow.link[:, 0] < 0
    assert unsolved.any() and (~unsolved).any() and (narrow.iters[unsolved] == cap).all() and (narrow.iters[~unsolved] < cap).all()
    assert (narrow.link[unsolved] == -1).all() and sum(narrow.ambiguous) == 0
    small = _free("narrow_small_budget")
    M = rrt_ref.CASES["narrow_small_budget"]["max_nodes"]
    full = small.count.max(1) == M
    assert int(full.sum()) >= 6 and (small.link[full] == -1).all() and (small.iters[full] < rrt_ref.CASES["narrow_small_budget"]["max_iters"]).all()
    ties = _free("ties")
    p = _problem("ties")
    for b in range(len(ties.count)):      # hundreds of copies of the box's point in each tree, all children of its FIRST copy
        for t in (0, 1):
            at = np.flatnonzero((ties.nodes[b, t, :ties.count[b, t]] == p.q_lo.astype(np.float32)).all(-1))
            assert len(at) > 256 and (ties.parent[b, t, at[1:]] == at[0]).all()
    panda = _free("panda")
    assert (panda.link[:, 0] >= 0).any() and int(panda.count.sum()) > 100 and sum(panda.ambiguous) == 0
    pm3 = _free("pm3")      # every problem solved, in three dimensions (first extensions below: the directions span all three axes)
    assert (pm3.link[:, 0] >= 0).all() and pm3.nodes.shape[-1] == 3 and int(pm3.count.sum()) > 40 and sum(pm3.ambiguous) == 0
    assert (pm3.iters < rrt_ref.CASES["pm3"]["max_iters"]).all() and int(pm3.iters.max()) > 10
    for name, trees in (("narrow", narrow), ("panda", panda), ("pm3", pm3)):      # first extensions: inserted in at least half the problems, directions not degenerate
        dirs = [d for d in trees.first_dirs if d is not None]
        assert len(dirs) >= len(trees.count) // 2 and rrt_ref.directions_span(dirs), name
