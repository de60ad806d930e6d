"""rrt_connect_kernel replayed decision by decision by its float64 restatement (tests/rrt_ref.py): given its seed the kernel is deterministic, so
every insertion of both trees - which tree, which index, which parent, which coordinates - every count, link and iteration number has ONE right
value.  The replay adopts the device's float32 coordinates after checking them (2e-6), so a later decision is judged on the device's own nodes;
a decision float64 cannot settle for a float32 evaluation (an edge's largest slack within 1e-5 of zero, two nearest candidates within 1e-6
relative, a steer within 1e-6 of the step length) ends that problem's comparison - at most one problem in eight per case may end so.

The seed is rebuilt from the rule RRTConnectBatch.grow documents: generator.initial_seed() * 1000003 + the process's launch count, mod 2^64.  The
launch count is set before grow() so that each case runs the seed its properties were established for (tests/test_rrt_ref_cpu.py)."""
import time

import numpy as np
import pytest
import torch

import rrt_ref
from helpers import rrt_problem, single_thread

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(rrt_ref.CASES))
def test_rrt_connect_kernel_equals_its_replay(name, monkeypatch):
    import mpd_public_amd as m
    from mpd_public_amd.generate_trajectories import RRTConnectBatch
    case = rrt_ref.CASES[name]
    ds = m.TrajectoryDataset(case["env"], case["robot"], tensor_args={"device": "cuda", "dtype": torch.float32})
    p = rrt_problem(ds, case)
    n = case["n"]
    gen = torch.Generator(device="cuda").manual_seed(case["gen_seed"])
    rrt = RRTConnectBatch(ds.task, torch.tensor(case["start"], device="cuda"), torch.tensor(case["goal"], device="cuda"), n, step_size=case["step"],
                          max_nodes=case["max_nodes"], n_edge_checks=case["n_edge_checks"], generator=gen)
    if "box" in case:
        rrt.lo, rrt.hi = (torch.tensor(v, device="cuda") for v in case["box"])
    monkeypatch.setattr(RRTConnectBatch, "_launches", case["launch"] - 1)
    used = rrt.grow(max_iters=case["max_iters"], max_connect_steps=case["max_connect_steps"])
    assert (gen.initial_seed() * 1000003 + RRTConnectBatch._launches) % 2 ** 64 == p.seed
    rec = rrt_ref.Trees(*(v.cpu().numpy() for v in (rrt.nodes, rrt.parent, rrt.count, rrt.link, rrt.iters)))
    t0 = time.perf_counter()
    with single_thread():
        rep = rrt_ref.compare(rec, p)
    solved = int((rec.link[:, 0] >= 0).sum())
    print(f"{name}: {used} iterations at most, {solved}/{n} solved, largest tree {int(rec.count.max())}; replay {time.perf_counter() - t0:.1f} s: "
          f"{rep.insertions} insertions and {rep.edge_checks} edge decisions verified, {len(rep.cut_short)} of {n} problems cut short {rep.cut_short}")
    assert rep.mismatches == [], rep.mismatches
    assert 8 * len(rep.cut_short) <= n, f"problems cut short at an ambiguous decision: {rep.cut_short}"
    if name == "narrow":
        assert int((rec.count.max(1) > 256).sum()) >= 2 and bool((rec.iters[rec.link[:, 0] < 0] == case["max_iters"]).all())
    if name == "narrow_small_budget":
        assert int((rec.count.max(1) == case["max_nodes"]).sum()) >= 6
    if name != "ties":      # (its sampling box is one point)
        dirs = [d for d in rep.first_dirs if d is not None]
        assert len(dirs) >= n // 2 and rrt_ref.directions_span(dirs), "first extensions of the problems: the sampler's directions are degenerate"
