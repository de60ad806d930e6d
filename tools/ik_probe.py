#!/usr/bin/env python3
"""Time the inverse-kinematics kernel (csrc/ik.hpp) on the Panda as a chain; needs a GPU, one process, one device.

  python tools/ik_probe.py [--reps 20] [--rounds 5] [--out profiles/ik_probe.md]

Work: 64 targets x 64 restarts x 100 iterations, position + orientation.  The tolerances are set below anything fp32 reaches, so that no restart
stops early and every lane does all 100 iterations (targets FK(q*) of random q*, seeds uniform in the limits, fixed generator).
  kernel     `reps` solve_ik calls (one launch each) between ONE event pair after a warm-up call, median over `rounds` rounds
  reference  the fp32 torch reference of tests/ik_ref.py on the CPU of the same host, the same work, wall clock of one solve
Writes the table as markdown and prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mpd_public_amd as m  # noqa: E402
import ik_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, R, iters = 64, 64, 100
    rng = np.random.default_rng(0)
    tpos, trot = ik_ref.target_of("Panda", ik_ref.random_q("Panda", (n,), rng, margin=0.2))
    seeds = ik_ref.random_q("Panda", (n, R), rng)
    kw = dict(pos_tol=1e-12, rot_tol=1e-12, rot_weight=ik_ref.ROT_WEIGHT)
    rob = m.RobotChain.panda()
    tp, tr, q0 = tpos.float().cuda(), trot.float().cuda(), seeds.cuda()
    solve = lambda: m.solve_ik(rob, tp, tr, n_restarts=R, q_init=q0, max_iters=iters, **kw)
    res = solve()
    torch.cuda.synchronize()
    assert int(res.iters.min()) == iters, "a restart stopped early"
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            solve()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.reps)
    ref = ik_ref.IKRef("Panda", torch.float32, adaptive=True, **kw, **ik_ref.LAMBDA)
    t0 = time.perf_counter()
    s = ref.solve(seeds, tpos[:, None, :], trot[:, None, :, :], max_iters=iters)
    cpu_s = time.perf_counter() - t0
    assert int(s["iters"].min()) == iters
    rec = dict(n_targets=n, restarts=R, iterations=iters, kernel_ms_median=statistics.median(ms), kernel_ms_min=min(ms), kernel_ms_max=max(ms),
               cpu_fp32_reference_s=cpu_s, cpu_threads=torch.get_num_threads(), device=torch.cuda.get_device_name(0))
    if a.out:
        Path(a.out).write_text(
            "# Inverse-kinematics kernel: time of one solve\n\n"
            f"`tools/ik_probe.py`, {rec['device']}, one process.  Panda as a chain, {n} targets x {R} restarts x {iters} iterations, position + orientation,\n"
            f"tolerances below fp32 so that every restart runs all iterations.  Kernel: {a.reps} `solve_ik` calls (one launch each, host call included) per event pair,\n"
            f"median of {a.rounds} rounds.  Reference: the fp32 torch restatement of `tests/ik_ref.py` on the same host's CPU ({rec['cpu_threads']} threads), one solve, wall clock.\n\n"
            "| | time of one solve |\n|---|---|\n"
            f"| `ik_solve_kernel<7>` | {rec['kernel_ms_median']:.3f} ms ({rec['kernel_ms_min']:.3f} ... {rec['kernel_ms_max']:.3f}) |\n"
            f"| fp32 torch reference, CPU | {cpu_s:.2f} s |\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
