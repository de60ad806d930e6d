#!/usr/bin/env python3
"""The paired joined launch of mpdx_plan (csrc/fused_level.hpp fused_join_split_kernel) against the batch -> profiles/level_split_ab.md.  Needs a GPU.

cfg2-shaped plans (bench.py: D = 4, dim_mults (1, 2, 4, 8), T = 100 + 5, unguided, return_chain) at B = 16, 64, 100, 128 on ONE handle, the option
(set_level_split) off and on interleaved per round.  Per setting the median over the rounds of the mean plan time, and the spread (max - min) of the
rounds.  The automatic rule (mpdx.hip level_split_auto) is read from this table: a batch takes the paired launch where `on` is below `off` by at least
three times the spread of `off`.

  python tools/level_split_probe.py [--batches 16,64,100,128] [--rounds 5] [--plans 10]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64,100,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plans", type=int, default=10)
    args = ap.parse_args()
    import torch
    import bench
    from mpd_public_amd import synthetic as syn
    dm, _ = bench.build_model(4, (1, 2, 4, 8), 100, "cuda")
    dm.manual_seed(30)
    hc = {0: torch.from_numpy(syn.synth_tensor("bench_hc0", (4,), "uniform", 0.6)).cuda(),
          63: torch.from_numpy(syn.synth_tensor("bench_hc1", (4,), "uniform", 0.6)).cuda()}
    print("| B | off: ms per plan (spread) | on: ms per plan (spread) | on - off | 3 x spread of off |")
    print("|---|---|---|---|---|")
    for B in [int(b) for b in args.batches.split(",")]:
        def plan():
            return dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, n_diffusion_steps_without_noise=5,
                                    noise_std_extra_schedule_fn=lambda t: 0.5)
        times = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                dm.model.set_level_split(on)
                plan(); plan()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.plans):
                    plan()
                torch.cuda.synchronize()
                times[on].append((time.perf_counter() - t0) / args.plans * 1e3)
                assert dm.model.status() == 0 and dm.model.plan_split() == (104 if on else 0) and dm.model.plan_joined() == 104
        m = {on: (statistics.median(v), max(v) - min(v)) for on, v in times.items()}
        print(f"| {B} | {m[False][0]:.3f} ({m[False][1]:.3f}) | {m[True][0]:.3f} ({m[True][1]:.3f}) | {m[True][0] - m[False][0]:+.3f} | {3 * m[False][1]:.3f} |", flush=True)
    dm.model.set_level_split(None)


if __name__ == "__main__":
    main()
