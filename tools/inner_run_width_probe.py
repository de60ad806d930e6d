#!/usr/bin/env python3
"""Width of the two persistent runs of mpdx_plan (csrc/inner_run.hpp) against the batch -> profiles/inner_run_narrow_ab.md.  Needs a GPU.

cfg2-shaped plans (bench.py: D = 4, dim_mults (1, 2, 4, 8), T = 100 + 5, unguided, return_chain) at B = 16, 32, 64, 100, 128 on ONE handle, the
settings interleaved per round: both runs, the seven-layer run alone and the tail run alone (set_inner_run_parts), each at width 32 and 16
(set_inner_run_width).  Per setting the median over the rounds of the mean plan time, and the spread (max - min) of the rounds.  The automatic width
(mpdx.hip inner_run_auto_width / tail_run_auto_width) is read from this table: a run takes width 16 at the batches where its `alone` row at 16 is
below the row at 32 by more than both rows' spreads.

  python tools/inner_run_width_probe.py [--batches 16,32,64,100,128] [--rounds 5] [--plans 10]
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
    ap.add_argument("--batches", default="16,32,64,100,128")
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
    settings = [(name, parts, w) for name, parts in (("both runs", 3), ("seven alone", 1), ("tail alone", 2)) for w in (32, 16)]
    print("| B | setting | width 32: ms per plan (spread) | width 16: ms per plan (spread) | 16 - 32 |")
    print("|---|---|---|---|---|")
    for B in [int(b) for b in args.batches.split(",")]:
        def plan():
            return dm.run_inference(None, hc, n_samples=B, horizon=64, return_chain=True, n_diffusion_steps_without_noise=5,
                                    noise_std_extra_schedule_fn=lambda t: 0.5)
        times = {s: [] for s in settings}
        for _ in range(args.rounds):
            for s in settings:
                dm.model.set_inner_run_parts(s[1])
                dm.model.set_inner_run_width(s[2])
                plan(); plan()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.plans):
                    plan()
                torch.cuda.synchronize()
                times[s].append((time.perf_counter() - t0) / args.plans * 1e3)
                assert dm.model.status() == 0 and dm.model.inner_run_layers() == 105 * ((7 if s[1] & 1 else 0) + (4 if s[1] & 2 else 0))
        for name, parts in (("both runs", 3), ("seven alone", 1), ("tail alone", 2)):
            cell = {}
            for w in (32, 16):
                v = times[(name, parts, w)]
                cell[w] = (statistics.median(v), max(v) - min(v))
            print(f"| {B} | {name} | {cell[32][0]:.3f} ({cell[32][1]:.3f}) | {cell[16][0]:.3f} ({cell[16][1]:.3f}) | {cell[16][0] - cell[32][0]:+.3f} |", flush=True)
    dm.model.set_inner_run(True)
    dm.model.set_inner_run_width(0)


if __name__ == "__main__":
    main()
