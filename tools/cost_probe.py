#!/usr/bin/env python3
"""Time the cost-value kernel (mpdx_traj_costs, csrc/costs.hpp) next to the metrics kernel (mpdx_traj_metrics) on the same trajectories with
n_check = n_points; needs a GPU, one process, one device.  Prints a markdown table and one JSON line.

  python tools/cost_probe.py [--rounds 7] [--window 0.2] [--metrics-lib build_ab/libmpdx_parent.so] [--out FILE.md]

Cases: the 2-D point mass (EnvSimple2D) at B = 100; the Panda (EnvSpheres3D) at B = 100 and 512, with the primitive tables and with the fixed
objects as a signed-distance grid at 2 cm; n_points 128 and 256 each.  The cost launch evaluates the whole composite of inference.py (every collision
field and the GP prior) and writes the clearance; a second variant also writes the point costs.  --metrics-lib: another build of the library whose
mpdx_traj_metrics is timed (the parent commit's, for an A/B across commits; default: this tree's - the metrics kernels compile from unchanged text).
Per variant: `reps` launches back to back between ONE event pair after warm-up launches, reps chosen so that a window lasts about --window seconds; the
variants alternate within each of `rounds` rounds (round 0 warms and is dropped); median, min and max over the rounds."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch  # noqa: E402
import mpd_public_amd as m  # noqa: E402
from mpd_public_amd import _lib  # noqa: E402
from mpd_public_amd.guides import build_device_params  # noqa: E402
from helpers import obstacle_hugging_trajs  # noqa: E402

TA = {"device": "cuda", "dtype": torch.float32}
CASES = [("point mass", "EnvSimple2D", "RobotPointMass", None, 100), ("Panda", "EnvSpheres3D", "RobotPanda", None, 100),
         ("Panda", "EnvSpheres3D", "RobotPanda", None, 512), ("Panda, grid 2 cm", "EnvSpheres3D", "RobotPanda", 0.02, 100),
         ("Panda, grid 2 cm", "EnvSpheres3D", "RobotPanda", 0.02, 512)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--metrics-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cost_probe needs a GPU (nothing is measured without one)")
    lib = _lib.load()
    mlib = lib
    if a.metrics_lib:
        mlib = C.CDLL(str(Path(a.metrics_lib).resolve()))
        mlib.mpdx_traj_metrics.restype, mlib.mpdx_traj_metrics.argtypes = _lib.SIGNATURES["mpdx_traj_metrics"]
    st = _lib.current_stream()
    variants, keep = {}, []
    for label, env_id, robot_id, cell, B in CASES:
        ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA, sdf_grid=None if cell is None else dict(cell_size=cell, mode="linear"))
        H, D = ds.n_support_points, ds.state_dim
        x = ds.unnormalize_trajectories(obstacle_hugging_trajs(ds, B, seed=f"cost_probe/{robot_id}/{B}").cuda()).contiguous()
        costs = [m.CostCollision(ds.robot, H, field=f) for f in ds.task.get_collision_fields()] + [m.CostGPTrajectory(ds.robot, H, 5.0 / H)]
        gp, prims = build_device_params(ds.robot, ds.env.dim, ds.task.obstacle_cutoff_margin, None, None, costs, [1.0] * len(costs), True, 128, True, 1.0, "cuda")
        gm = ds.task._params(x.device)
        keep += [ds, x, gp, prims, gm]
        for N in (128, 256):
            cost = torch.empty((B, _lib.COST_SLOTS), device="cuda")
            clr = torch.empty((B, _lib.MAX_FIELDS), device="cuda")
            pts = torch.empty((B, N, _lib.MAX_FIELDS + 1), device="cuda")
            out4 = torch.empty((B, 4), device="cuda")
            keep += [cost, clr, pts, out4]
            key = f"{label} | {B} | {N}"

            def f_cost(gp=gp, x=x, cost=cost, clr=clr, N=N, B=B, H=H, D=D, pts=None):
                _lib.check(lib.mpdx_traj_costs(C.byref(gp), x.data_ptr(), cost.data_ptr(), clr.data_ptr(), pts, N, B, H, D, st), "mpdx_traj_costs")

            def f_pts(f=f_cost, pts=pts):
                f(pts=pts.data_ptr())

            def f_met(gm=gm, x=x, out4=out4, N=N, B=B, H=H, D=D):
                rc = mlib.mpdx_traj_metrics(C.byref(gm), x.data_ptr(), out4.data_ptr(), N, B, H, D, st)
                if rc:
                    raise RuntimeError(f"mpdx_traj_metrics failed ({rc})")
            variants[key] = {"costs": f_cost, "costs + point costs": f_pts, "metrics": f_met}
    reps = {}
    for key, vs in variants.items():
        for name, fn in vs.items():
            timed(fn, 5)
            reps[(key, name)] = int(min(20000, max(10, a.window * 1e6 / max(timed(fn, 10), 1e-3))))
    times = {k: [] for k in reps}
    for rnd in range(a.rounds + 1):
        for key, vs in variants.items():
            for name, fn in vs.items():
                us = timed(fn, reps[(key, name)])
                if rnd:
                    times[(key, name)].append(us)
    torch.cuda.synchronize()
    lines = ["| case | B | n_points | mpdx_traj_costs us (min - max) | with point costs us | mpdx_traj_metrics us (min - max) | costs / metrics |", "|---|---|---|---|---|---|---|"]
    info = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "metrics_lib": a.metrics_lib or "this tree", "us_per_launch": {}}
    for key in variants:
        med = {n: statistics.median(times[(key, n)]) for n in variants[key]}
        rng = {n: (min(times[(key, n)]), max(times[(key, n)])) for n in variants[key]}
        info["us_per_launch"][key] = {n: round(v, 2) for n, v in med.items()}
        lines.append(f"| {key} | {med['costs']:.1f} ({rng['costs'][0]:.1f} - {rng['costs'][1]:.1f}) | {med['costs + point costs']:.1f} | "
                     f"{med['metrics']:.1f} ({rng['metrics'][0]:.1f} - {rng['metrics'][1]:.1f}) | {med['costs'] / med['metrics']:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    print(json.dumps(info))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n```json\n" + json.dumps(info) + "\n```\n")


if __name__ == "__main__":
    main()
