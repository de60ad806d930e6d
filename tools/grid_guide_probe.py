#!/usr/bin/env python3
"""Time the guide kernel with the fixed objects as primitives and as a signed-distance grid (both lookup modes); needs a GPU, one process, one device.

  python tools/grid_guide_probe.py [--primitive-only] [--reps 200] [--rounds 5]

Shapes: point mass (EnvDense2D) B = 100, Panda (EnvSpheres3D) B = 100 and B = 6400 (the cfg 4 / cfg 5 shard shapes).  Per shape and variant:
mpdx_guide_time (gradient-only launches, `reps` back to back between ONE event pair, after its own warm-up launches), the variants alternating within
each of `rounds` rounds, median over the rounds.  Prints one JSON line (us per launch, and the grid / primitive ratio per shape).
--primitive-only times the primitive guide alone - the form that also runs in a checkout that has no grid field (A/B of the primitive path
against another build: run it there the same way, alternating the two)."""
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
from helpers import product_guide, obstacle_hugging_trajs  # noqa: E402

SHAPES = [("pointmass_B100", "EnvDense2D", "RobotPointMass", 100, 0.01), ("panda_B100", "EnvSpheres3D", "RobotPanda", 100, 0.02),
          ("panda_B6400", "EnvSpheres3D", "RobotPanda", 6400, 0.02)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--primitive-only", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    ta = {"device": "cuda", "dtype": torch.float32}
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    out = {"lib": str(_lib.lib_path().name), "reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "us_per_launch": {}, "grid_over_primitive": {}}
    for tag, env_id, robot_id, B, cell in SHAPES:
        variants = {"primitive": None} if a.primitive_only else {"primitive": None, "grid_linear": "linear", "grid_nearest": "nearest"}
        ds0 = m.TrajectoryDataset(env_id, robot_id, tensor_args=ta)
        x = obstacle_hugging_trajs(ds0, B, seed="trace", scale=0.95).cuda()
        flag = torch.zeros(max(1, B // 50), dtype=torch.int32, device="cuda")
        g = torch.zeros_like(x)
        guides, keep = {}, []
        for name, mode in variants.items():
            ds = ds0 if mode is None else m.TrajectoryDataset(env_id, robot_id, tensor_args=ta, sdf_grid=dict(cell_size=cell, mode=mode))
            pg = product_guide(ds).cuda()
            guides[name] = pg.device_params(x.device)
            keep.append(pg)
        ms, times = C.c_float(0), {k: [] for k in variants}
        for rnd in range(a.rounds + 1):   # round 0 warms every variant and is dropped
            for name, gp in guides.items():
                _lib.check(lib.mpdx_guide_time(C.byref(gp), x.data_ptr(), g.data_ptr(), flag.data_ptr(), 50, B, 64, ds0.state_dim, a.reps, st, C.byref(ms)))
                if rnd:
                    times[name].append(ms.value * 1e3)
        med = {k: round(statistics.median(v), 3) for k, v in times.items()}
        out["us_per_launch"][tag] = {k: {"median": med[k], "min": round(min(times[k]), 3), "max": round(max(times[k]), 3)} for k in times}
        if not a.primitive_only:
            out["grid_over_primitive"][tag] = {k: round(med[k] / med["primitive"], 4) for k in med if k != "primitive"}
            gf = [f for f in keep[1].dataset.task.get_collision_fields() if f.kind == _lib.FIELD_GRID][0].grid
            out.setdefault("grid_bytes", {})[tag] = {"sdf_plane": gf.n_nodes * 4, "nodes": list(gf.shape), "cell": cell}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
