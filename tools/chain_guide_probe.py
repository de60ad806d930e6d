#!/usr/bin/env python3
"""Time the guide kernel of the table-driven chain robots (csrc/chain.hpp); needs a GPU, one process, one device.

  python tools/chain_guide_probe.py [--parent-lib build_ab/libmpdx_parent.so] [--reps 200] [--rounds 5] [--out profiles/chain_guide_probe.md]

Method (tools/grid_guide_probe.py): mpdx_guide_time - gradient-only launches, `reps` back to back between ONE event pair after its own warm-up
launches - the variants of a shape alternating within each of `rounds` rounds (a dropped round in front warms everything), median over the rounds.
  (a) the Panda as a chain (RobotChain.panda()) against the Panda kernel (RobotPanda), same trajectories, B = 100 and B = 6400: the price of
      generality;
  (b) the test robots R3 and R8 (tests/chain_ref.py) at B = 100;
  (c) with --parent-lib (a libmpdx.so built from the parent commit): the existing point-mass and Panda guide launch, parent library against
      this tree's, interleaved parent, child, parent per round - the child against the parent's own spread (tools/scene_batch_probe.py, part b).
Writes the table as markdown and prints one JSON line."""
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
from helpers import obstacle_hugging_trajs, product_guide  # noqa: E402
from chain_ref import product_robot  # noqa: E402

TA = {"device": "cuda", "dtype": torch.float32}


def bind(path):
    lib = C.CDLL(str(path))
    for name in ("mpdx_guide_time", "mpdx_absmax", "mpdx_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def timer(lib, gp, x, grad, flag, npc, reps):
    B, H, D = x.shape
    st = torch.cuda.current_stream().cuda_stream

    def one():
        ms = C.c_float()
        rc = lib.mpdx_guide_time(C.byref(gp), x.data_ptr(), grad.data_ptr(), flag.data_ptr(), npc, B, H, D, reps, st, C.byref(ms))
        if rc:
            raise RuntimeError(f"mpdx_guide_time failed ({rc}): {lib.mpdx_last_error()}")
        return ms.value * 1e3
    return one


def alternate(variants, rounds):
    """{name: callable} -> {name: {median, min, max}} us per launch; round 0 is dropped."""
    times = {k: [] for k in variants}
    for rnd in range(rounds + 1):
        for k, fn in variants.items():
            v = fn()
            if rnd:
                times[k].append(v)
    return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}


def inputs(ds, B, lib):
    """Normalised trajectories inside the joint limits and their per-context range flags (contexts of 50, as bench.py's shards)."""
    ds_p = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args=TA) if ds.robot.q_dim == 7 else None
    if ds_p is not None:
        x = obstacle_hugging_trajs(ds_p, B, seed="trace", scale=0.95).cuda()
    else:
        from chain_ref import chain_trajs
        x = (0.95 * chain_trajs(ds.robot.q_dim, B, 64, "chain_probe")).cuda()
    flag = torch.zeros(max(1, B // 50), dtype=torch.int32, device="cuda")
    _lib.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), 50, B, 64, ds.state_dim, torch.cuda.current_stream().cuda_stream))
    return x, flag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "chain_guide_probe.md"))
    a = ap.parse_args()
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "panda": {}, "chains": {}, "existing": []}
    keep = []
    # (a) the Panda: its own kernel against the chain kernel
    ds_p, ds_c = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args=TA), m.TrajectoryDataset("EnvSpheres3D", m.RobotChain.panda(), tensor_args=TA)
    pg_p, pg_c = product_guide(ds_p).cuda(), product_guide(ds_c).cuda()
    keep += [pg_p, pg_c]
    for B in (100, 6400):
        x, flag = inputs(ds_c, B, lib)
        g1, g2 = torch.zeros_like(x), torch.zeros_like(x)
        v = {"panda_kernel": timer(lib, pg_p.device_params(x.device), x, g1, flag, 50, a.reps), "chain_kernel": timer(lib, pg_c.device_params(x.device), x, g2, flag, 50, a.reps)}
        r = alternate(v, a.rounds)
        torch.cuda.synchronize()
        r["chain_over_panda"] = round(r["chain_kernel"]["median"] / r["panda_kernel"]["median"], 3)
        r["max_abs_diff_of_the_increments"] = float((g1 - g2).abs().max())
        res["panda"][f"B{B}"] = r
        print(json.dumps({f"panda_B{B}": r}), flush=True)
    # (b) R3 and R8
    for name in ("R3", "R8"):
        ds = m.TrajectoryDataset("EnvSpheres3D", product_robot(name), tensor_args=TA)
        pg = product_guide(ds).cuda()
        keep.append(pg)
        x, flag = inputs(ds, 100, lib)
        g = torch.zeros_like(x)
        res["chains"][f"{name}_B100"] = alternate({"chain_kernel": timer(lib, pg.device_params(x.device), x, g, flag, 50, a.reps)}, a.rounds)["chain_kernel"]
        print(json.dumps({name: res["chains"][f"{name}_B100"]}), flush=True)
    # (c) the existing kernels, parent library against this tree's
    if a.parent_lib:
        parent = bind(a.parent_lib)
        for label, env_id, robot, B in (("point mass, B = 100", "EnvDense2D", "RobotPointMass", 100), ("Panda, B = 100", "EnvSpheres3D", "RobotPanda", 100),
                                        ("Panda, B = 6400", "EnvSpheres3D", "RobotPanda", 6400)):
            ds = m.TrajectoryDataset(env_id, robot, tensor_args=TA)
            pg = product_guide(ds).cuda()
            keep.append(pg)
            x = obstacle_hugging_trajs(ds, B, seed="trace", scale=0.95).cuda()
            flag = torch.zeros(max(1, B // 50), dtype=torch.int32, device="cuda")
            _lib.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), 50, B, 64, ds.state_dim, torch.cuda.current_stream().cuda_stream))
            gp, gc = torch.zeros_like(x), torch.zeros_like(x)
            par, chi = timer(parent, pg.device_params(x.device), x, gp, flag, 50, a.reps), timer(lib, pg.device_params(x.device), x, gc, flag, 50, a.reps)
            r = alternate({"parent_A": par, "child": chi, "parent_B": par}, a.rounds)
            torch.cuda.synchronize()
            row = {"case": label, "us": r, "parent_vs_itself_us": round(abs(r["parent_A"]["median"] - r["parent_B"]["median"]), 3),
                   "parent_round_to_round_us": round(max(r["parent_A"]["max"] - r["parent_A"]["min"], r["parent_B"]["max"] - r["parent_B"]["min"]), 3),
                   "child_minus_parent_us": round(r["child"]["median"] - 0.5 * (r["parent_A"]["median"] + r["parent_B"]["median"]), 3),
                   "outputs_bit_identical": bool(torch.equal(gp, gc))}
            res["existing"].append(row)
            print(json.dumps(row), flush=True)
    L = ["# Chain guide kernel: launch times", "",
         f"`tools/chain_guide_probe.py`, {res['device']}, one process; `mpdx_guide_time`, {a.reps} gradient-only launches per event pair, median of {a.rounds} alternating rounds",
         "(a dropped round in front), us per launch (min ... max over the rounds in brackets).  H = 64, 128 interpolated points, EnvSpheres3D.", "",
         "## (a) the Panda as a chain against the Panda kernel", "", "| batch | Panda kernel | chain kernel | chain / Panda | max abs diff of the increments |", "|---|---|---|---|---|"]
    f = lambda d: f"{d['median']} ({d['min']} ... {d['max']})"
    for k, r in res["panda"].items():
        L.append(f"| {k[1:]} | {f(r['panda_kernel'])} | {f(r['chain_kernel'])} | {r['chain_over_panda']} | {r['max_abs_diff_of_the_increments']:.3e} |")
    L += ["", "## (b) the test robots at B = 100", "", "| robot | chain kernel |", "|---|---|"]
    for k, r in res["chains"].items():
        L.append(f"| {k.split('_')[0]} | {f(r)} |")
    if res["existing"]:
        L += ["", "## (c) the existing guide launch, parent library against this tree's, interleaved", "",
              "Per round: parent (slot A), child, parent (slot B).  `parent vs itself` = |median A - median B|; `round to round` = the largest max - min of a parent slot.", "",
              "| case | parent A | child | parent B | parent vs itself | round to round | child - parent mean | same bits |", "|---|---|---|---|---|---|---|---|"]
        for r in res["existing"]:
            u = r["us"]
            L.append(f"| {r['case']} | {u['parent_A']['median']} | {u['child']['median']} | {u['parent_B']['median']} | {r['parent_vs_itself_us']} | {r['parent_round_to_round_us']} | "
                     f"{r['child_minus_parent_us']:+} | {r['outputs_bit_identical']} |")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(L) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
