#!/usr/bin/env python3
"""Time the chain guide kernel with and without the tool-axis term (csrc/chain.hpp) and the tool metrics kernel; needs a GPU, one process, one device.

  python tools/tool_axis_probe.py [--parent-lib build_ab/libmpdx_parent.so] [--reps 200] [--rounds 5] [--out profiles/tool_axis_probe.md]

Method (tools/chain_guide_probe.py): mpdx_guide_time - gradient-only launches, `reps` back to back between ONE event pair after its own warm-up
launches - the variants of a shape alternating within each of `rounds` rounds (a dropped round in front warms everything), median over the rounds.
Per (robot, batch): the parent library (slot A), this tree with the term off, the parent again (slot B), this tree with the term alone and with the
full composite + the term.  The parent library reads the leading members of the parameter block only (the tool members are appended).  Robots:
RobotChain.panda() and the test robot R8 (tests/chain_ref.py: 8 joints, 16 spheres, 24 pairs), H = 64, 128 interpolated points, B = 100 and 6400.
Also: LDS bytes of each configuration (the carve of guide_common.hpp, restated here) and the workgroups per CU they allow, and the time of
mpdx_traj_tool_metrics (n_check = 256) between one event pair.  Writes the table as markdown and prints one JSON line."""
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
from helpers import product_guide  # noqa: E402
from chain_ref import chain_trajs, product_robot  # noqa: E402
from tool_ref import product_guide_tool  # noqa: E402

TA = {"device": "cuda", "dtype": torch.float32}
MAX_TILT = 0.3


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


def chain_guide_lds_bytes(gp, H, tool):
    """guide_lds_layout(kGuideChain, ...).total * 4 of csrc/guide_common.hpp for a one-scene block."""
    qd = gp.q_dim
    D, N, slots = 2 * qd, gp.n_interp, _lib.MAX_FIELDS + (1 if tool else 0)
    fks = 6 * qd + 3 * _lib.ROBOT_CHAIN_MAX_SPHERES + 1
    per_point = fks + (3 if tool else 0) + slots * qd
    return 4 * (H * D + gp.n_chain_floats + 3 + N * per_point + slots * H * qd + 2 * H * D + 8 + 3 + gp.n_prim_floats + 3 + 2 * D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tool_axis_probe.md"))
    a = ap.parse_args()
    lib = _lib.load()
    parent = bind(a.parent_lib) if a.parent_lib else None
    st = torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "guide": [], "metrics": []}
    keep = []
    for name in ("Panda", "R8"):
        ds = m.TrajectoryDataset("EnvSpheres3D", product_robot(name), tensor_args=TA)
        qd = ds.robot.q_dim
        pg_off = product_guide(ds).cuda()
        pg_alone, cost = product_guide_tool(ds, qd, MAX_TILT, "alone")
        pg_full, _ = product_guide_tool(ds, qd, MAX_TILT, "full")
        pg_alone, pg_full = pg_alone.cuda(), pg_full.cuda()
        keep += [pg_off, pg_alone, pg_full]
        for B in (100, 6400):
            x = (0.95 * chain_trajs(qd, B, 64, "tool_probe")).cuda()
            flag = torch.zeros(max(1, B // 50), dtype=torch.int32, device="cuda")
            _lib.check(lib.mpdx_absmax(x.data_ptr(), flag.data_ptr(), 50, B, 64, ds.state_dim, st))
            gpar, goff, g1, g2 = (torch.zeros_like(x) for _ in range(4))
            gps = {k: g.device_params(x.device) for k, g in (("off", pg_off), ("alone", pg_alone), ("full", pg_full))}
            v = {}
            if parent is not None:
                v["parent_A"] = timer(parent, gps["off"], x, gpar, flag, 50, a.reps)
            v["term_off"] = timer(lib, gps["off"], x, goff, flag, 50, a.reps)
            if parent is not None:
                v["parent_B"] = v["parent_A"]
            v["tool_alone"] = timer(lib, gps["alone"], x, g1, flag, 50, a.reps)
            v["full_plus_tool"] = timer(lib, gps["full"], x, g2, flag, 50, a.reps)
            r = alternate(v, a.rounds)
            torch.cuda.synchronize()
            row = {"robot": name, "B": B, "us": r,
                   "lds_bytes": {"term_off": chain_guide_lds_bytes(gps["off"], 64, False), "tool_alone": chain_guide_lds_bytes(gps["alone"], 64, True),
                                 "full_plus_tool": chain_guide_lds_bytes(gps["full"], 64, True)}}
            row["workgroups_per_cu_by_lds"] = {k: min(2, (160 * 1024) // b) for k, b in row["lds_bytes"].items()}   # (__launch_bounds__(512, 2): at most two)
            if parent is not None:
                row["parent_vs_itself_us"] = round(abs(r["parent_A"]["median"] - r["parent_B"]["median"]), 3)
                row["parent_round_to_round_us"] = round(max(r["parent_A"]["max"] - r["parent_A"]["min"], r["parent_B"]["max"] - r["parent_B"]["min"]), 3)
                row["off_minus_parent_us"] = round(r["term_off"]["median"] - 0.5 * (r["parent_A"]["median"] + r["parent_B"]["median"]), 3)
                row["off_bit_identical_to_parent"] = bool(torch.equal(gpar, goff))
            res["guide"].append(row)
            print(json.dumps(row), flush=True)
            # the metrics kernel: reps launches between one event pair, after a warm-up launch
            xu = ds.unnormalize_trajectories(x).contiguous()
            ds.task.tool_axis_metrics(xu, cost, n_check=256)
            tms = []
            for rnd in range(a.rounds + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                gp = gps["alone"]
                out = torch.empty((B, 2), device="cuda")
                e0.record()
                for _ in range(a.reps):
                    lib.mpdx_traj_tool_metrics(C.byref(gp), xu.data_ptr(), out.data_ptr(), None, 256, B, 64, ds.state_dim, st)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    tms.append(e0.elapsed_time(e1) * 1e3 / a.reps)
            mrow = {"robot": name, "B": B, "us": {"median": round(statistics.median(tms), 3), "min": round(min(tms), 3), "max": round(max(tms), 3)}}
            res["metrics"].append(mrow)
            print(json.dumps(mrow), flush=True)
    f = lambda d: f"{d['median']} ({d['min']} ... {d['max']})"
    L = ["# Tool-axis term: launch times of the chain guide kernel", "",
         f"`tools/tool_axis_probe.py`, {res['device']}, one process; `mpdx_guide_time`, {a.reps} gradient-only launches per event pair, median of {a.rounds} alternating rounds",
         "(a dropped round in front), us per launch (min ... max over the rounds in brackets).  H = 64, 128 interpolated points, EnvSpheres3D, max_tilt 0.3, frame = n_joints.", "",
         "## Guide launch", "", "Per round: parent library (slot A), this tree with the term off, parent (slot B), the term alone, the full composite + the term.", "",
         "| robot | B | parent A | term off | parent B | parent vs itself | parent round to round | off - parent mean | off == parent bits | tool alone | full + tool |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["guide"]:
        u = r["us"]
        if "parent_A" in u:
            L.append(f"| {r['robot']} | {r['B']} | {f(u['parent_A'])} | {f(u['term_off'])} | {f(u['parent_B'])} | {r['parent_vs_itself_us']} | {r['parent_round_to_round_us']} | "
                     f"{r['off_minus_parent_us']:+} | {r['off_bit_identical_to_parent']} | {f(u['tool_alone'])} | {f(u['full_plus_tool'])} |")
        else:
            L.append(f"| {r['robot']} | {r['B']} | - | {f(u['term_off'])} | - | - | - | - | - | {f(u['tool_alone'])} | {f(u['full_plus_tool'])} |")
    L += ["", "## LDS per workgroup and workgroups per CU (160 KB of LDS, `__launch_bounds__(512, 2)`)", "",
          "| robot | term off | tool alone | full + tool |", "|---|---|---|---|"]
    for r in res["guide"]:
        if r["B"] == 100:
            L.append(f"| {r['robot']} | " + " | ".join(f"{r['lds_bytes'][k]} B, {r['workgroups_per_cu_by_lds'][k]} / CU" for k in ("term_off", "tool_alone", "full_plus_tool")) + " |")
    L += ["", "## `traj_tool_chain_kernel` (mpdx_traj_tool_metrics, n_check = 256, one event pair around the launches)", "", "| robot | B | us per launch |", "|---|---|---|"]
    for r in res["metrics"]:
        L.append(f"| {r['robot']} | {r['B']} | {f(r['us'])} |")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(L) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
