#!/usr/bin/env python3
"""Time the depth-camera fusion (mpdx_tsdf_integrate) on the device, alone and followed by the occupancy transform it feeds
(mpdx_sdf_grid_from_occupancy, sdf plane; the per-frame cost of a perception loop), next to the transform alone and to the numpy reference
(tests/tsdf_ref.py) on this host's CPU; needs a GPU, one process, one device.  Writes a markdown report.

  python tools/tsdf_probe.py [--rounds 7] [--window 0.3] [--out profiles/tsdf_probe.md]

Grid: the Panda's workspace (EnvSpheres3D) at 2 cm on the box of grid_sdf.grid_spec_for (132 x 132 x 112 nodes).  Frames: 640 x 480, the
environment's fixed spheres and a floor ray-cast by tests/tsdf_ref.py from four cameras around the workspace (fx = fy = 480).  Per variant: `reps`
calls back to back between ONE hipEvent pair after warm-up calls, reps chosen so that a window lasts about --window seconds; the variants alternate
within each of `rounds` rounds (round 0 warms and is dropped); median, min and max over the rounds.  Before anything is timed, the device planes of
one fused frame are compared with the reference bit for bit."""
import argparse
import ctypes as C
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
from mpd_public_amd import _lib  # noqa: E402
from mpd_public_amd.planning import grid_spec_for  # noqa: E402
import tsdf_ref as R  # noqa: E402

W, H, FOCAL = 640, 480, 480.0


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def frames():
    env = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda").env
    o = env.obj_fixed
    spheres = np.concatenate([np.asarray(o.sphere_centers, np.float64), np.asarray(o.sphere_radii, np.float64)[:, None]], 1)
    floor = np.array([[0.0, 0.0, -0.45, 5.0, 5.0, 0.05]])
    K = (FOCAL, FOCAL, (W - 1) / 2, (H - 1) / 2)
    out = []
    for k in range(4):
        a = 2 * np.pi * (k + 0.3) / 4
        Mw = R.look_at((2.6 * np.cos(a), 2.6 * np.sin(a), 1.9), (0.0, -0.2, 0.5))
        out.append(R.camera(R.render(spheres, floor, K, Mw, W, H), K, Mw))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tsdf_probe.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_probe needs a GPU (nothing is measured without one)")
    lib = _lib.load()
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda")
    cell, trunc, max_weight = 0.02, 0.06, 20.0
    shape_xyz, origin = grid_spec_for(ds.task.ws_min, ds.task.ws_max, cell)
    shape = tuple(reversed(shape_xyz))
    nodes = int(np.prod(shape))
    cams = frames()
    imgs = [torch.from_numpy(c["depth"]).cuda() for c in cams]
    rec = (_lib.DepthCamera * 4)()
    for k, c in enumerate(cams):
        r = rec[k]
        r.depth, r.width, r.height = imgs[k].data_ptr(), W, H
        r.fx, r.fy, r.cx, r.cy = float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])
        r.cam_from_world[:], r.world_from_cam[:] = c["A"].reshape(-1).tolist(), c["B"].reshape(-1).tolist()
        r.min_depth, r.max_depth = float(c["min_depth"]), float(c["max_depth"])
    tsdf, weight = torch.zeros(nodes, device="cuda"), torch.zeros(nodes, device="cuda")
    occ = torch.zeros(nodes, dtype=torch.uint8, device="cuda")
    sdf, grad = torch.empty(nodes, device="cuda"), torch.empty(4 * nodes, device="cuda")
    n3, o3 = (C.c_int * 3)(*shape_xyz), (C.c_float * 3)(*[float(v) for v in origin])
    ws_bytes = lib.mpdx_sdf_grid_edt_ws_bytes(C.byref(n3))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device="cuda")
    st = _lib.current_stream()

    def integrate(n_cams):
        _lib.check(lib.mpdx_tsdf_integrate(rec, n_cams, None, 0, tsdf.data_ptr(), weight.data_ptr(), occ.data_ptr(), C.byref(n3), C.byref(o3), cell,
                                           trunc, max_weight, st), "mpdx_tsdf_integrate")

    def edt(with_grad=False):   # (the gradient plane: GridSDF mode 'nearest'; profiles/edt_probe.md times that form)
        _lib.check(lib.mpdx_sdf_grid_from_occupancy(occ.data_ptr(), sdf.data_ptr(), grad.data_ptr() if with_grad else None, None, C.byref(n3), cell,
                                                    0.0, ws.data_ptr(), ws_bytes, st))

    # ---- correctness at this size, before timing: one frame from an empty map, bit for bit against the reference
    integrate(1)
    torch.cuda.synchronize()
    z = np.zeros(shape, np.float32)
    t0 = time.perf_counter()
    want = R.integrate_ref(z, z, cams[:1], shape, origin, cell, trunc, max_weight)
    ref_s = time.perf_counter() - t0
    got = [tsdf.cpu().numpy().reshape(shape), weight.cpu().numpy().reshape(shape), occ.cpu().numpy().reshape(shape)]
    equal = all(np.array_equal(g, w) for g, w in zip(got, want))
    observed, occupied = int((want[1] > 0).sum()), int(want[2].sum())
    t0 = time.perf_counter()
    R.integrate_ref(z, z, cams, shape, origin, cell, trunc, max_weight)
    ref4_s = time.perf_counter() - t0
    # ---- timing
    variants = {"integrate 1 frame": lambda: integrate(1), "integrate 4 frames (one call)": lambda: integrate(4),
                "integrate 1 frame + transform": lambda: (integrate(1), edt()), "integrate 4 frames + transform": lambda: (integrate(4), edt()),
                "transform alone (sdf plane)": edt, "transform alone (sdf + gradient planes)": lambda: edt(True)}
    reps = {}
    for name, fn in variants.items():
        timed(fn, 5)
        reps[name] = int(min(20000, max(10, a.window * 1e6 / max(timed(fn, 10), 1e-3))))
    times = {k: [] for k in variants}
    for rnd in range(a.rounds + 1):
        for name, fn in variants.items():
            us = timed(fn, reps[name])
            if rnd:
                times[name].append(us)
    res = {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "reps": reps[k]} for k, v in times.items()}
    info = {"device": torch.cuda.get_device_name(0), "nodes_xyz": list(shape_xyz), "nodes": nodes, "cell": cell, "trunc": trunc, "frame": [W, H],
            "bit_equal_to_reference": equal, "observed_nodes_1_frame": observed, "occupied_nodes_1_frame": occupied,
            "reference_cpu_s": {"1 frame": round(ref_s, 2), "4 frames": round(ref4_s, 2)}, "us_per_call": res, "rounds": a.rounds}
    lines = ["# Depth-camera fusion: mpdx_tsdf_integrate on the Panda workspace", "",
             "Written by `tools/tsdf_probe.py` (hipEvent timing; per variant the median, min and max over "
             f"{a.rounds} rounds of back-to-back calls, variants alternating within each round).", "",
             f"- device: {info['device']}", f"- grid: {shape_xyz[0]} x {shape_xyz[1]} x {shape_xyz[2]} = {nodes} nodes at {cell} m, trunc {trunc} m, "
             f"max_weight {max_weight}", f"- frames: {W} x {H}, four cameras around the workspace (ray-cast fixed spheres of EnvSpheres3D and a floor)",
             f"- one frame from an empty map: {observed} nodes observed, {occupied} occupied; device planes bit-equal to tests/tsdf_ref.py: {equal}", "",
             "| variant | median us | min | max | reps |", "|---|---|---|---|---|"]
    for k, v in res.items():
        lines.append(f"| {k} | {v['median']} | {v['min']} | {v['max']} | {v['reps']} |")
    lines += ["", f"tests/tsdf_ref.py (numpy, this host's CPU, for context only): {ref_s:.2f} s for one frame, {ref4_s:.2f} s for four.", "",
              "```json", json.dumps(info), "```", ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines))
    print(json.dumps(info))


if __name__ == "__main__":
    main()
