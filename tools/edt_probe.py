#!/usr/bin/env python3
"""Time the occupancy transform (mpdx_sdf_grid_from_occupancy, sdf plane + gradient plane) on the device, next to scipy's exact transform of the same
occupancy on this host's CPU and to the primitive bake (mpdx_sdf_grid_bake, both planes) of the same environment; needs a GPU, one process, one device.

  python tools/edt_probe.py [--rounds 5] [--window 0.3]

Workspaces: the 2-D one at 1 cm (EnvSimple2D / point mass) and the Panda's at 2 cm (EnvSpheres3D), on the grid box of grid_sdf.grid_spec_for.  The
occupancy is (primitive sdf at the node <= 0), taken from the device bake.  Per workspace and variant: `reps` calls back to back between ONE event
pair after warm-up calls, reps chosen so that a window lasts about --window seconds; the variants alternate within each of `rounds` rounds; median,
min and max over the rounds.  The device d2 plane is compared with scipy's (rint of the squared distances) before anything is timed.  Prints one
JSON line (us per call)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mpd_public_amd as m  # noqa: E402
from mpd_public_amd import _lib  # noqa: E402

SHAPES = [("ws2d_1cm", "EnvSimple2D", "RobotPointMass", 0.01), ("panda_2cm", "EnvSpheres3D", "RobotPanda", 0.02)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edt_probe needs a GPU (nothing is measured without one)")
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    ta = {"device": "cuda", "dtype": torch.float32}
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_s": a.window, "us_per_call": {}, "grid": {}}
    for tag, env_id, robot_id, cell in SHAPES:
        ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=ta, sdf_grid=dict(cell_size=cell, mode="nearest"))
        baked = ds.task.df_collision_objects.grid
        sdf_b, _ = baked.node_values("cuda")
        occ = (sdf_b <= 0).to(torch.uint8).contiguous()
        dim, nodes = baked.dim, baked.n_nodes
        n3 = (C.c_int * 3)(*(list(baked.shape) + [1] * (3 - dim)))
        o3 = (C.c_float * 3)(*([float(v) for v in baked.origin] + [0.0] * (3 - dim)))
        sdf = torch.empty(nodes, device="cuda")
        grad = torch.empty(nodes * 4, device="cuda")
        d2 = torch.empty(nodes, dtype=torch.int32, device="cuda")
        ws_bytes = lib.mpdx_sdf_grid_edt_ws_bytes(C.byref(n3))
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device="cuda")
        st = _lib.current_stream()
        # the primitive bake's parameter block (as grid_sdf.GridSDF._bake builds it)
        gp = _lib.GuideParams()
        gp.ws_dim, gp.n_fields = dim, 1
        sp, bx = ds.env.obj_fixed.prim_floats()
        f = gp.fields[0]
        f.kind, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 0, sp.size // 4, sp.size, bx.size // 6
        prims = torch.from_numpy(np.concatenate([sp, bx, np.zeros(4, np.float32)]).astype(np.float32)).cuda()
        gp.prims, gp.n_prim_floats = prims.data_ptr(), sp.size + bx.size

        def edt(d2_ptr=None):
            _lib.check(lib.mpdx_sdf_grid_from_occupancy(occ.data_ptr(), sdf.data_ptr(), grad.data_ptr(), d2_ptr, C.byref(n3), cell, 0.0, ws.data_ptr(), ws_bytes, st))

        def bake():
            _lib.check(lib.mpdx_sdf_grid_bake(C.byref(gp), 0, sdf.data_ptr(), grad.data_ptr(), C.byref(n3), C.byref(o3), cell, st))

        # ---- correctness at this size, before timing: the device d2 against scipy's exact transform
        edt(d2.data_ptr())
        torch.cuda.synchronize()
        occ_h = occ.cpu().numpy().astype(bool)
        info = {"nodes": list(baked.shape), "cell": cell, "occupied": int(occ_h.sum()), "sdf_plane_bytes": nodes * 4, "workspace_bytes": int(ws_bytes)}
        cpu_us = None
        if ndi is not None:
            both = lambda: np.where(occ_h, ndi.distance_transform_edt(occ_h), ndi.distance_transform_edt(~occ_h))
            want = np.rint(both() ** 2).astype(np.int32)
            info["d2_equals_scipy"] = bool(np.array_equal(d2.cpu().numpy().reshape(occ_h.shape), want))
            info["max_d2"] = int(want.max())
            ts = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                both()
                ts.append((time.perf_counter() - t0) * 1e6)
            cpu_us = {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
        out["grid"][tag] = info
        # ---- timing
        variants = {"edt_sdf_and_gradient": edt, "primitive_bake_sdf_and_gradient": bake}
        reps = {}
        for name, fn in variants.items():
            timed(fn, 10)
            reps[name] = int(min(20000, max(20, a.window * 1e6 / max(timed(fn, 20), 1e-3))))
        times = {k: [] for k in variants}
        for rnd in range(a.rounds + 1):   # round 0 warms every variant and is dropped
            for name, fn in variants.items():
                us = timed(fn, reps[name])
                if rnd:
                    times[name].append(us)
        res = {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "reps": reps[k]} for k, v in times.items()}
        res["scipy_cpu_two_transforms"] = cpu_us if cpu_us is not None else "not measured (no scipy on this host)"
        out["us_per_call"][tag] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
