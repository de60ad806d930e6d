#!/usr/bin/env python3
"""Time the mesh producer (mpdx_sdf_grid_from_mesh, sdf plane only) on the device; needs a GPU, one process, one device.

  python tools/mesh_probe.py [--rounds 5] [--window 0.3] [--ab name=build_ab/libmpdx_<tag>.so ...] [--ab-faces 5120]

The grid is the Panda's workspace at 2 cm (grid_sdf.grid_spec_for: 132 x 132 x 112 nodes); the meshes are icospheres of 1 280, 5 120 and 20 480 faces
inside it, in both sign modes.  Per case and variant: `reps` calls back to back between ONE event pair after warm-up calls, reps chosen so that a
window lasts about --window seconds; the variants alternate within each of `rounds` rounds; median, min and max over the rounds (the protocol of
tools/edt_probe.py).  --ab adds libraries built with other MPDX_MESH_NPT / MPDX_MESH_TILE (MPDX_BUILD_DEFS) as variants of the --ab-faces case: they
are loaded next to the shipped one and called through the same binding.  Before anything is timed the device result is compared with the sphere the
mesh approximates (distance within the faces' sagitta, sign by the radius).  Prints one JSON line (us per call, node-face pairs per second)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mpd_public_amd as m  # noqa: E402
from mpd_public_amd import _lib  # noqa: E402
from mpd_public_amd.planning import grid_spec_for  # noqa: E402
import mesh_ref  # noqa: E402  (the icosphere)

CENTRE, RADIUS, CELL = (0.3, 0.0, 0.5), 0.25, 0.02
NAME = "mpdx_sdf_grid_from_mesh"
LAUNCH_PAIRS = 1 << 33      # the host's cap per launch (csrc/k_grid.hip)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def entry(path):
    """the mesh entry point of another build of the library, bound like the shipped one"""
    fn = getattr(C.CDLL(str(path), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND), NAME)   # its own kernels, not the shipped library's of the same names
    fn.restype, fn.argtypes = _lib.SIGNATURES[NAME]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--ab", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--ab-faces", type=int, default=5120)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_probe needs a GPU (nothing is measured without one)")
    libs = {"shipped": getattr(_lib.load(), NAME)}
    for spec in a.ab:
        name, path = spec.split("=", 1)
        libs[name] = entry(ROOT / path)
    env = m.make_env("EnvSpheres3D")
    shape, origin = grid_spec_for(env.limits[0], env.limits[1], CELL)
    nodes = int(np.prod(shape))
    n3, o3 = (C.c_int * 3)(*shape), (C.c_float * 3)(*[float(v) for v in origin])
    sdf = torch.empty(nodes, device="cuda")
    st = _lib.current_stream()
    P = torch.from_numpy(mesh_ref.nodes(shape, origin, CELL).reshape(-1, 3)).cuda()
    rad = torch.linalg.norm(P - torch.tensor(CENTRE, dtype=torch.float64, device="cuda"), dim=1)
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_s": a.window, "grid": {"nodes": list(shape), "cell": CELL}, "cases": {}}
    for sub in (3, 4, 5):
        V, F = mesh_ref.icosphere(sub, RADIUS, CENTRE)
        nf = int(F.shape[0])
        v, f = torch.from_numpy(V.astype(np.float32)).cuda(), torch.from_numpy(F).cuda()
        tri = V[F] - np.asarray(CENTRE)
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        sag = RADIUS - float((np.abs((tri[:, 0] * nrm).sum(1)) / np.linalg.norm(nrm, axis=1)).min())

        def call(fn, mode):
            rc = fn(v.data_ptr(), v.shape[0], f.data_ptr(), nf, sdf.data_ptr(), None, None, C.byref(n3), C.byref(o3), CELL, 0.0, mode, st)
            if rc != 0:
                raise RuntimeError(f"{NAME} failed (code {rc})")

        variants = {}
        for mode_name, mode in (("winding", _lib.MESH_SIGN_WINDING), ("none", _lib.MESH_SIGN_NONE)):
            for lib_name, fn in libs.items():
                if lib_name != "shipped" and nf != a.ab_faces:
                    continue
                # ---- correctness at this size, before timing: the sphere the mesh approximates
                sdf.fill_(float("nan"))
                call(fn, mode)
                torch.cuda.synchronize()
                want = (rad - RADIUS) if mode == _lib.MESH_SIGN_WINDING else (rad - RADIUS).abs()
                err = float((sdf.double() - want).abs().max())
                if not err <= sag + 1e-6:
                    raise SystemExit(f"{lib_name} {mode_name} F={nf}: max |s - sphere| = {err:.3e} exceeds the sagitta {sag:.3e}")
                variants[f"{mode_name}/{lib_name}"] = (lambda fn=fn, mode=mode: call(fn, mode))
        reps = {}
        for name, fn in variants.items():
            timed(fn, 2)
            reps[name] = int(min(2000, max(1, a.window * 1e6 / max(timed(fn, 2), 1e-3))))
        times = {k: [] for k in variants}
        for rnd in range(a.rounds + 1):   # round 0 warms every variant and is dropped
            for name, fn in variants.items():
                us = timed(fn, reps[name])
                if rnd:
                    times[name].append(us)
        pairs = nodes * nf
        launches = -(-nodes // max(1024, LAUNCH_PAIRS // nf // 1024 * 1024))
        res = {"faces": nf, "pairs": pairs, "launches_per_call": launches, "sagitta": sag, "us_per_call": {}}
        for k, t in times.items():
            med = statistics.median(t)
            res["us_per_call"][k] = {"median": round(med, 1), "min": round(min(t), 1), "max": round(max(t), 1), "reps": reps[k],
                                     "pairs_per_s": float(f"{pairs / (med * 1e-6):.4g}"), "us_per_full_launch": round(med * min(1.0, LAUNCH_PAIRS / pairs), 1)}
        out["cases"][f"icosphere_{nf}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
