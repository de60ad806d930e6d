#!/usr/bin/env python3
"""Measurements behind the scene batches (several obstacle scenes in one launch; csrc/scene_table.hpp) -> profiles/scene_batch_probe.md.  Needs a GPU.

  (a) register / scratch / occupancy table of k_guide.hip, parent against this tree: two outputs of tools/resource_usage.sh k_guide (CPU only, made
      beforehand) given with --resource-parent / --resource-child; the single-scene instantiations are expected to be identical.
  (b) single-scene guide launch time, parent library against this tree's, INTERLEAVED in one process: both libraries are loaded side by side
      (--parent-lib: a libmpdx.so built from the parent commit) and mpdx_guide_time is called parent, child, parent, child ... on the same
      buffers.  The parent is measured twice per round (slots A and B), so the probe shows the run-to-run spread of the parent against ITSELF:
      that spread is the margin the child is read against.  Point mass B = 100, Panda B = 100, Panda B = 6400.
  (c) S = 4 and S = 16 scenes x 100 trajectories in ONE guided plan against S separate guided single-scene plans (cfg3 / cfg4 shapes of bench.py).

  python tools/scene_batch_probe.py --parent-lib build_ab/libmpdx_parent.so --resource-parent a.txt --resource-child b.txt --out profiles/scene_batch_probe.md
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]


def bind(path):
    from mpd_public_amd import _lib
    lib = C.CDLL(str(path))
    for name in ("mpdx_guide_time", "mpdx_absmax", "mpdx_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def resource_rows(path):
    """tools/resource_usage.sh lines -> {kernel: 'VGPR / SGPR / scratch / occupancy'}"""
    import re
    rows = {}
    for ln in Path(path).read_text().splitlines():
        m = re.match(r"(?:void )?(mpdx::\S.*?)\s+vgpr\s+(\d+) agpr\s+\d+ spill\s+\S+ scratch\s+(\d+) sgpr\s+(\d+) occ (\d+) lds (\d+)", ln)
        if m:
            rows[m.group(1).strip()] = f"{m.group(2)} / {m.group(4)} / {m.group(3)} / {m.group(5)}"
    return rows


def guide_time_ab(parent, child, rounds, reps):
    import torch
    import bench
    from mpd_public_amd import synthetic as syn
    out = []
    for label, env_id, robot, B in (("point mass, B = 100", "EnvNarrowPassageDense2D", "RobotPointMass", 100), ("Panda, B = 100", "EnvSpheres3D", "RobotPanda", 100),
                                    ("Panda, B = 6400", "EnvSpheres3D", "RobotPanda", 6400)):
        g = bench.build_guide(env_id, robot, 100, "cuda")["guide"]
        D = g.dataset.state_dim
        gp = g.device_params(torch.device("cuda"))
        x = (0.9 * torch.from_numpy(syn.synth_tensor(f"scene_probe_x/{label}", (B, 64, D), "uniform"))).cuda().contiguous()
        grad = torch.empty_like(x)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        assert child.mpdx_absmax(x.data_ptr(), flag.data_ptr(), B, B, 64, D, st) == 0
        torch.cuda.synchronize()

        def one(lib):
            ms = C.c_float()
            rc = lib.mpdx_guide_time(C.byref(gp), x.data_ptr(), grad.data_ptr(), flag.data_ptr(), B, B, 64, D, reps, st, C.byref(ms))
            if rc:
                raise RuntimeError(f"mpdx_guide_time failed ({rc}): {lib.mpdx_last_error()}")
            return ms.value * 1e3
        one(parent)                       # (warm-up of both libraries, and: same bits from both on this input)
        torch.cuda.synchronize()
        ref = grad.clone()
        grad.zero_()
        one(child)
        torch.cuda.synchronize()
        same = bool(torch.equal(ref, grad))
        slots = {"parent_A": [], "child": [], "parent_B": []}
        for _ in range(rounds):
            slots["parent_A"].append(one(parent))
            slots["child"].append(one(child))
            slots["parent_B"].append(one(parent))
        med = {k: statistics.median(v) for k, v in slots.items()}
        out.append({"case": label, "reps_per_call": reps, "rounds": rounds, "us_per_launch_median": {k: round(v, 3) for k, v in med.items()},
                    "us_per_launch_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in slots.items()},
                    "parent_vs_itself_us": round(abs(med["parent_A"] - med["parent_B"]), 3),
                    "parent_round_to_round_us": round(max(max(slots["parent_A"]) - min(slots["parent_A"]), max(slots["parent_B"]) - min(slots["parent_B"])), 3),
                    "child_minus_parent_us": round(med["child"] - 0.5 * (med["parent_A"] + med["parent_B"]), 3), "outputs_bit_identical": same})
        print(json.dumps(out[-1]), flush=True)
    return out


def probe_scenes(dim, n):
    """n formula-defined extra-object sets (2 ... 6 spheres, 0 ... 2 boxes) of a dim-D workspace"""
    import numpy as np
    from mpd_public_amd import synthetic as syn
    from mpd_public_amd.planning import ObjectSet
    sets = []
    for s in range(n):
        ns, nb = 2 + s % 5, s % 3
        lo, hi = (-0.6, 0.6) if dim == 3 else (-0.8, 0.8)
        c = syn.hash_uniform(f"scene_probe/{dim}/{s}/c", (ns + nb) * dim, lo, hi).reshape(ns + nb, dim).astype(np.float32)
        if dim == 3:
            c[:, 2] = 0.3 + 0.5 * (c[:, 2] - lo) / (hi - lo)
        c3 = np.concatenate([c, np.zeros((ns + nb, 3 - dim), np.float32)], 1)
        r = syn.hash_uniform(f"scene_probe/{dim}/{s}/r", ns, 0.08, 0.15).astype(np.float32)
        half = np.concatenate([np.full((nb, dim), 0.08, np.float32), np.full((nb, 3 - dim), 1.0, np.float32)], 1)
        sets.append(ObjectSet(c3[:ns], r, c3[ns:], half))
    return sets


def scene_plans(plans):
    import copy
    import torch
    import bench
    import mpd_public_amd as m
    from mpd_public_amd import synthetic as syn
    from mpd_public_amd.parallel import expand_contexts, plan_contexts
    out = []
    n = 100
    for cfg in ("cfg3", "cfg4"):
        env_id, robot, D, mults, T, _, n0, _, _ = bench.CONFIGS[cfg]
        dm, _ = bench.build_model(D, mults, T, "cuda")
        dm.manual_seed(30)
        gk = bench.build_guide(env_id, robot, T, "cuda")
        g = gk.pop("guide")
        ds = g.dataset
        for S in (4, 16):
            scenes = m.PlanningScenes(ds.task, probe_scenes(ds.env.dim, S))
            st = torch.from_numpy(syn.synth_tensor("mc_s", (S, D), "uniform", 0.6)).cuda()
            gl = torch.from_numpy(syn.synth_tensor("mc_g", (S, D), "uniform", 0.6)).cuda()
            singles = []
            for s in range(S):    # the same guide against scene s alone
                d1 = copy.copy(ds)
                d1.task = scenes.scene_task(s)
                cl = [m.CostCollision(ds.robot, 64, field=f, sigma_coll=1.0) for f in d1.task.get_collision_fields()] + [g.cost.cost_l[-1]]
                singles.append(m.GuideManagerTrajectoriesWithVelocity(d1, m.CostComposite(ds.robot, 64, cl, weights_cost_l=g.cost.weight_cost_l), clip_grad=True,
                                                                      interpolate_trajectories_for_collision=True).cuda())
            kw = dict(n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda t: 0.5, **gk)

            def batched():
                return plan_contexts(dm, st, gl, n, horizon=64, guide=g, scenes=scenes, scene_of_context=list(range(S)), **kw)[0]

            def separate():
                return [dm.plan({0: st[s], 63: gl[s]}, n, 64, return_chain=False, guide=singles[s], **kw)[0] for s in range(S)]

            def same_scene():     # the same-scene bound: S contexts, one scene (today's multi-context plan)
                hs, hg = expand_contexts(st, gl, n)
                return dm.plan({0: hs, 63: hg}, S * n, 64, return_chain=False, guide=g, n_per_context=n, **kw)[0]
            rec = {"cfg": cfg, "robot": robot, "scenes": S, "trajectories_per_scene": n, "T": T, "n_without_noise": n0, "plans_timed": plans}
            for name, fn in (("one_plan_S_scenes", batched), ("S_separate_plans", separate), ("one_plan_same_scene", same_scene)):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(plans):
                    fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / plans
                rec[name] = {"ms": round(dt * 1e3, 2), "ms_per_context": round(dt * 1e3 / S, 2)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
    return out


def markdown(res, rp, rc):
    L = ["# Scene batches: resource usage, single-scene guide time, S scenes in one plan", "",
         "Produced by `tools/scene_batch_probe.py` (the JSON next to this file holds every figure).  Several obstacle scenes in one launch are the template",
         "parameter `MULTI_SCENE` of the guide / metrics kernels (`csrc/guide.hpp`, `csrc/scene_table.hpp`), chosen by the launcher when `n_scenes > 1`.", ""]
    if rp and rc:
        L += ["## (a) `k_guide.hip`: VGPR / SGPR / scratch B / occupancy (`tools/resource_usage.sh k_guide`, parent commit against this tree)", "",
              "| kernel (parent's template arguments) | parent | this tree, `MULTI_SCENE = false` | this tree, `MULTI_SCENE = true` |", "|---|---|---|---|"]
        same = True
        for k, v in rp.items():
            ks = k[:-1] + ", false>" if k.endswith(">") else k
            km = k[:-1] + ", true>" if k.endswith(">") else None
            cs = rc.get(ks, rc.get(k, "-"))
            same &= cs == v
            L.append(f"| `{k}` | {v} | {cs} | {rc.get(km, '-') if km else '-'} |")
        L += ["", f"Every single-scene figure equals the parent's: **{same}**.  No kernel has scratch; static LDS is 0 everywhere (all LDS is dynamic, sized by the launcher:",
              "a scene batch stages one scene block + the shared tail where a single scene stages its whole table).", ""]
    if res.get("guide_time"):
        L += ["## (b) single-scene guide launch, parent library against this tree's, interleaved in one process (`mpdx_guide_time`)", "",
              "Per round: parent (slot A), child, parent (slot B); medians over the rounds, us per launch.  `parent vs itself` = |median A - median B|, the margin;",
              "`round to round` = the largest max - min of a parent slot.", "",
              "| case | parent A | child | parent B | parent vs itself | round to round | child - parent mean | inside the margin | same bits |", "|---|---|---|---|---|---|---|---|---|"]
        for r in res["guide_time"]:
            m_ = r["us_per_launch_median"]
            L.append(f"| {r['case']} ({r['rounds']} x {r['reps_per_call']} launches) | {m_['parent_A']} | {m_['child']} | {m_['parent_B']} | {r['parent_vs_itself_us']} | "
                     f"{r['parent_round_to_round_us']} | {r['child_minus_parent_us']:+} | {abs(r['child_minus_parent_us']) <= r['parent_vs_itself_us']} | {r['outputs_bit_identical']} |")
        L.append("")
    if res.get("scene_plans"):
        L += ["## (c) S scenes x 100 trajectories in one guided plan against S separate guided plans (ms per context; no pass mark)", "",
              "`same scene` is the bound: the same S contexts in one plan with ONE scene (the multi-context plan as it was).", "",
              "| shape | S | one plan, S scenes | S separate plans | one plan, same scene |", "|---|---|---|---|---|"]
        for r in res["scene_plans"]:
            L.append(f"| {r['cfg']} ({r['robot']}, T = {r['T']} + {r['n_without_noise']}) | {r['scenes']} | {r['one_plan_S_scenes']['ms_per_context']} ({r['one_plan_S_scenes']['ms']} ms per plan) | "
                     f"{r['S_separate_plans']['ms_per_context']} ({r['S_separate_plans']['ms']} ms in all) | {r['one_plan_same_scene']['ms_per_context']} |")
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libmpdx.so built from the parent commit (part b)")
    ap.add_argument("--resource-parent")
    ap.add_argument("--resource-child")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--plans", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scene_batch_probe.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scene_batch_probe needs a GPU (parts b and c are measurements)")
    from mpd_public_amd import _lib
    res = {}
    if a.parent_lib:
        res["guide_time"] = guide_time_ab(bind(a.parent_lib), bind(_lib.lib_path()), a.rounds, a.reps)
    res["scene_plans"] = scene_plans(a.plans)
    rp = resource_rows(a.resource_parent) if a.resource_parent else None
    rc = resource_rows(a.resource_child) if a.resource_child else None
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(markdown(res, rp, rc) + "\n")
    out.with_suffix(".json").write_text(json.dumps(res, indent=1) + "\n")
    print(out)


if __name__ == "__main__":
    main()
