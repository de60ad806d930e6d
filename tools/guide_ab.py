#!/usr/bin/env python3
"""Bit-for-bit A/B of the guide, metrics and baseline-planner kernels between two builds of the library (dev tool, needs a GPU):

   MPDX_LIB=<other build> python tools/guide_ab.py save <file>      - run the matrix below on one build and keep every output tensor
   python tools/guide_ab.py cmp <file>                              - run it on this build and compare: every tensor must be torch.equal
   [MPDX_LIB=<lib>] python tools/guide_ab.py                         - the Panda guide's time per launch at B = 100 / 6400 alone

The matrix (small shapes: B = 6 in two contexts of 3, context 1 outside +-1 so that its range test fires; H in {8, 72}; interpolation off and
n_interp = 2 H + 1): point mass 2-D and 3-D, the Panda, the Panda as a chain and a 3-joint chain with a prismatic joint, each with one scene and with
two, the built-in robots also with a grid field; the guide in gradient-only and in apply mode, the metrics with their mask; one GPMP2 step and one
RRT-Connect + paths call per built-in robot; a guided plan of the cfg 3 and cfg 4 shapes with B = 8 and the step's noise drawn in place.
MPDX_GUIDE_DENSE=1 in the environment: the Panda guide cases alone, through the dense variant (the switch is read once per process)."""
import ctypes as C, os, sys
from math import ceil
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch
import mpd_public_amd as m
from mpd_public_amd import _lib
from mpd_public_amd.generate_trajectories import GPMP2, RRTConnectBatch
from chain_ref import chain_trajs, product_robot
from helpers import product_guide, obstacle_hugging_trajs, t
from scene_ref import scene_object_sets

mode = sys.argv[1] if len(sys.argv) > 1 else ""
TA = {"device": "cuda", "dtype": torch.float32}
DENSE = os.environ.get("MPDX_GUIDE_DENSE", "") == "1"
NPC, B = 3, 6
lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream
out = {}


def timed_panda():
    ds = m.TrajectoryDataset("EnvSpheres3D", "RobotPanda", tensor_args=TA)
    for Bt in (100, 6400):
        x = obstacle_hugging_trajs(ds, Bt, seed="trace", scale=0.95).cuda()
        pg = product_guide(ds).cuda()
        gp = pg.device_params(x.device)
        flag = torch.zeros(max(1, Bt // 50), dtype=torch.int32, device="cuda")
        g = torch.zeros_like(x)
        ms = C.c_float(0)
        best = 1e9
        for rep in range(3):
            _lib.check(lib.mpdx_guide_time(C.byref(gp), x.data_ptr(), g.data_ptr(), flag.data_ptr(), 50, Bt, 64, ds.state_dim, 50, st, C.byref(ms)))
            best = min(best, ms.value)
        out[f"timed/panda/B{Bt}"] = g.cpu()
        print(f"{_lib.lib_path().name}: Panda guide B={Bt}: {best * 1e3:.1f} us per launch", flush=True)


def make_guide(ds, H, interp):
    costs = [m.CostCollision(ds.robot, H, field=f, sigma_coll=1.0) for f in ds.task.get_collision_fields()]
    weights = [1e-2] * len(costs)
    costs.append(m.CostGPTrajectory(ds.robot, H, 5.0 / H, sigma_gp=1.0))
    weights.append(1e-7)
    return m.GuideManagerTrajectoriesWithVelocity(ds, m.CostComposite(ds.robot, H, costs, weights_cost_l=weights), clip_grad=True,
                                                  interpolate_trajectories_for_collision=interp, num_interpolated_points_for_collision=2 * H + 1)


ROBOTS = [("pm2", "EnvDense2D", "RobotPointMass", True), ("pm3", "EnvSpheres3D", "RobotPointMass3D", True), ("panda", "EnvSpheres3D", "RobotPanda", True),
          ("panda_chain", "EnvSpheres3D", "chain:Panda", False), ("r3_chain", "EnvSpheres3D", "chain:R3", False)]


def guide_and_metrics():
    for tag, env_id, robot_id, builtin in ROBOTS:
        if DENSE and tag != "panda":
            continue
        robot = product_robot(robot_id[6:]) if robot_id.startswith("chain:") else robot_id
        for H in (8, 72):
            for grid in ((False, True) if builtin else (False,)):
                ds = m.TrajectoryDataset(env_id, robot, n_support_points=H, tensor_args=TA)
                if grid:
                    ds.task = m.PlanningTask(ds.env, ds.robot, obstacle_cutoff_margin=ds.task.obstacle_cutoff_margin, sdf_grid=dict(cell_size=0.05))
                D = ds.state_dim
                x = chain_trajs(D // 2, B, H, f"guide_ab/{tag}/{H}")
                x[NPC:] *= 1.12
                x = x.cuda()
                hs, hg = t(f"guide_ab/hs/{tag}", (B, D), "uniform").cuda(), t(f"guide_ab/hg/{tag}", (B, D), "uniform").cuda()
                flag_in = torch.zeros(B // NPC, dtype=torch.int32, device="cuda")
                _lib.check(lib.mpdx_absmax(x.data_ptr(), flag_in.data_ptr(), NPC, B, H, D, st))
                scenes = m.PlanningScenes(ds.task, scene_object_sets(ds.env.dim)[1:])
                for multi in (False, True):
                    key = f"{'dense/' if DENSE else ''}{tag}/H{H}/{'grid' if grid else 'prims'}/{'2scenes' if multi else '1scene'}"
                    for interp in (False, True):
                        pg = make_guide(ds, H, interp)
                        pg = (pg.with_scenes(scenes, [1, 0], NPC) if multi else pg).cuda()
                        gp = pg.device_params(x.device)
                        g = torch.zeros_like(x)
                        _lib.check(lib.mpdx_guide_step(C.byref(gp), x.data_ptr(), g.data_ptr(), None, None, flag_in.data_ptr(), None, NPC, B, H, D, st))
                        y, flag_out = x.clone(), torch.zeros_like(flag_in)
                        _lib.check(lib.mpdx_guide_step(C.byref(gp), y.data_ptr(), None, hs.data_ptr(), hg.data_ptr(), flag_in.data_ptr(), flag_out.data_ptr(), NPC, B, H, D, st))
                        k = f"{key}/{'interp' if interp else 'nointerp'}"
                        out[k + "/grad"], out[k + "/applied"], out[k + "/absmax"] = g.cpu(), y.cpu(), flag_out.cpu()
                        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
                    if DENSE:
                        continue
                    xu = ds.unnormalize_trajectories(x)
                    n_check = 2 * H + 1
                    if multi:
                        o4, mask = scenes.trajectory_metrics(xu, [1, 0], NPC, n_check=n_check, return_mask=True)
                    else:
                        o4, mask = ds.task.trajectory_metrics(xu, n_check=n_check, return_mask=True)
                    out[key + "/metrics"], out[key + "/mask"] = o4.cpu(), mask.cpu()
        print(f"guide + metrics: {tag} done", flush=True)


def planners():
    for tag, env_id, robot_id, _ in ROBOTS[:3]:
        ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
        q = ds.state_dim // 2
        gen = torch.Generator(device="cuda").manual_seed(11)
        qs = ds.task.random_coll_free_q(n_samples=2, device="cuda", generator=gen)
        rrt = RRTConnectBatch(ds.task, qs[0], qs[1], 4, max_nodes=256, generator=torch.Generator(device="cuda").manual_seed(5))
        rrt.grow(max_iters=300)
        trajs, plen = rrt.trajectories(64, 5.0 / 64, return_path_len=True)
        for name, v in (("nodes", rrt.nodes), ("parent", rrt.parent), ("count", rrt.count), ("link", rrt.link), ("iters", rrt.iters), ("trajs", trajs), ("path_len", plen)):
            out[f"rrt/{tag}/{name}"] = v.cpu()
        gp2 = GPMP2(ds, 5.0 / 64)
        out[f"gpmp/{tag}/x"] = gp2.optimize(trajs, opt_iters=1).cpu()
        out[f"gpmp/{tag}/state"] = gp2.state.cpu()
        assert q == trajs.shape[-1] // 2
        print(f"planners: {tag} done ({int(rrt.done.sum())} of 4 searches connected)", flush=True)


def guided_plans():
    from mpd_public_amd import synthetic as syn
    for cfg, env_id, robot_id, D in (("cfg3", "EnvNarrowPassageDense2D", "RobotPointMass", 4), ("cfg4", "EnvSpheres3D", "RobotPanda", 14)):
        T, n0 = 100, 5
        net = m.TemporalUnet(n_support_points=64, state_dim=D, unet_input_dim=32, dim_mults=(1, 2, 4, 8))
        net.load_state_dict(syn.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
        dm = m.GaussianDiffusionModel(model=net, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True).cuda().eval()
        dm.manual_seed(30)
        ds = m.TrajectoryDataset(env_id, robot_id, tensor_args=TA)
        hc = {0: torch.from_numpy(syn.synth_tensor("bench_hc0", (D,), "uniform", 0.6)).cuda(), 63: torch.from_numpy(syn.synth_tensor("bench_hc1", (D,), "uniform", 0.6)).cuda()}
        chain = dm.run_inference(None, hc, n_samples=8, horizon=64, return_chain=True, n_diffusion_steps_without_noise=n0, noise_std_extra_schedule_fn=lambda tt: 0.5,
                                 guide=product_guide(ds).cuda(), n_guide_steps=5, t_start_guide=ceil(0.25 * T))
        out[f"plan/{cfg}/chain"] = chain.cpu()
        print(f"guided plan: {cfg} done, chain {tuple(chain.shape)}", flush=True)


if mode not in ("save", "cmp"):
    timed_panda()
    sys.exit(0)
print(f"library: {_lib.lib_path()}{'  (MPDX_GUIDE_DENSE=1: Panda guide cases only)' if DENSE else ''}", flush=True)
guide_and_metrics()
if not DENSE:
    timed_panda()
    planners()
    guided_plans()
if mode == "save":
    torch.save(out, sys.argv[2])
    print(f"saved {len(out)} tensors to {sys.argv[2]}")
else:
    ref = torch.load(sys.argv[2])
    assert sorted(ref) == sorted(out), "the two runs produced different sets of tensors"
    bad = [k for k in out if not (out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]))]
    groups = {}
    for k in out:
        g = "/".join(k.split("/")[:2 if k.split("/")[0] == "dense" else 1])
        groups.setdefault(g, [0, 0])
        groups[g][0] += 1
        groups[g][1] += k in bad
    for g, (n, nb) in groups.items():
        print(f"  {g:14s} {n:4d} tensors, {n - nb:4d} bit-identical")
    for k in bad:
        print(f"  DIFFERS {k}: max|this - other| = {(out[k].double() - ref[k].double()).abs().max().item():.3e}")
    print(f"{len(out) - len(bad)} of {len(out)} tensors bit-identical to {sys.argv[2]}")
    sys.exit(1 if bad else 0)
