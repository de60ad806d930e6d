"""float64 restatement of rrt_connect_kernel, written from the contract in include/mpdx.h (mpdx_rrt_connect) and the algorithm
(Kuffner & LaValle 2000: two trees grown alternately, extend towards a sample, greedy connect of the other tree) - Python floats and
numpy float64, no product tensor code.  Collisions come in as `slack_fn(q[N, q_dim]) -> [N]` (max over every hinge of link radius
minus signed distance: a configuration collides iff its slack is positive; tests pass helpers.oracle_config_slack).

  sample `it` (1-based) of problem b   the uniforms of Philox counters (b << 32) | 2 it  and  (b << 32) | (2 it + 1), keyed by the seed;
                                       the first q_dim of the eight scale into [q_lo, q_hi]
  active tree                          it & 1 (tree 0 grows from the start, tree 1 from the goal); a full tree ends the search, and the
                                       iteration that finds it full counts in `iters`
  nearest                              smallest squared distance, lowest index wins ties
  steer                                by at most float32(step); reaches iff dist <= step, and then returns the target itself
  edge_free                            on n_edge_checks configurations (1 - w) qa + w qb, w = c / (n - 1), end points included
  iteration                            extend the active tree from its nearest node; if the edge is free insert the node, then walk the other
                                       tree from ITS nearest node towards the new node, for up to max_connect_steps free steps, inserting each;
                                       a step that reaches the new node links the trees (the node is not inserted twice) and ends the search

free_run() runs that loop on its own.  compare() replays it against recorded trees: it predicts every insertion, checks it, ADOPTS the
recorded float32 coordinates and goes on, so every later decision is judged on the device's own node values.  A decision the float64
values cannot settle for a float32 evaluation (AMBIGUOUS below) ends the comparison of that problem: what came before is verified, the
problem counts as cut short.

The FAULTS are deliberately wrong variants of free_run for tests/test_rrt_ref_cpu.py: compare() has to notice each of them."""
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

import philox_ref as pr

EDGE_EPS = 1e-5        # an edge whose largest slack over its check configurations lies within this of zero
NEAREST_REL = 1e-6     # a nearest query whose two smallest squared distances (of nodes with different coordinates) differ by no more, relatively
STEER_REL = 1e-6       # a steer with |dist - step| < STEER_REL * step
COORD_TOL = 2e-6       # inserted coordinates: |q| <= pi, a steer is a handful of float32 roundings of <= 2.4e-7 each

FAULTS = ("rounds9", "swap_counters", "nearest256", "tie_high", "dup_reached", "w_over_n")


@dataclass
class Problem:
    """one launch's parameters as the kernel receives them (limits and step rounded to float32, as the options struct holds them)"""
    start: np.ndarray              # [n, q] float32 values
    goal: np.ndarray               # [n, q]
    q_lo: np.ndarray               # [q]
    q_hi: np.ndarray               # [q]
    step: float
    max_nodes: int
    max_iters: int
    max_connect_steps: int
    n_edge_checks: int
    seed: int
    slack_fn: Callable

    def __post_init__(self):
        f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)   # noqa: E731
        self.start, self.goal = np.atleast_2d(f32(self.start)), np.atleast_2d(f32(self.goal))
        self.q_lo, self.q_hi, self.step = f32(self.q_lo), f32(self.q_hi), float(np.float32(self.step))
        self.seed = int(self.seed) & pr.MASK64


@dataclass
class Trees:
    """what RRTConnectBatch holds after grow(): numpy arrays"""
    nodes: np.ndarray              # [n, 2, M, q]
    parent: np.ndarray             # [n, 2, M]
    count: np.ndarray              # [n, 2]
    link: np.ndarray               # [n, 2]
    iters: np.ndarray              # [n]
    ambiguous: List[int] = field(default_factory=list)    # free_run: ambiguous decisions met per problem
    first_dirs: List[Optional[np.ndarray]] = field(default_factory=list)   # free_run: as Report.first_dirs


@dataclass
class Report:
    mismatches: List[str] = field(default_factory=list)           # empty: the recorded trees are the reference's trees
    cut_short: List[int] = field(default_factory=list)            # problems whose comparison ended at an ambiguous decision
    insertions: int = 0                                           # insertions verified
    edge_checks: int = 0
    first_dirs: List[Optional[np.ndarray]] = field(default_factory=list)   # per problem: unit direction root -> first sample (None: first extension not inserted)


class _Ambiguous(Exception):
    pass


class _Mismatch(Exception):
    pass


def sample(p: Problem, b: int, it: int, fault=None):
    rounds = 9 if fault == "rounds9" else 10
    c0, c1 = (b << 32) | (2 * it), (b << 32) | (2 * it + 1)
    if fault == "swap_counters":
        c0, c1 = c1, c0
    u = np.concatenate([pr.uniform4(p.seed, c0, rounds), pr.uniform4(p.seed, c1, rounds)])[: len(p.q_lo)]
    return p.q_lo + (p.q_hi - p.q_lo) * u


def _search(p: Problem, b: int, rec: Optional[Trees], fault, rep: Optional[Report]):
    """the loop of one problem; rec is None: free run, else teacher-forced replay against rec (raises _Mismatch / _Ambiguous).
    Returns (nodes [2, M, q], parent [2, M], count [2], link [2], iters, ambiguous decisions met, unit direction of the first extension or None)."""
    M, qd = p.max_nodes, len(p.q_lo)
    nodes, parent, count = np.zeros((2, M, qd)), np.full((2, M), -1, dtype=np.int64), [1, 1]
    nodes[0, 0], nodes[1, 0] = p.start[b], p.goal[b]
    link, used, n_amb, first_dir = [-1, -1], 0, 0, None
    if rec is not None:
        for t in (0, 1):
            if not np.array_equal(rec.nodes[b, t, 0].astype(np.float64), nodes[t, 0]) or int(rec.parent[b, t, 0]) != -1:
                raise _Mismatch(f"problem {b}: root of tree {t}")

    def ambiguous(what):
        nonlocal n_amb
        n_amb += 1
        if rec is not None:
            raise _Ambiguous(what)

    def nearest(t, target):
        n = count[t]
        if fault == "nearest256":
            n = min(n, 256)
        d2 = ((nodes[t, :n] - target) ** 2).sum(-1)
        order = np.argsort(d2, kind="stable")
        i0 = int(order[0])
        if n > 1:
            i1 = int(order[1])
            if d2[i1] - d2[i0] <= NEAREST_REL * d2[i1]:
                if not np.array_equal(nodes[t, i0], nodes[t, i1]):
                    ambiguous("nearest")
                elif fault == "tie_high":      # equal coordinates give equal distances in any arithmetic: the tie rule decides
                    i0 = int(np.flatnonzero(d2 == d2[i0]).max())
        return i0

    def steer(frm, to):
        dist = math.sqrt(float(((to - frm) ** 2).sum()))
        if abs(dist - p.step) < STEER_REL * p.step:
            ambiguous("steer")
        if dist <= p.step:
            return to.copy(), True
        return frm + (to - frm) * (p.step / max(dist, 1e-12)), False

    def edge_free(qa, qb):
        n = p.n_edge_checks
        w = (np.arange(n) / (n if fault == "w_over_n" else n - 1))[:, None]
        s = float(np.max(np.asarray(p.slack_fn((1.0 - w) * qa + w * qb), dtype=np.float64)))
        if rep is not None:
            rep.edge_checks += 1
        if abs(s) <= EDGE_EPS:
            ambiguous("edge")
        return s <= 0.0

    def add(t, q, par):
        idx = count[t]
        if rec is not None:
            if int(rec.count[b, t]) <= idx:
                raise _Mismatch(f"problem {b}: tree {t} ends at {int(rec.count[b, t])} nodes, the reference inserts node {idx} (iteration {used})")
            if int(rec.parent[b, t, idx]) != par:
                raise _Mismatch(f"problem {b}: tree {t} node {idx} has parent {int(rec.parent[b, t, idx])}, reference {par} (iteration {used})")
            got = rec.nodes[b, t, idx].astype(np.float64)
            err = float(np.abs(got - q).max())
            if not err <= COORD_TOL:
                raise _Mismatch(f"problem {b}: tree {t} node {idx} is {err:.3e} from the reference's (iteration {used})")
            q = got                               # adopt the recorded float32 coordinates
            rep.insertions += 1
        nodes[t, idx], parent[t, idx] = q, par
        count[t] = idx + 1
        return idx

    done = False
    for it in range(1, p.max_iters + 1):
        used = it
        ta, tb = it & 1, 1 - (it & 1)
        if count[0] >= M or count[1] >= M:
            break
        qr = sample(p, b, it, fault)
        ia = nearest(ta, qr)
        qn = nodes[ta, ia]
        qnew, _ = steer(qn, qr)
        if not edge_free(qn, qnew):
            continue
        inew = add(ta, qnew, ia)
        qnew = nodes[ta, inew]
        if it == 1:
            first_dir = (qr - qn) / np.linalg.norm(qr - qn)
            if rep is not None:
                rep.first_dirs[b] = first_dir
        cur = nearest(tb, qnew)
        for _ in range(p.max_connect_steps):
            qcur = nodes[tb, cur]
            nxt, reach = steer(qcur, qnew)
            if not edge_free(qcur, nxt):
                break
            if reach:
                if fault == "dup_reached" and count[tb] < M:
                    cur = add(tb, nxt, cur)
                link = [inew, cur] if ta == 0 else [cur, inew]
                done = True
                break
            if count[tb] >= M:
                break
            cur = add(tb, nxt, cur)
        if done:
            break
    return nodes, parent, count, link, used, n_amb, first_dir


def free_run(p: Problem, fault=None, problems=None) -> Trees:
    """the reference's own trees (`problems`: only these indices are searched, the others stay as initialised)"""
    n, M, qd = len(p.start), p.max_nodes, len(p.q_lo)
    assert fault is None or fault in FAULTS
    out = Trees(np.zeros((n, 2, M, qd), dtype=np.float32), np.full((n, 2, M), -1, dtype=np.int32), np.ones((n, 2), dtype=np.int32),
                np.full((n, 2), -1, dtype=np.int32), np.zeros(n, dtype=np.int32))
    for b in (range(n) if problems is None else problems):
        nodes, parent, count, link, used, n_amb, first_dir = _search(p, b, None, fault, None)
        out.nodes[b], out.parent[b], out.count[b], out.link[b], out.iters[b] = nodes, parent, count, link, used
        out.ambiguous.append(n_amb)
        out.first_dirs.append(first_dir)
    return out


def compare(rec: Trees, p: Problem, problems=None) -> Report:
    """teacher-forced replay of the recorded trees (`problems`: of these indices only); see the module docstring"""
    n, M = len(p.start), p.max_nodes
    rep = Report(first_dirs=[None] * n)
    if rec.nodes.shape != (n, 2, M, len(p.q_lo)) or rec.parent.shape != (n, 2, M):
        rep.mismatches.append(f"shapes {rec.nodes.shape} {rec.parent.shape}")
        return rep
    for b in (range(n) if problems is None else problems):
        try:
            _, _, count, link, used, _, _ = _search(p, b, rec, None, rep)
        except _Ambiguous:
            rep.cut_short.append(b)
            continue
        except _Mismatch as e:
            rep.mismatches.append(str(e))
            continue
        got = ([int(v) for v in rec.count[b]], [int(v) for v in rec.link[b]], int(rec.iters[b]))
        if got != (count, link, used):
            rep.mismatches.append(f"problem {b}: (count, link, iters) = {got}, reference {(count, link, used)}")
            continue
        for t in (0, 1):    # rows behind the count: as RRTConnectBatch initialised them
            if rec.nodes[b, t, count[t]:].any() or (rec.parent[b, t, count[t]:] != -1).any():
                rep.mismatches.append(f"problem {b}: tree {t} has rows written behind its {count[t]} nodes")
    return rep


def directions_span(dirs, rel=0.1):
    """Do the unit vectors `dirs` span k = min(len, q_dim) dimensions: is the k-th singular value of their matrix at least `rel` of the
    largest?  A sampler that leaves out a coordinate (or repeats one) puts every direction into a hyperplane (a line in the plane): the
    k-th value is then zero; from a corner of the box the directions fill a quadrant at best, which gives about 0.4."""
    d = np.stack(dirs)
    s = np.linalg.svd(d, compute_uv=False)
    return bool(s[min(d.shape) - 1] >= rel * s[0])


# ---------------------------------------------------------------------------------------------- the cases of the CPU and the GPU tests
# start / goal: fixed configurations whose float64 slack is below -0.02 (checked in tests/test_rrt_ref_cpu.py).  gen_seed is the torch generator's seed and
# `launch` the value RRTConnectBatch._launches has after grow(): the launch's seed is gen_seed * 1000003 + launch (mod 2^64).
_PM = dict(robot="RobotPointMass", max_nodes=2048, max_connect_steps=64, n_edge_checks=16)
CASES = {
    "dense": dict(_PM, env="EnvDense2D", n=8, step=0.1, max_iters=600, gen_seed=5, launch=3, start=(-0.9, 0.05), goal=(0.9, 0.1)),
    # trees beyond 256 nodes (the strided part of the nearest loop), solved problems and problems that stop at the iteration cap
    "narrow": dict(_PM, env="EnvNarrowPassageDense2D", n=8, step=0.05, max_iters=1500, gen_seed=0xC0FFEE1234567, launch=9, start=(-0.9, -0.9), goal=(0.9, 0.9)),
    "narrow_small_budget": dict(_PM, env="EnvNarrowPassageDense2D", n=8, step=0.05, max_iters=400, max_nodes=24, gen_seed=1, launch=2 ** 33 + 1,
                                start=(-0.9, -0.9), goal=(0.9, 0.9)),
    # 24 checks do not divide the workgroup's 256 threads: the last 16 threads must stay out of the check
    "dense_24_checks": dict(_PM, env="EnvDense2D", n=8, step=0.1, max_iters=600, n_edge_checks=24, gen_seed=2 ** 64 - 1, launch=13, start=(-0.9, 0.05),
                            goal=(0.9, 0.1)),
    # a sampling box that is ONE point: every tree walks to it and then inserts it again and again, so nearest() meets hundreds of nodes at distance
    # exactly zero - the lowest index has to win across lanes, waves and the strided loop.  No connect steps: the search ends with a full tree.
    "ties": dict(_PM, env="EnvDense2D", n=2, step=0.02, max_iters=1000, max_nodes=320, max_connect_steps=0, gen_seed=7, launch=5, start=(-0.9, 0.9),
                 goal=(-0.62, 0.953), box=((-0.62, 0.83), (-0.62, 0.83))),
    # the Panda: link spheres and self-collision pairs split over the threads of a check; the straight line start -> goal (1.8 rad) collides
    "panda": dict(_PM, env="EnvSpheres3D", robot="RobotPanda", n=3, step=0.25, max_iters=150, gen_seed=2 ** 40 + 3, launch=2,
                  start=(0.03, -0.3, -0.46, -0.96, 1.25, 3.65, 2.56), goal=(0.06, 0.63, 0.4, -2.04, 1.15, 2.99, 2.25)),
    # the 3-D point mass (the q_dim 3 / ws_dim 3 instantiation): three coordinates per sample, across the sphere field of EnvSpheres3D
    "pm3": dict(_PM, env="EnvSpheres3D", robot="RobotPointMass3D", n=4, step=0.15, max_iters=300, gen_seed=11, launch=4, start=(-0.9, 0.0, 0.6),
                goal=(0.9, 0.1, 0.6)),
}


def case_seed(case):
    return (case["gen_seed"] * 1000003 + case["launch"]) % 2 ** 64
