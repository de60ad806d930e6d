"""float64 restatement of rrt_path_kernel, written from the contract in include/mpdx.h (mpdx_rrt_paths) and the published algorithms (path
extraction from the two trees of RRT-Connect, greedy shortcutting, arc-length resampling) - Python floats and numpy float64, no product
tensor code.  Collisions come in as the `slack_fn(q[N, q_dim]) -> [N]` that rrt_ref.Problem uses (helpers.oracle_config_slack).

  extract    start ... meeting node of tree 0, then tree 1's branch from ITS meeting node ... goal; a negative entry in either link, or a path of
             more than max_path (1024) nodes, gives [start, goal]
  shortcut   per round, from node i jump to the LAST later node whose edge is free, else to the next node; stop when a round removes nothing
             or 2 nodes are left.  An edge is checked on n_edge_checks configurations (1 - w) qa + w qb, w = c / (n - 1), end points included
  resample   cumulative arc length s; u_h = total h / (H - 1); segment = first node with s[k] > u, clamped to [1, m - 1]; linear interpolation
             with the segment length clamped to 1e-12 from below; the first and the last support are exactly the first and the last node;
             velocities by central differences over 2 dt, zero at both ends

compare() judges recorded device output.  An edge whose largest slack lies within rrt_ref.EDGE_EPS of zero cannot be settled by float64 for a
float32 evaluation: it ends that problem's comparison (the problem counts as cut short).

The bound is derived, not chosen.  eps = 2^-23, m path nodes, total length L, Q = max |q| over the path:
  positions   pos_tol = eps (2 (m + 3) L + 4 Q): a float32 running sum of m segment lengths plus the product and the quotient for u move the
              point ALONG a unit-speed path by at most the first term; the interpolation adds a few roundings of Q
  velocities  vel_tol = pos_tol / dt + 2 eps |v|  (two positions, each within pos_tol, over 2 dt; the difference's and the quotient's rounding)
End supports and end velocities are compared for equality.

FAULTS are deliberately wrong variants of the pipeline (run(p, fault)) for tests/test_paths_ref_cpu.py: compare() has to notice each of them.
EQUIVALENT_FAULTS are variants that NO input can tell from the pipeline, kept with the proof: `one_round` - a round of "jump to the last
visible later node" leaves a fixed point.  The kept nodes k_0 < k_1 < ... satisfy: k_(i+1) is the last node after k_i that k_i sees (or k_i + 1
when it sees none).  In the next round k_i examines a SUBSET of the nodes it examined before (the kept ones behind it), with the same,
deterministic edge checks, so its choice is k_(i+1) again: the second round removes nothing and the loop ends.  More than one round changes
the result only for a rule that is not idempotent, such as `first_visible`."""
import functools
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

from rrt_ref import EDGE_EPS

EPS32 = 2.0 ** -23
MAX_PATH = 1024
FAULTS = ("first_visible", "w_over_n", "searchsorted_left_unclamped", "forward_difference", "end_velocity_nonzero", "tree1_reversed",
          "link_node_twice", "ends_interpolated")
EQUIVALENT_FAULTS = ("one_round",)


class Ambiguous(Exception):
    pass


@dataclass
class Problem:
    """one launch's arguments as the kernel receives them: float32 values, held as float64"""
    start: np.ndarray              # [n, q]
    goal: np.ndarray               # [n, q]
    nodes: np.ndarray              # [n, 2, M, q]   tree 0 grows from the start, tree 1 from the goal
    parent: np.ndarray             # [n, 2, M]
    link: np.ndarray               # [n, 2]
    H: int
    dt: float
    n_edge_checks: int
    rounds: int
    slack_fn: Optional[Callable] = None      # (rounds = 0 needs none)

    def __post_init__(self):
        f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)   # noqa: E731
        self.start, self.goal, self.nodes = np.atleast_2d(f32(self.start)), np.atleast_2d(f32(self.goal)), f32(self.nodes)
        self.parent, self.link = np.asarray(self.parent, dtype=np.int64), np.asarray(self.link, dtype=np.int64)
        self.dt = float(np.float32(self.dt))

    @property
    def n(self):
        return len(self.start)

    @property
    def max_nodes(self):
        return self.nodes.shape[2]


@dataclass
class Report:
    mismatches: List[str] = field(default_factory=list)   # empty: the recorded trajectories are the reference's, within the bound
    cut_short: List[int] = field(default_factory=list)    # problems whose comparison ended at an ambiguous edge
    edge_checks: int = 0                                  # shortcut edge decisions verified (of the problems that were compared to the end)
    compared: int = 0                                     # problems compared to the end
    pos_frac: float = 0.0                                 # worst position error as a fraction of pos_tol
    vel_frac: float = 0.0                                 # worst velocity error as a fraction of vel_tol
    path_len: List[int] = field(default_factory=list)     # the reference's path length per problem (-1: cut short / not compared)


# ---------------------------------------------------------------------------------------------------------------------------- the three steps
def extract(nodes, parent, link, start, goal, max_path=MAX_PATH, fault=None):
    """nodes [2, M, q], parent [2, M], link [2] of ONE problem -> [m, q]"""
    nodes, start, goal = np.asarray(nodes, dtype=np.float64), np.asarray(start, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    line = np.stack([start, goal])
    if int(link[0]) < 0 or int(link[1]) < 0:
        return line
    branch = []
    for t in (0, 1):
        seq, k = [], int(link[t])
        while k >= 0:
            seq.append(k)
            if len(seq) > max_path:      # (also ends the walk over a parent table that loops)
                return line
            k = int(parent[t][k])
        branch.append(seq)
    if len(branch[0]) + len(branch[1]) > max_path:
        return line
    b0, b1 = nodes[0][branch[0][::-1]], nodes[1][branch[1]]
    if fault == "tree1_reversed":
        b1 = b1[::-1]
    if fault == "link_node_twice":
        b0 = np.concatenate([b0, b0[-1:]])
    return np.concatenate([b0, b1])


def edge_slack(qa, qb, slack_fn, n_edge_checks, fault=None):
    """largest slack over the edge's check configurations"""
    n = int(n_edge_checks)
    w = (np.arange(n) / (n if fault == "w_over_n" else n - 1))[:, None]
    return float(np.max(np.asarray(slack_fn((1.0 - w) * qa + w * qb), dtype=np.float64)))


def shortcut(path, slack_fn, n_edge_checks, rounds, fault=None, log=None):
    """-> the shortcut path [m', q]; raises Ambiguous at an edge float64 cannot settle.  `log`: a list that receives (i, j, largest slack) of
    every edge examined."""
    p = np.asarray(path, dtype=np.float64)
    if fault == "one_round":
        rounds = min(rounds, 1)

    def free(i, j):
        s = edge_slack(p[i], p[j], slack_fn, n_edge_checks, fault)
        if log is not None:
            log.append((i, j, s))
        if abs(s) <= EDGE_EPS:
            raise Ambiguous(f"edge {i} -> {j}: largest slack {s:.3e}")
        return s <= 0.0

    for _ in range(int(rounds)):
        m = len(p)
        if m <= 2:
            break
        keep, i = [0], 0
        while i < m - 1:
            later = range(i + 2, m) if fault == "first_visible" else range(m - 1, i + 1, -1)
            j = next((k for k in later if free(i, k)), i + 1)
            keep.append(j)
            i = j
        if len(keep) == m:
            break
        p = p[keep]
    return p


def _arc_f32(p):
    """cumulative arc length of a float32 path, every operation rounded to float32"""
    f = np.float32
    s = np.zeros(len(p), dtype=np.float32)
    for k in range(1, len(p)):
        d2 = f(0)
        for v in p[k] - p[k - 1]:
            d2 = f(d2 + f(v * v))
        s[k] = f(s[k - 1] + np.sqrt(d2))
    return s


def _resample_f32(path, H):
    """the interpolation formula in float32 for EVERY support, the two ends included (fault ends_interpolated: what an implementation gives
    that does not pin the ends to the nodes - in exact arithmetic the formula reproduces them, in float32 it need not)"""
    f = np.float32
    p = np.asarray(path, dtype=np.float32)
    m, s = len(p), _arc_f32(np.asarray(path, dtype=np.float32))
    out = np.zeros((H, p.shape[1]), dtype=np.float32)
    for h in range(H):
        u = f(f(s[-1] * f(h)) / f(H - 1))
        k = 1
        while k < m - 1 and s[k] <= u:
            k += 1
        den = max(f(s[k] - s[k - 1]), f(1e-12))
        w = min(max(f(f(u - s[k - 1]) / den), f(0)), f(1))
        out[h] = p[k - 1] * f(f(1) - w) + p[k] * w
    return out.astype(np.float64)


def resample(path, H, dt, fault=None):
    """[m, q] -> [H, 2q]"""
    p = np.asarray(path, dtype=np.float64)
    m, H = len(p), int(H)
    seg = np.sqrt(((p[1:] - p[:-1]) ** 2).sum(-1))
    s = np.concatenate([[0.0], np.cumsum(seg)])
    u = s[-1] * np.arange(H) / (H - 1)
    if fault == "searchsorted_left_unclamped":
        # first node with s[k] >= u, no clamp: index 0 (u = 0) makes the segment start at "node -1", which is outside the path - modelled as NaN
        k = np.searchsorted(s, u, side="left")
        pp, ss = np.concatenate([p, np.full((1, p.shape[1]), np.nan)]), np.concatenate([s, [np.nan]])   # row -1: not a node
        a, b, sa, sb = pp[k - 1], pp[np.minimum(k, m - 1)], ss[k - 1], ss[np.minimum(k, m - 1)]
    else:
        k = np.clip(np.searchsorted(s, u, side="right"), 1, m - 1)
        a, b, sa, sb = p[k - 1], p[k], s[k - 1], s[k]
    with np.errstate(invalid="ignore"):
        w = np.clip((u - sa) / np.maximum(sb - sa, 1e-12), 0.0, 1.0)[:, None]
    pos = a * (1.0 - w) + b * w
    if fault == "ends_interpolated":
        f32 = _resample_f32(p, H)
        pos[0], pos[-1] = f32[0], f32[-1]
    else:
        pos[0], pos[-1] = p[0], p[-1]
    vel = np.zeros_like(pos)
    if fault == "forward_difference":
        vel[1:-1] = (pos[2:] - pos[1:-1]) / dt
    else:
        vel[1:-1] = (pos[2:] - pos[:-2]) / (2.0 * dt)
    if fault == "end_velocity_nonzero":
        vel[0], vel[-1] = (pos[1] - pos[0]) / dt, (pos[-1] - pos[-2]) / dt
    return np.concatenate([pos, vel], axis=-1)


def tolerances(path, ref, dt):
    """(pos_tol scalar, vel_tol [H, q]) of the module docstring for the final path and its reference trajectory"""
    p = np.asarray(path, dtype=np.float64)
    q = p.shape[1]
    L = float(np.sqrt(((p[1:] - p[:-1]) ** 2).sum(-1)).sum())
    pos_tol = EPS32 * (2.0 * (len(p) + 3) * L + 4.0 * float(np.abs(p).max()))
    return pos_tol, pos_tol / dt + 2.0 * EPS32 * np.abs(ref[:, q:])


# ---------------------------------------------------------------------------------------------------------------------------- whole problems
def solve(p: Problem, b: int, fault=None, log=None):
    """problem b -> (final path [m, q], trajectory [H, 2q]); raises Ambiguous"""
    path = extract(p.nodes[b], p.parent[b], p.link[b], p.start[b], p.goal[b], fault=fault)
    if p.rounds > 0 and len(path) > 2:
        path = shortcut(path, p.slack_fn, p.n_edge_checks, p.rounds, fault, log)
    return path, resample(path, p.H, p.dt, fault)


def run(p: Problem, fault=None):
    """the pipeline on its own -> (trajs [n, H, 2q] float32, path_len [n] int32): what a device with that fault would return.  A problem with
    an ambiguous edge gets NaN trajectories and path_len -1 (compare() cuts it short before it looks at them)."""
    assert fault is None or fault in FAULTS + EQUIVALENT_FAULTS
    q = p.start.shape[1]
    trajs, plen = np.full((p.n, p.H, 2 * q), np.nan, dtype=np.float32), np.full(p.n, -1, dtype=np.int32)
    for b in range(p.n):
        try:
            path, tr = solve(p, b, fault)
        except Ambiguous:
            continue
        trajs[b], plen[b] = tr, len(path)
    return trajs, plen


def compare(trajs, path_len, p: Problem, problems=None) -> Report:
    """trajs [n, H, 2q] (and path_len [n], or None) as mpdx_rrt_paths wrote them, against the reference on the same trees"""
    trajs = np.asarray(trajs)
    q = p.start.shape[1]
    rep = Report(path_len=[-1] * p.n)
    if trajs.shape != (p.n, p.H, 2 * q) or (path_len is not None and np.asarray(path_len).shape != (p.n,)):
        rep.mismatches.append(f"shapes {trajs.shape} {None if path_len is None else np.asarray(path_len).shape}")
        return rep
    for b in (range(p.n) if problems is None else problems):
        log = []
        try:
            path, ref = solve(p, b, None, log)
        except Ambiguous:
            rep.cut_short.append(b)
            continue
        rep.compared += 1
        rep.edge_checks += len(log)
        rep.path_len[b] = len(path)
        got = trajs[b].astype(np.float64)
        if path_len is not None and int(path_len[b]) != len(path):
            rep.mismatches.append(f"problem {b}: path_len {int(path_len[b])}, reference {len(path)}")
            continue
        if not np.isfinite(got).all():
            rep.mismatches.append(f"problem {b}: {int((~np.isfinite(got)).sum())} values are not finite")
            continue
        pos_tol, vel_tol = tolerances(path, ref, p.dt)
        if not (np.array_equal(got[0, :q], path[0]) and np.array_equal(got[-1, :q], path[-1])):
            rep.mismatches.append(f"problem {b}: the end supports are not the path's end nodes (off by "
                                  f"{np.abs(got[0, :q] - path[0]).max():.3e} / {np.abs(got[-1, :q] - path[-1]).max():.3e})")
        if got[0, q:].any() or got[-1, q:].any():
            rep.mismatches.append(f"problem {b}: end velocities {got[0, q:]} / {got[-1, q:]}")
        pf = float(np.abs(got[:, :q] - ref[:, :q]).max() / pos_tol) if pos_tol > 0 else (0.0 if np.array_equal(got[:, :q], ref[:, :q]) else math.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            ve = np.abs(got[:, q:] - ref[:, q:])
            vf = float(np.where(vel_tol > 0, ve / np.where(vel_tol > 0, vel_tol, 1.0), np.where(ve > 0, math.inf, 0.0)).max())
        rep.pos_frac, rep.vel_frac = max(rep.pos_frac, pf), max(rep.vel_frac, vf)
        if pf > 1.0:
            h = int(np.abs(got[:, :q] - ref[:, :q]).max(-1).argmax())
            rep.mismatches.append(f"problem {b}: position error {pf:.3g} x the bound {pos_tol:.3e} (support {h}, path of {len(path)} nodes)")
        if vf > 1.0:
            rep.mismatches.append(f"problem {b}: velocity error {vf:.3g} x the bound (pos_tol {pos_tol:.3e}, dt {p.dt:g})")
    return rep


# ---------------------------------------------------------------------------------------------------------------------------- hand-built trees
def plant(M, branch0, branch1, seed, decoys=True):
    """one problem's trees around a given path: branch0 [k0, q] start ... meeting node, branch1 [k1, q] tree 1's meeting node ... goal.
    The roots sit at index 0; the other branch nodes at increasing, randomly chosen indices (a child behind its parent, as a search inserts
    them), interleaved with nodes that are NOT on the path: random coordinates, parents among the earlier nodes, branch nodes included.
    -> nodes [2, M, q] float32, parent [2, M] int32, link [2]"""
    rng = np.random.default_rng(seed)
    branch0, branch1 = np.atleast_2d(np.asarray(branch0, dtype=np.float32)), np.atleast_2d(np.asarray(branch1, dtype=np.float32))
    q = branch0.shape[1]
    nodes, parent, link = np.zeros((2, M, q), dtype=np.float32), np.full((2, M), -1, dtype=np.int32), [0, 0]
    for t, br in ((0, branch0), (1, branch1[::-1])):
        k = len(br)
        assert 1 <= k <= M
        at = np.concatenate([[0], 1 + np.sort(rng.choice(M - 1, k - 1, replace=False))]) if decoys else np.arange(k)
        used = int(at[-1]) + 1 if k > 1 else 1
        if decoys:      # fill every slot up to the last branch node, and a few behind it
            used = min(M, used + 3)
            for i in range(1, used):
                nodes[t, i], parent[t, i] = rng.uniform(-1.0, 1.0, q), rng.integers(0, i)
        nodes[t, at] = br
        parent[t, at[1:]] = at[:-1]
        parent[t, 0] = -1
        link[t] = int(at[-1])
    return nodes, parent, np.asarray(link, dtype=np.int32)


def problem_of(paths, M, H, dt, n_edge_checks=32, rounds=0, seed=0, splits=None, links=None, decoys=True):
    """a launch of hand-built trees: paths[b] = [m_b, q] start ... goal; splits[b] = nodes of tree 0's branch (default: alternating ends, middle);
    links[b] overrides the planted link (to declare a problem unsolved)"""
    n = len(paths)
    nodes, parent, link, start, goal = [], [], [], [], []
    for b, path in enumerate(paths):
        path = np.asarray(path, dtype=np.float32)
        k0 = (1, len(path) - 1, len(path) // 2)[b % 3] if splits is None or splits[b] is None else splits[b]
        k0 = max(1, min(len(path) - 1, k0))
        nd, pa, lk = plant(M, path[:k0], path[k0:], seed * 1000 + b, decoys)
        if links is not None and links[b] is not None:
            lk = np.asarray(links[b], dtype=np.int32)
        nodes.append(nd), parent.append(pa), link.append(lk), start.append(path[0]), goal.append(path[-1])
    return Problem(np.stack(start), np.stack(goal), np.stack(nodes), np.stack(parent), np.stack(link), H, dt, n_edge_checks, rounds)


# ---------------------------------------------------------------------------------------------------------------------------- the cases
# of tests/test_paths_ref_cpu.py (conditions, faults) and tests/test_gpu_rrt_paths.py (the device).  Each builder returns (env, robot, Problem
# without its slack_fn); helpers.paths_case attaches the oracle's float64 slack.
PM2, PM3, PANDA = ("EnvSimple2D", "RobotPointMass"), ("EnvSpheres3D", "RobotPointMass3D"), ("EnvSpheres3D", "RobotPanda")
NARROW = ("EnvNarrowPassageDense2D", "RobotPointMass")
DT = 5.0 / 64


def _rand_path(rng, m, q, scale=1.0):
    return rng.uniform(-scale, scale, (m, q))


def case_extract():
    """rounds = 0: which nodes, in which order (the geometry is free to be awkward: no collision check looks at it)"""
    rng = np.random.default_rng(11)
    paths = [_rand_path(rng, m, 2) for m in (2, 11, 11, 14, 9, 9, 3, 2)]
    #        both roots | deep tree 0, tree 1 at its root | the reverse | both deep | unsolved (-1, -1) | (k, -1) | one node beside a root | (-1, k)
    splits = [1, 10, 1, 6, 4, 5, 2, 1]
    p = problem_of(paths, 48, 16, DT, seed=1, splits=splits, links=[None, None, None, None, (-1, -1), None, None, None])
    p.link[5, 1], p.link[7, 0] = -1, -1
    return PM2 + (p,)


def _arc(k, radius, phase):
    a = phase + (math.pi / 2) * np.arange(k) / (k - 1)
    return radius * np.stack([np.cos(a), np.sin(a)], -1) - radius * 0.6


def case_path_cap():
    """the kPathMax = 1024 boundary: quarter arcs of length 2.2 ... 2.7 as chains of 1024 nodes (resampled as the arc) and of 1025 nodes (the
    straight line, path_len 2) - arc and chord are 0.4 apart in the middle, the bound is 6e-4"""
    ks = [(1024, 512), (1025, 513), (1024, 600), (1025, 400), (1025, 640), (1024, 384)]
    paths = [_arc(k, 1.4 + 0.06 * b, 0.3 * b) for b, (k, _) in enumerate(ks)]
    return PM2 + (problem_of(paths, 640, 64, DT, seed=2, splits=[k0 for _, k0 in ks]),)


@functools.lru_cache(maxsize=None)
def _resample_paths(q, H, scale):
    rng = np.random.default_rng(100 * q + H)
    e = np.eye(q)
    segs = max(d for d in range(1, 12) if (H - 1) % d == 0)
    step = 0.25 * scale
    a = np.cumsum(np.concatenate([np.zeros((1, q)), [step * (e[0] if k % 2 == 0 else e[1]) for k in range(segs)]]), 0) - 0.5 * scale   # equal segments, exact sums
    u = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=q))   # noqa: E731
    b = np.cumsum(np.stack([-0.7 * np.ones(q), 1.0 * u(), 1e-4 * u(), 1.0 * u(), 1e-4 * u()]) * np.array([[1], [scale], [1], [scale], [1]]), 0)
    c0 = _rand_path(rng, 3, q, scale)
    c = c0[[0, 1, 1, 1, 2]]                                  # zero-length segments in the middle
    d = np.stack([c0[0], c0[0]])                             # start == goal
    g = _rand_path(rng, 9, q, scale)
    loop = np.concatenate([c0, c0[:1]])                      # start == goal at the ends of a path with length
    dup_ends = g[[0, 0, 1, 2, 3, 3]]                         # zero-length first and last segment
    # a goal at the origin behind a long last segment, and a first node shifted until the float32 value of u_(H-1) = total (H - 1) / (H - 1) is NOT
    # the total (there is such a shift for H = 64 and 1024; the product and quotient are exact for H = 2, 3): interpolating the last support
    # instead of taking the node then leaves a residue of the last but one node there, where the goal's zeros make it visible
    z = np.stack([c0[0], 0.8 * scale * u(), np.zeros(q)])
    if H > 3:
        f = np.float32
        for k in range(40000):
            zk = z + np.concatenate([[1e-4 * k * scale * e[0]], np.zeros((2, q))])
            total = _arc_f32(zk.astype(f))[-1]
            if f(f(total * f(H - 1)) / f(H - 1)) < total:
                z = zk
                break
        assert not np.array_equal(_resample_f32(z, H)[-1], np.zeros(q)), "no shift found"
    return [a, b, c, d, g, loop, dup_ends, z]


def case_resample(robot, H, dt, M=24):
    q = {PM2: 2, PM3: 3, PANDA: 7}[robot]
    paths = _resample_paths(q, H, 1.0 if q < 7 else 2.0)
    return robot + (problem_of(paths, M, H, dt, seed=3 + H + q, links=[None, None, None, (0, 0), None, None, None, None],
                               splits=[None, None, None, 1, None, None, None, None]),)


# EnvNarrowPassageDense2D: the wall at x = 0 (|x| <= 0.05) with its gap |y| < 0.05; left of it a free pocket around (-0.15, 0.05), right of it
# one around (0.2, 0)
_L0, _L1, _R0, _R1 = (-0.15, 0.12), (-0.15, 0.0), (0.15, 0.0), (0.15, 0.15)
NARROW_PATHS = [
    # 12 nodes along the gap's axis that all see each other: "last visible" leaves 2 nodes in one round; "first visible" still has 3 after three
    [(-0.18 + 0.045 * k, 0.012 * ((k * 5) % 3 - 1)) for k in range(12)],
    [_L0, _L1, _R0, _R1],                                    # nothing can be removed: every chord crosses the wall
    [_R1, _R0, _L1, _L0],
    # from the first node the 3rd and 5th are visible, the 4th and 6th are not: first visible / last visible differ within ONE round
    [(-0.2, 0.0), (-0.1, 0.02), (0.12, 0.0), (0.12, 0.2), (0.3, 0.0), (0.3, 0.25), (0.2, 0.3)],
    [_L0, (-0.2, 0.1), _L1, (-0.1, -0.01), (0.02, -0.01), (0.1, 0.01), _R0, (0.25, 0.1), _R1, (0.3, 0.3)],
    [_L0, _R1],                                              # unsolved: the straight line through the wall, never shortcut
]


def case_shortcut(n_edge_checks, rounds):
    p = problem_of(NARROW_PATHS, 32, 64, DT, n_edge_checks, rounds, seed=5, links=[None] * 5 + [(-1, -1)], splits=[4, 2, 1, 5, 5, 1])
    return NARROW + (p,)


# the Panda among the spheres: a path around the colliding straight line of rrt_ref.CASES["panda"] (its start and goal; the three nodes between them
# are a solution of the search's reference, shortcut and rounded to two decimals), with a removable midpoint in its first and in its last edge
_P = np.array([[0.03, -0.3, -0.46, -0.96, 1.25, 3.65, 2.56], [-0.36, 0.04, -0.4, -1.49, 0.18, 2.47, 0.8], [-0.45, 0.13, -0.29, -1.56, 0.09, 2.31, 0.73],
               [-0.56, 0.63, 0.05, -1.7, -0.02, 2.27, 1.71], [0.06, 0.63, 0.4, -2.04, 1.15, 2.99, 2.25]])
PANDA_PATH = np.stack([_P[0], 0.5 * (_P[0] + _P[1]), _P[1], _P[2], _P[3], 0.5 * (_P[3] + _P[4]), _P[4]]).round(3)
# a via point around a chord whose deciding hinge is a SELF-collision pair (found by a scan of random chords through self-colliding configurations)
PANDA_SELF_PATH = np.array([[0.46, 0.65, 0.48, -2.94, -1.98, 0.29, -1.22], [-0.07, 0.89, -0.07, -2.71, -1.96, 1.19, -1.29],
                            [0.65, 1.45, -0.58, -3.03, -1.91, 0.68, -1.57]])
PANDA_PATHS = [PANDA_PATH, PANDA_PATH[::-1], PANDA_PATH[[0, 2, 3, 4, 6]], PANDA_PATH[[0, 1, 2, 4, 5, 6]][::-1], PANDA_PATH[[0, 6]], PANDA_SELF_PATH]


def case_panda(n_edge_checks):
    """n_edge_checks 16 / 32 / 100 / 200: the link spheres and self-collision pairs of a configuration are split over 12 / 8 / 2 / 1 threads"""
    return PANDA + (problem_of(PANDA_PATHS, 16, 64, DT, n_edge_checks, 3, seed=7, splits=[3, 2, 1, 4, 1, 2]),)


CASES = {
    "extract": case_extract,
    "path_cap": case_path_cap,
    **{f"resample_q2_H{H}_dt{i}": (lambda H=H, dt=dt: case_resample(PM2, H, dt)) for H in (2, 3, 64, 1024) for i, dt in enumerate((DT, 1e-3))},
    "resample_q3_H64": lambda: case_resample(PM3, 64, DT),
    "resample_q7_H3": lambda: case_resample(PANDA, 3, 1e-3),
    "resample_q7_H64": lambda: case_resample(PANDA, 64, DT),
    "resample_q7_H1024_lds": lambda: case_resample(PANDA, 1024, DT, M=2048),     # 82 KB of LDS: the launch that raises the 64 KB limit
    **{f"shortcut_c{c}_r{r}": (lambda c=c, r=r: case_shortcut(c, r)) for c, r in ((2, 3), (24, 1), (24, 3), (32, 3), (256, 1), (256, 3))},
    **{f"panda_c{c}": (lambda c=c: case_panda(c)) for c in (16, 32, 100, 200)},
}
HAND_BUILT_SHORTCUT = [k for k in CASES if k.startswith(("shortcut_", "panda_"))]


def case_search(trees, rrt_problem, n_edge_checks=32, rounds=3, H=64, dt=DT):
    """the full pipeline at its defaults on the trees of the search's reference (rrt_ref.free_run, cast to float32 as the device holds them)"""
    return Problem(rrt_problem.start, rrt_problem.goal, trees.nodes, trees.parent, trees.link, H, dt, n_edge_checks, rounds, rrt_problem.slack_fn)
