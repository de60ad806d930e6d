"""The conditions of tests/test_gpu_grid_edges.py and what its yardstick can tell apart, from the fp64 reference alone (tests/grid_edges_ref.py over
the planes of tests/edt_ref.py): every case reaches the clamped branch of the lookup and its unclamped interior, stays inside the ambiguity cap, and
has a different node count along every used axis; and a reference altered the way a plausible bug of csrc/grid_field.hpp would alter the kernel -
a stride from the wrong node counts, the gradient kept along a clamped axis, the second grid read at offset 0 - differs from the true one by more
than twice the GPU test's tolerance at one or more unambiguous support waypoints of the case's own inputs."""
import numpy as np
import pytest

import grid_edges_ref as ger

EDGE_CASES = [(n, m) for n in ger.CASES for m in ("linear", "nearest")] + [("two", None)]
MIN_HINGES = 10


def _spec(name):
    return ger.TWO if name == "two" else ger.CASES[name]


@pytest.mark.parametrize("name,mode", EDGE_CASES, ids=[f"{n}-{m}" if m else n for n, m in EDGE_CASES])
def test_edge_case_conditions(name, mode):
    r = ger.cpu_reference(name, mode)
    c, comp = _spec(name), r["comp"]
    cap = ger.CAP[ger.robot_of(c["robot_id"])]
    print(f"{name} {mode}: ambiguous support waypoints {r['amb'].mean():.4f}, checked points {r['amb_m'].mean():.4f} (cap {cap}); "
          f"{int(r['hit'].sum())} of {r['hit'].size} checked points collide")
    assert r["amb"].mean() <= cap and r["amb_m"].mean() <= cap
    assert r["hit"].any() and not r["hit"].all()
    assert len(r["ks"]) == (2 if name == "two" else 1)
    robot = comp.cost_l[0].robot
    pts = robot.link_points(r["xi"][..., : robot.q_dim])                  # [B, N, K, dim]
    for k in r["ks"]:
        gf = comp.cost_l[k].field
        assert len(set(gf.n)) == gf.dim
        u = ((pts - gf.origin.double()) * gf.inv).numpy()
        hi = np.array([v - 1 for v in gf.n], np.float64)
        assert (u < 0).any() and (u > hi).any(), "link points leave the box below and above"
        active = (comp.cost_l[k].factors(r["xi"]) > 0).numpy()           # [B, N, K]
        cl = ger.clamped_points(gf, pts).numpy()
        n_cl, n_in, n_y = int((active & cl.any(-1)).sum()), int((active & ~cl.any(-1)).sum()), int((active & cl[..., 1]).sum())
        print(f"  field {k}: n = {gf.n}, active grid hinges {int(active.sum())}: {n_cl} at clamped link points ({n_y} with y clamped), {n_in} unclamped")
        if gf.n[1] == 2:
            assert n_y >= MIN_HINGES
        else:
            assert n_cl >= MIN_HINGES and n_in >= MIN_HINGES


def _mutations():
    out = []
    for name, mode in EDGE_CASES:
        if name == "two":
            out += [(name, mode, "row"), (name, mode, "clamped"), (name, mode, "offset0")]
            continue
        out.append((name, mode, "row"))
        if len(ger.CASES[name]["shape"]) == 3:
            out.append((name, mode, "plane"))
        if mode == "linear":
            out.append((name, mode, "clamped"))
    return out


MUTATIONS = _mutations()


@pytest.mark.parametrize("name,mode,kind", MUTATIONS, ids=[f"{n}-{m}-{k}" if m else f"{n}-{k}" for n, m, k in MUTATIONS])
def test_altered_reference_is_rejected(name, mode, kind):
    """'row' / 'plane' / 'clamped' alter the case's (last) grid field; 'offset0' reads the two-grid block's second field from the first field's
    planes.  The true reference passes the same yardstick."""
    r = ger.cpu_reference(name, mode)
    mut = ger.mutant_increment(name, mode, kind)
    bad = ger.outside(mut, r["ref"], 2.0) & ~r["amb"]
    print(f"{name} {mode} {kind}: the altered reference differs by > 2 x the tolerance at {int(bad.sum())} of {int((~r['amb']).sum())} unambiguous supports")
    assert bad.any()
    assert not (ger.outside(r["ref"], r["ref"]) & ~r["amb"]).any()


def test_two_grid_block_layout():
    """the two-grid block's first field is a nearest grid whose node count is no multiple of 4 (its planes are padded in the grid buffer), the
    second a linear grid over another box and with another cell"""
    a, b = ger.TWO["grids"]
    assert a["mode"] == "nearest" and b["mode"] == "linear"
    assert int(np.prod(a["shape"])) % 4 and a["shape"] != b["shape"] and a["origin"] != b["origin"] and a["cell"] != b["cell"]
    for g in (a, b):
        assert len(set(g["shape"])) == len(g["shape"]) and int(np.prod(g["shape"])) <= 100_000
    for c in ger.CASES.values():
        assert len(set(c["shape"])) == len(c["shape"]) and int(np.prod(c["shape"])) <= 100_000
    assert sum(1 for c in ger.CASES.values() if c["shape"][1] == 2) == 1
