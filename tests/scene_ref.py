"""Shared pieces of the scene-batch tests (tests/test_scenes_cpu.py, tests/test_gpu_scenes.py): the three obstacle scenes, single-scene
views of a dataset, and the oracle's guide increment evaluated scene by scene (autograd over oracle/costs.py, as tests/helpers.py::oracle_guide)."""
import copy

import numpy as np
import torch

from mpd_public_amd import synthetic as syn
from mpd_public_amd.planning import ObjectSet

from helpers import oracle_guide, product_guide

SCENE_OF_CONTEXT = [2, 0, 2, 1]   # non-monotone, scene C used twice
N_PER_CONTEXT = 2


def _spheres(tag, n, dim, lo, hi, rlo, rhi, z_lo=None, z_hi=None):
    c = syn.hash_uniform(f"scenes/{tag}/c", n * dim, lo, hi).reshape(n, dim).astype(np.float32)
    if dim == 3 and z_lo is not None:   # keep them where the arm works
        c[:, 2] = z_lo + (z_hi - z_lo) * (c[:, 2] - lo) / (hi - lo)
    c3 = np.concatenate([c, np.zeros((n, 3 - dim), np.float32)], 1)
    return c3, syn.hash_uniform(f"scenes/{tag}/r", n, rlo, rhi).astype(np.float32)


def _boxes(tag, n, dim, lo, hi, half, z_lo=None, z_hi=None):
    c = syn.hash_uniform(f"scenes/{tag}/c", n * dim, lo, hi).reshape(n, dim).astype(np.float32)
    if dim == 3 and z_lo is not None:
        c[:, 2] = z_lo + (z_hi - z_lo) * (c[:, 2] - lo) / (hi - lo)
    c3 = np.concatenate([c, np.zeros((n, 3 - dim), np.float32)], 1)
    h3 = np.concatenate([np.full((n, dim), half, np.float32), np.full((n, 3 - dim), 1.0, np.float32)], 1)   # 2-D boxes: unbounded along z, as make_env
    return c3, h3


def scene_object_sets(dim, tag="abc"):
    """Scenes A (no extra primitive), B (3 spheres), C (5 spheres + 2 boxes) of a `dim`-D workspace."""
    z = dict(z_lo=0.3, z_hi=0.8) if dim == 3 else {}
    lo, hi = (-0.6, 0.6) if dim == 3 else (-0.8, 0.8)
    e = ObjectSet.empty()
    bc, br = _spheres(f"{tag}/B{dim}", 3, dim, lo, hi, 0.10, 0.16, **z)
    cc, cr = _spheres(f"{tag}/C{dim}", 5, dim, lo, hi, 0.08, 0.15, **z)
    cbc, cbh = _boxes(f"{tag}/Cb{dim}", 2, dim, lo, hi, 0.09, **z)
    return [e, ObjectSet(bc, br, e.box_centers.copy(), e.box_half.copy()), ObjectSet(cc, cr, cbc, cbh)]


def scene_dataset(ds, scenes, s, for_oracle=False):
    """`ds` with its task replaced by scene s as a single-scene PlanningTask: what one call per scene plans against.
    for_oracle: a field without a primitive is left out (oracle.costs.ObjectField takes the minimum over at least one primitive; the
    term it would stand for is zero, and so is the kernel's for an empty table)."""
    d = copy.copy(ds)
    d.task = scenes.scene_task(s)
    if for_oracle:
        for name in ("df_collision_extra_objects", "df_collision_objects"):
            f = getattr(d.task, name)
            if f is not None and f.objects is not None and f.grid is None and len(f.objects.sphere_radii) + len(f.objects.box_centers) == 0:
                setattr(d.task, name, None)
    return d


def single_scene_guides(ds, scenes, **kw):
    """One ordinary (single-scene) product guide per scene, built from the same primitives."""
    return [product_guide(scene_dataset(ds, scenes, s), **kw) for s in range(scenes.n_scenes)]


def oracle_increment(ds, scenes, scene_of_context, n_per_context, x, dtype=torch.float64, **kw):
    """guide(x) of the oracle, context by context, each against its own scene (the whole-tensor range test of the normaliser per context,
    as one reference call per context evaluates it).  x: normalised [B,H,D] CPU tensor -> [B,H,D] in `dtype`."""
    guides = {}
    out = []
    for c, s in enumerate(scene_of_context):
        if s not in guides:
            guides[s] = oracle_guide(scene_dataset(ds, scenes, s, for_oracle=True), dtype=dtype, **kw)[0]
        out.append(guides[s](x[c * n_per_context:(c + 1) * n_per_context].to(dtype)))
    return torch.cat(out)


def mismatch_fraction(got, ref, rtol=1e-3, atol=2e-6):
    """Fraction of waypoints with an element outside atol + rtol |ref| (the guide tolerance), and the mask."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = (np.abs(got - ref) > atol + rtol * np.abs(ref)).any(-1)
    return float(bad.mean()), bad
