"""GPU test of the gradient-by-differences launcher the occupancy and the mesh producers share (csrc/k_grid.hip: launch_grid_gradient ->
grid_gradient_kernel<2 | 3> of csrc/grid_field.hpp) at the smallest shapes where its edge logic can go wrong: two nodes along every axis (every node is
first or last on every axis: one-sided differences only), two along some axes, a 2-D grid (the DIM = 2 instantiation), and one with interior nodes on
every axis.  The gradient plane must equal tests/edt_ref.grad_ref of the sdf plane the SAME call wrote, bit for bit: the same rounded fp32 operations,
so there is no tolerance."""
import numpy as np
import pytest

import edt_ref
import mesh_ref
from test_gpu_mesh_sdf import _run as run_mesh
from test_gpu_occupancy import _run_transform as run_occupancy

pytestmark = pytest.mark.gpu

CELL = 0.3
SHAPES = [(2, 2, 2), (2, 3, 4), (3, 2, 1), (5, 4, 3)]    # (nx, ny, nz)


def _same_bits(got, want):
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_shared_gradient_launcher_at_the_smallest_shapes(shape):
    nx, ny, nz = shape
    varied = 0
    for name in ("random50", "corner"):
        _, sdf, grad = run_occupancy(edt_ref.pattern(shape, name), CELL, 0.0)
        assert sdf.shape == (nz, ny, nx) and not np.isnan(sdf).any()
        assert _same_bits(grad, edt_ref.grad_ref(sdf, CELL)), (shape, name)
        assert not grad[..., 3].view(np.uint32).any() and (nz > 1 or not grad[..., 2].view(np.uint32).any())
        varied += int(grad[..., :2].any())
    assert varied, "every occupancy pattern gave a constant sdf plane: the differences were never exercised"
    if nz > 1:
        V, F = mesh_ref.box(*mesh_ref.BOX)
        # nodes on both sides of the box's faces: (lo + hi) / 2 - (n - 1) / 2 cells, moved off the symmetric position
        origin = tuple(float(0.5 * (lo + hi) - 0.5 * (n - 1) * CELL + 0.037) for lo, hi, n in zip(*mesh_ref.BOX, shape))
        sdf, grad, _ = run_mesh(V.astype(np.float32), F, dict(n=shape, origin=origin, cell=CELL), with_wind=False)
        assert _same_bits(grad, edt_ref.grad_ref(sdf, CELL)), shape
        assert not grad[..., 3].view(np.uint32).any() and grad[..., :3].any()
