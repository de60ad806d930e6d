"""fp64 reference of the grid signed-distance lookup (include/mpdx.h, mpdx_field; csrc/grid_field.hpp) - test infrastructure.

`GridField` has the duck type oracle.costs.CostCollision reads (`kind == "objects"`, `sdf(points)`), so it plugs into the unchanged oracle guide and
its autograd:
  linear  : plain torch ops on the fp32 node values upcast to the dtype of the points; cell coordinate formed as the header says -
            (p - origin) * inv with inv = 1 / cell taken ONCE in fp32, then everything in the points' dtype; autograd differentiates it
            (a clamped axis gets zero gradient from torch.clamp);
  nearest : a torch.autograd.Function that returns the value of the node round((p - origin) * inv) (torch.round: half to even) and, in backward,
            that node's STORED gradient.
The node values come from whoever builds the field; the GPU tests download them from the device bake, so that guide parity does not depend on
the bake's rounding (the bake has a test of its own).
"""
import numpy as np
import torch


class _NearestLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, field):
        idx = field.node_index(p.detach())
        ctx.field, ctx.idx = field, idx
        return field.sdf_flat.to(p.dtype)[idx]

    @staticmethod
    def backward(ctx, gout):
        g = ctx.field.grad_flat.to(gout.dtype)[ctx.idx]
        return gout.unsqueeze(-1) * g, None


class GridField:
    kind = "objects"

    def __init__(self, sdf, origin, cell, mode="linear", grad=None):
        """sdf [nz, ny, nx] or [ny, nx] (fp32 node values, x fastest); grad [..., >= dim] node gradients (nearest mode); origin [dim]; cell float"""
        sdf = torch.as_tensor(sdf).detach().cpu().to(torch.float32)
        self.dim = sdf.dim()
        self.n = tuple(reversed(sdf.shape))                      # (nx, ny[, nz])
        self.sdf_flat = sdf.reshape(-1)
        self.grad_flat = None if grad is None else torch.as_tensor(grad).detach().cpu().to(torch.float32).reshape(-1, grad.shape[-1])[:, :self.dim]
        self.origin = torch.tensor(np.asarray(origin, np.float32)[:self.dim])     # fp32 values, as the descriptor carries them
        self.cell = float(np.float32(cell))
        self.inv = float(np.float32(1.0) / np.float32(cell))    # the reciprocal the launcher takes, in fp32
        if mode not in ("linear", "nearest"):
            raise ValueError(mode)
        if mode == "nearest" and self.grad_flat is None:
            raise ValueError("nearest mode returns the stored gradient")
        self.mode = mode
        self.strides = [1, self.n[0], self.n[0] * self.n[1]][:self.dim]

    # ---- cell coordinates
    def coords(self, p):
        """clamped cell coordinate c [..., dim] of points p [..., dim] (differentiable; zero gradient where clamped)"""
        u = (p - self.origin.to(p.dtype)) * self.inv
        hi = torch.tensor([v - 1 for v in self.n], dtype=p.dtype)
        return torch.minimum(torch.maximum(u, torch.zeros_like(u)), hi.expand_as(u))

    def node_index(self, p):
        c = self.coords(p)
        idx = torch.round(c).long()
        flat = torch.zeros(idx.shape[:-1], dtype=torch.long)
        for j in range(self.dim):
            flat = flat + idx[..., j].clamp(0, self.n[j] - 1) * self.strides[j]
        return flat

    def discontinuity_distance(self, p):
        """distance (in cells) of every point to the nearest discontinuity of the lookup along any axis: a cell face (integer cell coordinate) in
        linear mode - the gradient jumps there -, a cell mid-plane (half-integer) in nearest mode - value and gradient jump there.  Uses the
        UNCLAMPED coordinate (a point beyond the box is measured against the box face it was clamped to in linear mode; in nearest mode a point
        beyond the box is far from every mid-plane)."""
        u = ((p - self.origin.to(p.dtype)) * self.inv).detach()
        hi = torch.tensor([v - 1 for v in self.n], dtype=p.dtype)
        if self.mode == "linear":
            inside = (u - torch.round(u)).abs()
            d = torch.where(u < 0, -u, torch.where(u > hi, u - hi, inside))
        else:
            c = torch.minimum(torch.maximum(u, torch.zeros_like(u)), hi.expand_as(u))
            d = ((c - torch.floor(c)) - 0.5).abs()
            d = torch.where((u < -0.5) | (u > hi + 0.5), torch.full_like(d, 0.5), d)
        return d.amin(-1)

    # ---- lookup
    def sdf(self, p):
        if self.mode == "nearest":
            return _NearestLookup.apply(p, self)
        c = self.coords(p)
        i = torch.floor(c.detach()).long()
        for j in range(self.dim):
            i[..., j] = i[..., j].clamp(0, self.n[j] - 2)
        w = c - i.to(p.dtype)
        nodes = self.sdf_flat.to(p.dtype)
        base = sum(i[..., j] * self.strides[j] for j in range(self.dim))

        def corner(dx, dy, dz=0):
            off = dx + dy * self.strides[1] + (dz * self.strides[2] if self.dim == 3 else 0)
            return nodes[base + off]

        def lerp_xy(dz):
            s0 = corner(0, 0, dz) + w[..., 0] * (corner(1, 0, dz) - corner(0, 0, dz))
            s1 = corner(0, 1, dz) + w[..., 0] * (corner(1, 1, dz) - corner(0, 1, dz))
            return s0 + w[..., 1] * (s1 - s0)
        if self.dim == 2:
            return lerp_xy(0)
        t0, t1 = lerp_xy(0), lerp_xy(1)
        return t0 + w[..., 2] * (t1 - t0)

    def node_positions(self, dtype=torch.float64):
        """[nz, ny, nx, dim] (or [ny, nx, dim]) positions of the nodes exactly as the bake forms them: origin + (float)i * cell in fp32"""
        axes = [(np.arange(self.n[j], dtype=np.float32) * np.float32(self.cell) + self.origin[j].numpy()).astype(np.float32) for j in range(self.dim)]
        mesh = np.meshgrid(*reversed(axes), indexing="ij")          # z, y, x order of the leading axes
        return torch.from_numpy(np.stack(list(reversed(mesh)), -1)).to(dtype)
