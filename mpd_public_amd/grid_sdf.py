"""Signed-distance grids (MPDX_FIELD_GRID) and the ways to make one: node values of the caller's own, a bake from sphere / box primitives, an occupancy
map or a point cloud, a triangle mesh, depth frames.  The last four run on the device (csrc/k_grid.hip); the lookups are in csrc/grid_field.hpp.
planning.py - the environments, robots and tasks that use a grid as a collision field - imports the names from here; this module does not import it
at load time (the robot mask of the depth fusion takes planning.robot_link_spheres when it is called).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _lib

GRID_MODES = {"linear": _lib.GRID_LINEAR, "nearest": _lib.GRID_NEAREST}
MESH_SIGNS = {"winding": _lib.MESH_SIGN_WINDING, "none": _lib.MESH_SIGN_NONE}


@dataclass
class GridSDF:
    """A signed-distance field sampled on a regular grid (torch_robotics' GridMapSDF, un-vendored: the lookup is restated in include/mpdx.h with
    both plausible forms - `mode` 'linear': bi-/trilinear interpolation, gradient = its analytic derivative; 'nearest': the value and the STORED
    gradient of the nearest node, GridMapSDF as recalled).

    sdf    [nz, ny, nx] (3-D) or [ny, nx] (2-D) node values, x fastest; node (ix, iy, iz) sits at origin + (ix, iy, iz) * cell
    grad   None (linear mode needs none) or [..., dim] / [..., 4] node gradients, same leading shape as sdf
    A grid to be baked on first use from primitives (`for_primitives`, `PlanningTask(sdf_grid=...)`) has sdf = None and carries `source` / `shape` instead.
    A grid made from an occupancy map or a point cloud (`from_occupancy`, `from_points`: an exact Euclidean distance transform on the device,
    mpdx_sdf_grid_from_occupancy) holds its planes on the device from the start and can be re-run in place (`update_occupancy`).
    So does a grid made from a triangle mesh (`from_mesh`: every node against every triangle on the device, mpdx_sdf_grid_from_mesh; `update_mesh`);
    `mesh_info` says what was done to the mesh on the way (None for every other grid).  A grid made from depth frames (`from_depth`: TSDF integration,
    mpdx_tsdf_integrate, then the transform of the occupancy it leaves) also holds its tsdf and weight planes and fuses more frames (`integrate_depth`)."""
    sdf: Optional[torch.Tensor]
    origin: np.ndarray
    cell: float
    mode: str = "linear"
    grad: Optional[torch.Tensor] = None
    source: Any = None                      # bake from these primitives (an ObjectSet: its prim_floats(); mpdx_sdf_grid_bake) when sdf is None
    shape: Optional[tuple] = None           # (nx, ny[, nz]) of a grid still to be baked
    inflate: float = 0.0                    # occupancy grids: every obstacle thickened by this much (a point cloud has no thickness of its own)

    def __post_init__(self):
        if self.mode not in GRID_MODES:
            raise ValueError(f"GridSDF mode {self.mode!r}: 'linear' or 'nearest'")
        self.origin = np.asarray(self.origin, np.float32).reshape(-1)
        self.cell = float(self.cell)
        if not self.cell > 0:
            raise ValueError("GridSDF cell must be positive")
        if self.sdf is None:
            if self.source is None or self.shape is None:
                raise ValueError("GridSDF needs node values (sdf) or primitives to bake them from (source, shape)")
        else:
            self.sdf = torch.as_tensor(self.sdf)
            if self.sdf.dim() not in (2, 3):
                raise ValueError("GridSDF sdf is [ny, nx] or [nz, ny, nx]")
            self.shape = tuple(reversed(self.sdf.shape))
            if self.grad is not None:
                self.grad = torch.as_tensor(self.grad)
                if tuple(self.grad.shape[:-1]) != tuple(self.sdf.shape) or self.grad.shape[-1] not in (self.dim, 4):
                    raise ValueError("GridSDF grad is sdf.shape + (dim,) or sdf.shape + (4,)")
            elif self.mode == "nearest":
                raise ValueError("GridSDF mode 'nearest' returns the stored node gradient: give grad")
        self.shape = tuple(int(v) for v in self.shape)
        if len(self.shape) != self.origin.size or min(self.shape) < 2:
            raise ValueError("GridSDF: one origin coordinate per axis and at least 2 nodes along every axis")
        self._planes = None
        self._occ = None      # occupancy grids: the byte map [n_nodes] and the transform's workspace, both on the device of the planes
        self._ws = None
        self._mesh = None     # mesh grids: (vertices [V, 3] fp32, faces [F, 3] int32, sign mode) on the device of the planes
        self.mesh_info = None
        self._tsdf = None     # depth grids: (tsdf [n_nodes], weight [n_nodes]) fp32 on the device of the planes, and the settings of the fusion
        self._depth_cfg = None

    @classmethod
    def for_primitives(cls, objects, ws_min, ws_max, cell_size, mode="linear", padding=0.3):
        """A grid still to be baked (on the device, on first use) from the spheres and boxes of `objects`, on the box `grid_spec_for` places around the workspace."""
        if getattr(objects, "track", None) is not None:
            raise ValueError("GridSDF.for_primitives: the object set carries a track, and a grid does not move - keep a moving set as primitives "
                             "(PlanningTask(moving_objects=...)) and bake the fixed objects only")
        shape, origin = grid_spec_for(ws_min, ws_max, cell_size, padding)
        return cls(None, origin, cell_size, mode=mode, source=objects, shape=shape)

    @classmethod
    def _on_device(cls, shape, origin, cell, mode, inflate, device, what):
        """An empty grid whose planes live on `device` from the start; `what` completes the refusal of any other device."""
        if mode not in GRID_MODES:
            raise ValueError(f"GridSDF mode {mode!r}: 'linear' or 'nearest'")
        if not (float(inflate) >= 0 and np.isfinite(float(inflate))):
            raise ValueError("GridSDF inflate must be non-negative and finite")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"a signed-distance grid is made from {what}; there is no CPU fallback")
        rev = tuple(reversed([int(v) for v in shape]))
        sdf = torch.empty(rev, dtype=torch.float32, device=device)
        grad = torch.empty(rev + (4,), dtype=torch.float32, device=device) if mode == "nearest" else None   # linear mode reads none
        g = cls(sdf, origin, cell, mode=mode, grad=grad, inflate=float(inflate))
        g._planes = (g.sdf.reshape(-1), None if grad is None else g.grad.reshape(-1))
        return g

    @property
    def dim(self) -> int:
        return len(self.shape)

    @property
    def n_nodes(self) -> int:
        return int(np.prod(self.shape))

    @property
    def _made_on_device(self) -> bool:   # an occupancy or mesh grid lives where it was made: the planes update_* writes are the planes every user reads
        return self._occ is not None or self._mesh is not None

    def _n3(self):                       # n[3] and origin[3] of the C ABI: 1 and 0 along the unused axis of a 2-D grid
        return (C.c_int * 3)(*(list(self.shape) + [1] * (3 - self.dim)))

    def _origin3(self):
        return (C.c_float * 3)(*([float(v) for v in self.origin] + [0.0] * (3 - self.dim)))

    def planes(self, device):
        """(sdf plane [n_nodes] fp32, gradient plane [n_nodes * 4] fp32 or None) on `device`, baked there first if need be."""
        device = torch.device(device)
        if self._made_on_device:
            here = self._planes[0].device
            if device.type != here.type or device.index not in (None, here.index):
                what = "depth frames" if self._tsdf is not None else "an occupancy map" if self._occ is not None else "a mesh"
                raise RuntimeError(f"this GridSDF was made from {what} on {here}; it is not copied to {device}")
            return self._planes
        if self._planes is not None and self._planes[0].device == device:
            return self._planes
        if self.sdf is None:
            self._planes = self._bake(device)
        else:
            sdf = self.sdf.to(device=device, dtype=torch.float32).contiguous().reshape(-1)
            grad = None
            if self.grad is not None:
                g = self.grad.to(device=device, dtype=torch.float32).reshape(-1, self.grad.shape[-1])
                grad = torch.zeros((g.shape[0], 4), dtype=torch.float32, device=device)
                grad[:, :self.dim] = g[:, :self.dim]
                grad = grad.reshape(-1)
            self._planes = (sdf, grad)
        return self._planes

    def _bake(self, device):
        if device.type != "cuda":
            raise RuntimeError("a signed-distance grid is baked on the GPU (mpdx_sdf_grid_bake); there is no CPU fallback")
        gp = _lib.GuideParams()
        gp.ws_dim, gp.n_fields = self.dim, 1
        sp, bx = self.source.prim_floats()
        f = gp.fields[0]
        f.kind, f.sphere_off, f.n_spheres, f.box_off, f.n_boxes = _lib.FIELD_OBJECTS, 0, sp.size // 4, sp.size, bx.size // 6
        table = np.concatenate([sp, bx, np.zeros(4, np.float32)]).astype(np.float32)
        prims = torch.from_numpy(table).to(device)
        gp.prims, gp.n_prim_floats = prims.data_ptr(), sp.size + bx.size
        sdf = torch.empty(self.n_nodes, dtype=torch.float32, device=device)
        grad = torch.empty(self.n_nodes * 4, dtype=torch.float32, device=device) if self.mode == "nearest" else None   # linear mode reads none
        with torch.cuda.device(device):
            _lib.check(_lib.load().mpdx_sdf_grid_bake(C.byref(gp), 0, sdf.data_ptr(), None if grad is None else grad.data_ptr(), C.byref(self._n3()),
                                                      C.byref(self._origin3()), self.cell, _lib.current_stream()), "mpdx_sdf_grid_bake")
            torch.cuda.current_stream().synchronize()   # (prims may be freed after this)
        return sdf, grad

    # ---- occupancy maps and point clouds: the exact Euclidean distance transform of csrc/edt.hpp (arithmetic in include/mpdx.h)
    @classmethod
    def _empty_occupancy(cls, shape, origin, cell, mode, inflate, device):
        g = cls._on_device(shape, origin, cell, mode, inflate, device, "an occupancy map on the GPU (mpdx_sdf_grid_from_occupancy)")
        g._occ = torch.zeros(g.n_nodes, dtype=torch.uint8, device=g.sdf.device)
        g._ws = torch.empty(max(1, _lib.load().mpdx_sdf_grid_edt_ws_bytes(g._n3()) // 4), dtype=torch.int32, device=g.sdf.device)
        return g

    @classmethod
    def from_occupancy(cls, occ, origin, cell, mode="linear", inflate=0.0, device="cuda"):
        """occ: bool / uint8 array or tensor [ny, nx] or [nz, ny, nx] (x fastest; non-zero = occupied; node (ix, iy, iz) is the voxel centre
        origin + i * cell).  Returns a GridSDF whose planes already live on `device`; the gradient plane is written for mode='nearest' only."""
        occ = _occupancy_bytes(occ)
        g = cls._empty_occupancy(tuple(reversed(occ.shape)), origin, cell, mode, inflate, device)
        g._occ.copy_(occ.reshape(-1))
        g._transform()
        return g

    @classmethod
    def from_points(cls, points, ws_min, ws_max, cell_size, padding=0.3, mode="linear", inflate=0.0, device="cuda"):
        """points [P, 3] (z ignored in 2-D), voxelised on the device into the grid box `grid_spec_for` places around the
        workspace (a point outside the box, or with a non-finite coordinate, is dropped), then transformed."""
        shape, origin = grid_spec_for(ws_min, ws_max, cell_size, padding)
        g = cls._empty_occupancy(shape, origin, cell_size, mode, inflate, device)
        g._voxelise(points)
        g._transform()
        return g

    def update_occupancy(self, occ=None, points=None):
        """Re-run the transform INTO THE PLANES THIS GRID ALREADY HOLDS (a perception loop): `occ` (same shape as before) replaces the map, `points`
        are voxelised into it (into an empty map when occ is None).  A guide or task whose grid buffer is a concatenation of planes copies them
        again with its refresh_grids(); where the single plane is used in place there is nothing to copy."""
        if self._occ is None:
            raise ValueError("update_occupancy: this GridSDF was not made by from_occupancy / from_points")
        if occ is None and points is None:
            raise ValueError("update_occupancy: give occ, points or both")
        if occ is not None:
            occ = _occupancy_bytes(occ)
            if tuple(occ.shape) != tuple(reversed(self.shape)):
                raise ValueError(f"update_occupancy: occ has shape {tuple(occ.shape)}, the grid {tuple(reversed(self.shape))} (the planes are re-used: same shape)")
        if points is not None:
            points = self._points(points)      # (both inputs are checked before the map is touched)
        if occ is not None:
            self._occ.copy_(occ.reshape(-1))
        else:
            self._occ.zero_()
        if points is not None:
            self._voxelise(points)
        self._transform()
        return self

    def occupancy(self):
        """the byte map [nz, ny, nx] | [ny, nx] on the device (None for a grid that was not made from one)"""
        return None if self._occ is None else self._occ.reshape(tuple(reversed(self.shape)))

    def _points(self, points):
        pts = torch.as_tensor(points)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"points are [P, 3] (z is ignored in 2-D), got {tuple(pts.shape)}")
        return pts.to(device=self._occ.device, dtype=torch.float32).contiguous()

    def _voxelise(self, points):
        pts = self._points(points)
        with torch.cuda.device(self._occ.device):
            _lib.check(_lib.load().mpdx_occupancy_from_points(pts.data_ptr(), int(pts.shape[0]), self._occ.data_ptr(), C.byref(self._n3()),
                                                              C.byref(self._origin3()), self.cell, _lib.current_stream()), "mpdx_occupancy_from_points")
            pts.record_stream(torch.cuda.current_stream())

    def _transform(self):
        sdf, grad = self._planes
        with torch.cuda.device(self._occ.device):
            _lib.check(_lib.load().mpdx_sdf_grid_from_occupancy(self._occ.data_ptr(), sdf.data_ptr(), None if grad is None else grad.data_ptr(), None,
                                                                C.byref(self._n3()), self.cell, self.inflate, self._ws.data_ptr(), self._ws.numel() * 4,
                                                                _lib.current_stream()), "mpdx_sdf_grid_from_occupancy")

    # ---- triangle meshes: every node against every triangle, csrc/mesh_sdf.hpp (arithmetic in include/mpdx.h)
    @classmethod
    def from_mesh(cls, vertices, faces, ws_min, ws_max, cell_size, padding=0.3, mode="linear", inflate=0.0, sign="winding", device="cuda"):
        """vertices [V, 3], faces [F, 3] (integer; arrays or tensors), or a path (.obj / .stl, mesh.load_mesh) in place of vertices with faces=None.
        The grid box is the one `grid_spec_for` places around the (3-D) workspace.  sign='winding': a closed mesh, negative inside (generalised winding
        number > 0.5; a mesh whose signed volume is negative is taken as oriented inwards and its faces are reversed); sign='none': the unsigned
        distance, for open sheets and scans - `inflate` gives them thickness.  Zero-area faces are dropped.  `mesh_info` records dropped_faces,
        flipped, signed_volume and the counts.  The planes live on `device` from the start; the gradient plane is written for mode='nearest' only."""
        v32, f32, info = _check_mesh(vertices, faces, sign)
        ws_min, ws_max = np.asarray(ws_min, np.float64).reshape(-1), np.asarray(ws_max, np.float64).reshape(-1)
        if ws_min.size != 3 or ws_max.size != 3:
            raise ValueError(f"from_mesh: a mesh grid is 3-D only (the workspace has {ws_min.size} axes)")
        shape, origin = grid_spec_for(ws_min, ws_max, cell_size, padding)
        g = cls._on_device(shape, origin, cell_size, mode, inflate, device, "a mesh on the GPU (mpdx_sdf_grid_from_mesh)")
        g._mesh = (torch.from_numpy(v32).to(g.sdf.device), torch.from_numpy(f32).to(g.sdf.device), MESH_SIGNS[sign])
        g.mesh_info = info
        g._mesh_run()
        return g

    def update_mesh(self, vertices, faces=None):
        """Re-run INTO THE PLANES THIS GRID ALREADY HOLDS.  faces=None keeps the faces the grid holds (as they were left by from_mesh: zero-area faces
        dropped, an inward mesh reversed) and takes the same number of vertices - an object that moves rigidly between frames; with faces the mesh is
        checked, cleaned and oriented afresh.  A guide or task copies the planes again with its refresh_grids(), as after update_occupancy."""
        if self._mesh is None:
            raise ValueError("update_mesh: this GridSDF was not made by from_mesh")
        old_v, old_f, sign_mode = self._mesh
        sign = [k for k, v in MESH_SIGNS.items() if v == sign_mode][0]
        if faces is None:
            v32 = _mesh_vertices(vertices)
            if v32.shape[0] != old_v.shape[0]:
                raise ValueError(f"update_mesh: {v32.shape[0]} vertices for the {old_v.shape[0]} the stored faces index (give faces too for another mesh)")
            self._mesh = (torch.from_numpy(v32).to(old_v.device), old_f, sign_mode)
        else:
            v32, f32, info = _check_mesh(vertices, faces, sign)
            self._mesh = (torch.from_numpy(v32).to(old_v.device), torch.from_numpy(f32).to(old_v.device), sign_mode)
            self.mesh_info = info
        self._mesh_run()
        return self

    def _mesh_run(self):
        sdf, grad = self._planes
        v, f, sign_mode = self._mesh
        with torch.cuda.device(v.device):
            _lib.check(_lib.load().mpdx_sdf_grid_from_mesh(v.data_ptr(), int(v.shape[0]), f.data_ptr(), int(f.shape[0]), sdf.data_ptr(),
                                                           None if grad is None else grad.data_ptr(), None, C.byref(self._n3()), C.byref(self._origin3()),
                                                           self.cell, self.inflate, sign_mode, _lib.current_stream()), "mpdx_sdf_grid_from_mesh")
            for t in (v, f):
                t.record_stream(torch.cuda.current_stream())

    # ---- depth frames: projective TSDF integration, csrc/tsdf.hpp (arithmetic in include/mpdx.h), then the transform of the occupancy it leaves
    @classmethod
    def from_depth(cls, depth, intrinsics, world_from_cam, ws_min, ws_max, cell_size, padding=0.3, mode="linear", inflate=0.0, trunc=None,
                   max_weight=20.0, depth_range=(0.1, 5.0), depth_scale=1.0, robot=None, q=None, robot_padding=0.02, device="cuda"):
        """Fuse depth frames into a grid on the box `grid_spec_for` places around the (3-D) workspace, then transform its occupancy (as from_occupancy).
        depth        one image [h, w] or a list of them (or an [n, h, w] array), one per camera, each of its own size: float metres along the optical
                     axis, or uint16 scaled by `depth_scale` (0.001 for millimetres).  Pixels outside depth_range (NaN, inf, 0 ...) are no measurement.
        intrinsics   (fx, fy, cx, cy) per camera (pinhole, OpenCV frame x right / y down / z forward, pixel (iu, iv) centred at (iu, iv); undistorted)
        world_from_cam  a 4x4 or 3x4 [R | t] per camera, checked in float64 (finite, R orthonormal to 1e-4) and inverted there
        trunc        the truncation distance, default 3 * cell_size; max_weight caps the per-node weight (default 20: a node forgets an old surface
                     within about that many frames).  Both defaults are plain defaults, not tuned values.
        robot, q     mask the robot's link spheres (planning.robot_link_spheres, each padded by robot_padding) out of the frames: a pixel whose
                     back-projected point lies inside one neither carves nor occupies.  q [q_dim] or [k, q_dim]; at most 64 spheres in all.
        Unobserved nodes are free (a solid's unseen interior is free behind an occupied shell about trunc thick); `inflate` applies as for
        from_occupancy.  The planes (sdf, gradient for mode='nearest', tsdf, weight, occupancy) live on `device` from the start."""
        ws_min, ws_max = np.asarray(ws_min, np.float64).reshape(-1), np.asarray(ws_max, np.float64).reshape(-1)
        if ws_min.size != 3 or ws_max.size != 3:
            raise ValueError(f"from_depth: a depth grid is 3-D only (the workspace has {ws_min.size} axes)")
        cell = float(cell_size)
        trunc = 3.0 * cell if trunc is None else float(trunc)
        if not (trunc > 0 and np.isfinite(trunc)):
            raise ValueError("from_depth: trunc must be positive and finite")
        max_weight = float(max_weight)
        if not 1.0 <= max_weight <= float(1 << 24):
            raise ValueError("from_depth: max_weight must lie in 1 ... 2^24")
        lo, hi = (float(v) for v in depth_range)
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo < hi):
            raise ValueError("from_depth: depth_range is (min, max) with 0 <= min < max, finite")
        if not (float(depth_scale) > 0 and np.isfinite(float(depth_scale))):
            raise ValueError("from_depth: depth_scale must be positive and finite")
        if not (float(robot_padding) >= 0 and np.isfinite(float(robot_padding))):
            raise ValueError("from_depth: robot_padding must be non-negative and finite")
        cfg = dict(trunc=trunc, max_weight=max_weight, depth_range=(lo, hi), depth_scale=float(depth_scale), robot_padding=float(robot_padding))
        frames = _depth_frames(depth, intrinsics, world_from_cam, cfg["depth_scale"])
        spheres = _mask_spheres(robot, q, cfg["robot_padding"])
        shape, origin = grid_spec_for(ws_min, ws_max, cell, padding)
        g = cls._empty_occupancy(shape, origin, cell, mode, inflate, device)
        g._tsdf = (torch.zeros(g.n_nodes, dtype=torch.float32, device=g.sdf.device), torch.zeros(g.n_nodes, dtype=torch.float32, device=g.sdf.device))
        g._depth_cfg = cfg
        g._integrate(frames, spheres)
        g._transform()
        return g

    def integrate_depth(self, depth, intrinsics, world_from_cam, robot=None, q=None, reset=False):
        """Fuse more frames (the arguments of from_depth, with its settings) INTO THE TSDF, WEIGHT AND OCCUPANCY PLANES THIS GRID ALREADY HOLDS, then
        re-run the transform into its sdf and gradient planes; reset=True starts from an empty map (tsdf = weight = 0).  Returns self: a guide or task
        copies the planes again with its refresh_grids(), as after update_occupancy."""
        if self._tsdf is None:
            raise ValueError("integrate_depth: this GridSDF was not made by from_depth")
        frames = _depth_frames(depth, intrinsics, world_from_cam, self._depth_cfg["depth_scale"])
        spheres = _mask_spheres(robot, q, self._depth_cfg["robot_padding"])
        if reset:
            for p in self._tsdf:
                p.zero_()
        self._integrate(frames, spheres)
        self._transform()
        return self

    def tsdf(self):
        """(tsdf, weight) [nz, ny, nx] fp32 views on the device (None for a grid that was not made from depth frames)"""
        if self._tsdf is None:
            return None
        shp = tuple(reversed(self.shape))
        return self._tsdf[0].reshape(shp), self._tsdf[1].reshape(shp)

    def _integrate(self, frames, spheres):
        """mpdx_tsdf_integrate over the frames, at most MPDX_TSDF_MAX_CAMS per call (the cameras are taken in order either way)"""
        dev = self._occ.device
        cfg = self._depth_cfg
        sp = (C.c_float * max(4, spheres.size))(*spheres.reshape(-1).tolist())
        tsdf, weight = self._tsdf
        with torch.cuda.device(dev):
            imgs = [img.to(dev) if isinstance(img, torch.Tensor) else torch.from_numpy(img).to(dev) for img, _, _, _ in frames]
            for lo in range(0, len(frames), _lib.TSDF_MAX_CAMS):
                chunk = list(range(lo, min(len(frames), lo + _lib.TSDF_MAX_CAMS)))
                cams = (_lib.DepthCamera * len(chunk))()
                for c, i in enumerate(chunk):
                    _, k, A, B = frames[i]
                    cam = cams[c]
                    cam.depth, cam.height, cam.width = imgs[i].data_ptr(), int(imgs[i].shape[0]), int(imgs[i].shape[1])
                    cam.fx, cam.fy, cam.cx, cam.cy = (float(v) for v in k)
                    cam.cam_from_world[:], cam.world_from_cam[:] = A.reshape(-1).tolist(), B.reshape(-1).tolist()
                    cam.min_depth, cam.max_depth = cfg["depth_range"]
                _lib.check(_lib.load().mpdx_tsdf_integrate(cams, len(chunk), sp if spheres.size else None, spheres.shape[0], tsdf.data_ptr(),
                                                           weight.data_ptr(), self._occ.data_ptr(), C.byref(self._n3()), C.byref(self._origin3()),
                                                           self.cell, cfg["trunc"], cfg["max_weight"], _lib.current_stream()), "mpdx_tsdf_integrate")
            for t in imgs:
                t.record_stream(torch.cuda.current_stream())

    def node_values(self, device="cuda"):
        """(sdf [nz, ny, nx] | [ny, nx], grad [..., 4] or None) as the kernels read them (downloaded by the tests for their fp64 reference)."""
        sdf, grad = self.planes(device)
        shp = tuple(reversed(self.shape))
        return sdf.reshape(shp), (None if grad is None else grad.reshape(shp + (4,)))


def _mesh_vertices(vertices):
    """array or tensor [V, 3] -> contiguous fp32 numpy array, checked in float64: shape, finite"""
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 3 or v.dtype.kind not in "fiu":
        raise ValueError(f"mesh vertices are a [V, 3] array of at least three points (got {v.dtype} {tuple(v.shape)})")
    v = v.astype(np.float64)
    if not np.isfinite(v).all() or np.abs(v).max() > 3.0e38:
        raise ValueError("mesh vertices must be finite (in fp32)")
    return np.ascontiguousarray(v.astype(np.float32))


def _check_mesh(vertices, faces, sign):
    """The host-side checks of GridSDF.from_mesh, in float64, before anything is uploaded -> (vertices fp32 [V, 3], faces int32 [F, 3], mesh_info).
    A path goes through mesh.load_mesh.  Zero-area faces (of the fp32 vertices the device gets) are dropped; with sign='winding' a mesh of negative
    signed volume sum a . (b x c) / 6 is reversed."""
    if sign not in MESH_SIGNS:
        raise ValueError(f"from_mesh sign {sign!r}: 'winding' or 'none'")
    if isinstance(vertices, (str, bytes)) or hasattr(vertices, "__fspath__"):
        if faces is not None:
            raise ValueError("from_mesh: a mesh file brings its own faces (give faces=None with a path)")
        from .mesh import load_mesh
        vertices, faces = load_mesh(vertices)
    if faces is None:
        raise ValueError("from_mesh: faces are missing (only a path brings its own)")
    v32 = _mesh_vertices(vertices)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f"mesh faces are a [F, 3] array of vertex indices (got shape {tuple(f.shape)})")
    if f.dtype.kind not in "iu":
        raise ValueError(f"mesh faces are integers (got {f.dtype})")
    f = f.astype(np.int64)
    if f.min() < 0 or f.max() >= v32.shape[0]:
        raise ValueError(f"mesh faces index vertices 0 ... {v32.shape[0] - 1} (got {int(f.min())} ... {int(f.max())})")
    v = v32.astype(np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    keep = (np.cross(b - a, c - a) != 0).any(1)
    dropped = int((~keep).sum())
    f, a, b, c = f[keep], a[keep], b[keep], c[keep]
    if f.shape[0] == 0:
        raise ValueError("mesh faces: every face has zero area")
    if f.shape[0] > (1 << 20):
        raise ValueError(f"mesh faces: {f.shape[0]} faces (at most 2^20: decimate the mesh)")
    volume = float((a * np.cross(b, c)).sum() / 6.0)
    flipped = sign == "winding" and volume < 0
    if flipped:
        f = f[:, ::-1]
    info = dict(n_vertices=int(v32.shape[0]), n_faces=int(f.shape[0]), dropped_faces=dropped, flipped=bool(flipped), signed_volume=volume, sign=sign)
    return v32, np.ascontiguousarray(f.astype(np.int32)), info


def _depth_frames(depth, intrinsics, world_from_cam, depth_scale):
    """The host-side checks of GridSDF.from_depth / integrate_depth, in float64, before anything is uploaded -> [(image fp32 [h, w] (numpy, or the
    caller's float tensor), (fx, fy, cx, cy) float64, cam_from_world fp32 [3, 4], world_from_cam fp32 [3, 4])], one per camera.  The inverse is
    formed in float64 from the 4x4 pose and both matrices are rounded to fp32."""
    if isinstance(depth, (list, tuple)):
        imgs = list(depth)
    elif (depth.dim() if isinstance(depth, torch.Tensor) else np.ndim(depth)) == 3:
        imgs = list(depth)
    else:
        imgs = [depth]
    n = len(imgs)
    if n < 1:
        raise ValueError("depth: no frames")
    out = []
    for i, img in enumerate(imgs):
        if isinstance(img, torch.Tensor) and img.dtype.is_floating_point:
            im = img.detach().to(torch.float32).contiguous()
        else:
            a = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
            if a.dtype == np.uint16:
                a = a.astype(np.float64) * float(depth_scale)
            elif a.dtype.kind != "f":
                raise ValueError(f"depth[{i}]: float metres or uint16 (scaled by depth_scale) are expected, got {a.dtype}")
            im = np.ascontiguousarray(a.astype(np.float32))
        if im.ndim != 2 or not (1 <= im.shape[0] <= 8192 and 1 <= im.shape[1] <= 8192):
            raise ValueError(f"depth[{i}]: an image [h, w] with 1 ... 8192 pixels along each axis is expected, got {tuple(im.shape)}")
        out.append(im)
    k = np.asarray(intrinsics, np.float64)
    if k.shape == (4,) and n == 1:
        k = k[None]
    if k.shape != (n, 4):
        raise ValueError(f"intrinsics: (fx, fy, cx, cy) per camera, [{n}, 4] expected, got {tuple(k.shape)}")
    if not np.isfinite(k).all() or (k[:, :2] <= 0).any():
        raise ValueError("intrinsics: fx, fy must be positive and finite, cx, cy finite")
    if isinstance(world_from_cam, (list, tuple)) and any(np.ndim(v) == 2 for v in world_from_cam):
        poses = [np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float64) for v in world_from_cam]   # 4x4 and 3x4 mixed
    else:
        M = np.asarray(world_from_cam.detach().cpu().numpy() if isinstance(world_from_cam, torch.Tensor) else world_from_cam, np.float64)
        poses = [M] if M.ndim == 2 else list(M)
    if len(poses) != n or any(P.shape not in ((3, 4), (4, 4)) for P in poses):
        raise ValueError(f"world_from_cam: a 4x4 or 3x4 pose per camera ({n}) expected, got {[tuple(P.shape) for P in poses]}")
    if not all(np.isfinite(P).all() for P in poses):
        raise ValueError("world_from_cam: the poses must be finite")
    if any(P.shape[0] == 4 and (P[3] != np.array([0.0, 0.0, 0.0, 1.0])).any() for P in poses):
        raise ValueError("world_from_cam: the last row of a 4x4 pose must be (0, 0, 0, 1)")
    M = np.stack([P[:3] for P in poses])
    R = M[:, :3, :3]
    dev = np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max(axis=(1, 2))
    if (dev > 1e-4).any():
        raise ValueError(f"world_from_cam[{int(np.argmax(dev))}]: the rotation is not orthonormal to 1e-4 (|R R^T - I| = {dev.max():.3g})")
    H = np.zeros((n, 4, 4))
    H[:, :3] = M[:, :3]
    H[:, 3, 3] = 1.0
    inv = np.linalg.inv(H)
    return [(out[i], k[i], inv[i, :3].astype(np.float32), H[i, :3].astype(np.float32)) for i in range(n)]


def _mask_spheres(robot, q, padding):
    """[S, 4] fp32 (centre, radius + padding) of planning.robot_link_spheres(robot, q), S <= 64; [0, 4] without a robot"""
    if robot is None:
        if q is not None:
            raise ValueError("robot mask: q without a robot")
        return np.zeros((0, 4), np.float32)
    if q is None:
        raise ValueError("robot mask: give q with the robot")
    from .planning import robot_link_spheres
    sp = robot_link_spheres(robot, q)
    if sp.shape[0] > _lib.TSDF_MAX_SPHERES:
        raise ValueError(f"robot mask: {sp.shape[0]} spheres (at most {_lib.TSDF_MAX_SPHERES}: fewer configurations in q)")
    sp = sp.copy()
    sp[:, 3] += float(padding)
    sp = sp.astype(np.float32)
    if not np.isfinite(sp).all():
        raise ValueError("robot mask: the spheres must be finite in fp32")
    return sp


def _occupancy_bytes(occ):
    """bool / integer array or tensor [ny, nx] | [nz, ny, nx] -> contiguous uint8 tensor (non-zero = occupied), where it lives"""
    occ = torch.as_tensor(occ)
    if occ.dim() not in (2, 3):
        raise ValueError("occupancy is [ny, nx] or [nz, ny, nx]")
    if occ.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"occupancy is a bool or uint8 array (got {occ.dtype})")
    return occ.to(torch.uint8).contiguous()


def grid_spec_for(ws_min, ws_max, cell_size, padding=0.3, shift=0.37):
    """Node counts and origin of the grid box of a workspace: the limits grown by `padding` (default 0.3 m: more than the largest link radius 0.10 +
    the cutoff margin) with the origin moved down by a further `shift` cells.  The shift keeps geometry that is aligned with the world axes off the
    node planes - the Panda's first two collision spheres lie on the base axis (x = y = 0 at every configuration); unshifted they sit exactly on
    a node plane at every waypoint, where the interpolant has its kinks."""
    cell = float(cell_size)
    lo = np.asarray(ws_min, np.float64) - padding - shift * cell
    hi = np.asarray(ws_max, np.float64) + padding
    n = np.ceil((hi - lo) / cell).astype(np.int64) + 1
    return tuple(int(v) for v in n), lo.astype(np.float32)
