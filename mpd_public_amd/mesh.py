"""Triangle meshes from files, for GridSDF.from_mesh (grid_sdf.py): Wavefront OBJ and STL (binary and ASCII), numpy only.

load_mesh(path) -> (vertices float64 [V, 3], faces int32 [F, 3]).  Nothing here touches the device; the checks a mesh must pass before it is uploaded
(finite vertices, indices in range, zero-area faces, orientation) are GridSDF.from_mesh's."""
from __future__ import annotations

import os
import struct

import numpy as np


def load_mesh(path):
    """OBJ: `v` and `f` records (polygons become triangle fans; `f v/vt/vn` forms and negative indices are accepted; everything else is ignored).
    STL: binary or ASCII, told apart by the 80-byte header plus a triangle count consistent with the file size; vertices are merged by exact equality.
    Any other suffix: ValueError."""
    path = os.fspath(path)
    suffix = os.path.splitext(path)[1].lower()
    if suffix == ".obj":
        return _load_obj(path)
    if suffix == ".stl":
        return _load_stl(path)
    raise ValueError(f"load_mesh: {path!r} is neither .obj nor .stl")


def _load_obj(path):
    verts, faces = [], []
    with open(path, "r", errors="replace") as f:
        for lineno, line in enumerate(f, 1):
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{lineno}: a vertex needs three coordinates")
                verts.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    if i == 0:
                        raise ValueError(f"{path}:{lineno}: OBJ indices start at 1")
                    i = i - 1 if i > 0 else len(verts) + i          # negative: relative to the vertices read so far
                    if not 0 <= i < len(verts):
                        raise ValueError(f"{path}:{lineno}: vertex index {t} is out of range")
                    idx.append(i)
                if len(idx) < 3:
                    raise ValueError(f"{path}:{lineno}: a face needs at least three vertices")
                faces += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
    if not verts or not faces:
        raise ValueError(f"{path}: no vertices or no faces")
    return np.array(verts, np.float64), np.array(faces, np.int32)


def _load_stl(path):
    with open(path, "rb") as f:
        raw = f.read()
    binary = False
    if len(raw) >= 84:
        (count,) = struct.unpack_from("<I", raw, 80)
        binary = len(raw) == 84 + 50 * count
    if binary:
        rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), count=count, offset=84)
        tri = rec["v"].astype(np.float64).reshape(-1, 3)
    else:
        tok = raw.decode("ascii", errors="replace").split()
        if not tok or tok[0].lower() != "solid" or "vertex" not in (t.lower() for t in tok):
            raise ValueError(f"{path}: neither a binary STL (header + triangle count do not match the file size) nor an ASCII one")
        pts = [[float(tok[k + 1]), float(tok[k + 2]), float(tok[k + 3])] for k, t in enumerate(tok) if t.lower() == "vertex" and k + 3 < len(tok)]
        if len(pts) % 3:
            raise ValueError(f"{path}: ASCII STL with {len(pts)} vertex records (three per facet)")
        tri = np.array(pts, np.float64)
    if tri.shape[0] == 0:
        raise ValueError(f"{path}: no triangles")
    verts, inverse = np.unique(tri, axis=0, return_inverse=True)        # exact equality
    return verts, inverse.reshape(-1, 3).astype(np.int32)
