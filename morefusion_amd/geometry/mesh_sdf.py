"""Triangle meshes on the device: signed distance and solid voxelization (csrc/meshsdf.hip).

What the reference's ``YCBVideoModels`` gets from trimesh and binvox (datasets/ycb_video/models.py:56-115):
``cad.nearest.signed_distance(points)`` (positive inside) and a solid voxel grid of the CAD model.  Here both
are one float64 kernel (include/mfhip.h ``mf_meshsdf_*``): per query the nearest-face distance (Ericson's
closest point), the arg-min face and the generalized winding number; inside := w >= 0.5 or d <= 1e-8.  The
solid grid is D^3 cells over the cube of the mesh's largest bbox extent, anchored at the bbox min; a cell is
occupied iff w >= 0.5 at its centre or its centre is within h / 2 of the surface.  DESIGN.md "CAD model
preparation" has the contract; binvox / trimesh parity is unpinned.

NumPy in, NumPy out; tensors in, tensors on their device out.  The ``*_batch`` forms take many meshes in one
launch per stage.
"""
import collections

import numpy as np
import torch

from .. import _lib

_THREADS = 256  # queries per workgroup (k_meshsdf_query)

TriangleMesh = collections.namedtuple("TriangleMesh", ["vertices", "faces"])


class SolidVoxelGrid:
    """``matrix`` bool [D, D, D] ((i, j, k) = x, y, z), ``points`` = centres of the occupied cells [n, 3] in matrix
    order, ``origin`` [3] (the bbox min: the corner of cell (0, 0, 0)), ``pitch`` (the cell size)."""

    def __init__(self, matrix, points, origin, pitch):
        self.matrix, self.points, self.origin, self.pitch = matrix, points, origin, pitch

    def __repr__(self):
        return f"SolidVoxelGrid(shape={tuple(self.matrix.shape)}, filled={len(self.points)}, pitch={self.pitch:.6g})"


def load_obj(path, return_colors=False):
    """Wavefront OBJ -> (vertices float64 [V, 3], faces int32 [F, 3]).  Reads ``v`` and ``f`` lines only; face
    corners ``a``, ``a/b``, ``a//c``, ``a/b/c``, 1-based or negative (relative to the vertices read so far);
    polygons are fan-triangulated (a, b, c), (a, c, d), ...  ``return_colors``: -> (vertices, faces, colors), the
    ``r g b`` that ``v x y z r g b`` lines carry (the vertex-colour extension, 0 .. 1) as float64 [V, 3] with 0 0 0 for a
    vertex without them, or None if no ``v`` line of the file has a colour."""
    verts, faces, colors, coloured = [], [], [], False
    with open(path, "r") as fh:
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                verts.append([float(x) for x in parts[1:4]])
                if return_colors:
                    rgb = [float(x) for x in parts[4:7]]
                    coloured |= len(rgb) == 3
                    colors.append(rgb if len(rgb) == 3 else [0.0, 0.0, 0.0])
            elif parts[0] == "f":
                idx = []
                for c in parts[1:]:
                    i = int(c.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{path}: face index outside the {len(v)} vertices")
    if return_colors:
        return v, f.astype(np.int32), np.asarray(colors, np.float64).reshape(-1, 3) if coloured else None
    return v, f.astype(np.int32)


def save_obj(path, vertices, faces, colors=None):
    """(vertices [V, 3], faces [F, 3]; NumPy or tensors) -> a Wavefront OBJ of ``v`` and ``f`` lines that ``load_obj``
    reads back: faces exactly, vertices to the 17 significant digits written (every float64 survives them).
    ``colors``: uint8 [V, 4] (r, g, b, alpha: ``TsdfVolume.sample_colors``) or [V, 3]; the lines become ``v x y z r g b``
    with r, g, b divided by 255 -- the vertex-colour extension that viewers read -- and 0 0 0 where alpha is 0."""
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    v, f = v.astype(np.float64).reshape(-1, 3), f.astype(np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"face index outside the {len(v)} vertices")
    if colors is not None:
        c = colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape[0] != len(v) or c.shape[1] not in (3, 4):
            raise ValueError(f"colors must be uint8 [{len(v)}, 3 or 4], got {c.dtype} {c.shape}")
        rgb = c[:, :3].astype(np.float64) / 255.0
        if c.shape[1] == 4:
            rgb[c[:, 3] == 0] = 0.0
    with open(path, "w") as fh:
        if colors is not None:
            for (x, y, z), (r, g, b) in zip(v.tolist(), rgb.tolist()):
                fh.write(f"v {x:.17g} {y:.17g} {z:.17g} {r:.17g} {g:.17g} {b:.17g}\n")
        else:
            for x, y, z in v.tolist():
                fh.write(f"v {x:.17g} {y:.17g} {z:.17g}\n")
        for a, b, c in f.tolist():
            fh.write(f"f {a + 1} {b + 1} {c + 1}\n")


def _device(x, device):
    if device is not None:
        return torch.device(device)
    return x.device if isinstance(x, torch.Tensor) else torch.device("cuda")


def _rows(x, device, dtype=torch.float64):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=dtype).reshape(-1, 3).contiguous()


class _Meshes:
    """Packed meshes with their face records (one prepare launch)."""

    def __init__(self, meshes, device):
        L = _lib.lib()
        self.device = device
        vs = [_rows(m[0], device) for m in meshes]
        fs = [_rows(m[1], device, torch.int32) for m in meshes]
        if not vs:
            raise ValueError("no meshes")
        for v, f in zip(vs, fs):
            if v.shape[0] == 0:
                raise ValueError("a mesh without vertices")
            if f.shape[0] and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
                raise ValueError(f"face index outside the mesh's {v.shape[0]} vertices")
        if device.type == "cuda":
            _lib.require_gpu(*vs, *fs)
        self.vertices = vs
        self.v_off = [0]
        self.f_off = [0]
        for v, f in zip(vs, fs):
            self.v_off.append(self.v_off[-1] + v.shape[0])
            self.f_off.append(self.f_off[-1] + f.shape[0])
        self.n = len(vs)
        self._v = torch.cat(vs)
        self._f = torch.cat(fs)
        self._v_off = torch.tensor(self.v_off, dtype=torch.int64, device=device)
        self._f_off = torch.tensor(self.f_off, dtype=torch.int64, device=device)
        nbytes = L.mf_meshsdf_workspace_bytes(self.f_off[-1])
        if nbytes < 0:
            raise ValueError(f"{self.f_off[-1]} faces: past the cap of {1 << 26} faces per batch")
        self._rec = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)
        b = self._batch()
        _lib.check(L.mf_meshsdf_prepare(b, self.f_off[-1], _lib.stream_ptr()), "mf_meshsdf_prepare")

    def _batch(self, **kw):
        b = _lib.MeshSdfBatch()
        b.vertices, b.v_off, b.faces, b.f_off = (_lib.ptr(t) for t in (self._v, self._v_off, self._f, self._f_off))
        b.face_rec = _lib.ptr(self._rec)
        b.n_meshes = self.n
        for k, v in kw.items():
            setattr(b, k, _lib.ptr(v) if isinstance(v, torch.Tensor) or v is None else v)
        return b

    def query(self, counts, points=None, grid_origin=None, grid_h=None, grid_dim=0, outputs=("sdf",)):
        """One query launch: ``counts[m]`` queries of mesh m (packed ``points`` or grid cells) -> dict of
        packed outputs among dist, face, winding, sdf, occupancy."""
        L = _lib.lib()
        q_off, blk_off = [0], [0]
        for c in counts:
            q_off.append(q_off[-1] + int(c))
            blk_off.append(blk_off[-1] + (int(c) + _THREADS - 1) // _THREADS)
        if blk_off[-1] >= 2 ** 31:
            raise ValueError("too many queries for one launch")
        Q, dev = q_off[-1], self.device
        dt = dict(dist=torch.float64, face=torch.int32, winding=torch.float64, sdf=torch.float64,
                  occupancy=torch.uint8)
        out = {k: torch.empty(Q, dtype=dt[k], device=dev) for k in outputs}
        q_off_d = torch.tensor(q_off, dtype=torch.int64, device=dev)
        blk_off_d = torch.tensor(blk_off, dtype=torch.int32, device=dev)
        b = self._batch(points=points, q_off=q_off_d, blk_off=blk_off_d, grid_origin=grid_origin, grid_h=grid_h,
                        **{k: out.get(k) for k in dt})
        b.n_blocks, b.grid_dim = blk_off[-1], int(grid_dim)
        _lib.check(L.mf_meshsdf_query(b, _lib.stream_ptr()), "mf_meshsdf_query")
        return out, q_off


def mesh_signed_distance_batch(meshes, points, outputs=("sdf", "dist", "face", "winding"), device=None):
    """``meshes`` = [(vertices [V, 3], faces [F, 3]), ...], ``points`` = one [n, 3] set per mesh -> a list (one
    per mesh) of dicts of float64 / int32 tensors on the device: sdf (+ inside, - outside), dist, face (the
    nearest face, lowest index on a tie; -1 without faces), winding.  One launch for all meshes."""
    dev = _device(points[0] if len(points) else meshes[0][0], device)
    M = _Meshes(meshes, dev)
    if len(points) != M.n:
        raise ValueError(f"{M.n} meshes but {len(points)} point sets")
    P = [_rows(p, dev) for p in points]
    packed = torch.cat(P) if P else torch.zeros((0, 3), dtype=torch.float64, device=dev)
    if dev.type == "cuda":
        _lib.require_gpu(packed)
    out, q_off = M.query([p.shape[0] for p in P], points=packed, outputs=outputs)
    return [{k: v[q_off[m]:q_off[m + 1]] for k, v in out.items()} for m in range(M.n)]


def mesh_signed_distance(vertices, faces, points, return_distance=False, return_face=False, return_winding=False,
                         device=None):
    """Signed distance of ``points`` [..., 3] to the mesh (positive inside, as trimesh's
    ``nearest.signed_distance``), float64 of the points' leading shape.  With ``return_distance`` /
    ``return_face`` / ``return_winding``: a tuple (sdf, [distance], [face id], [winding number])."""
    shape = tuple(points.shape[:-1]) if hasattr(points, "shape") else np.asarray(points).shape[:-1]
    r = mesh_signed_distance_batch([(vertices, faces)], [points], device=device)[0]
    flags = (("dist", return_distance), ("face", return_face), ("winding", return_winding))
    keep = ["sdf"] + [k for k, f in flags if f]
    res = [r[k].reshape(shape) for k in keep]
    if not isinstance(points, torch.Tensor):
        res = [x.cpu().numpy() for x in res]
    return res[0] if len(res) == 1 else tuple(res)


def grid_params(vertices, dimension):
    """(origin = bbox min [3] float64, h = largest bbox extent / dimension) of a float64 [V, 3] tensor."""
    vmin = vertices.min(dim=0).values
    ext = (vertices.max(dim=0).values - vmin).max()
    return vmin, ext / dimension


def solid_voxel_grid_batch(meshes, dimension=64, device=None):
    """Solid voxelization of many meshes in one launch -> list of SolidVoxelGrid with device tensors."""
    dev = _device(meshes[0][0], device)
    M = _Meshes(meshes, dev)
    D = int(dimension)
    if not 1 <= D <= 1024:
        raise ValueError("dimension must be 1..1024")
    params = [grid_params(v, D) for v in M.vertices]
    origin = torch.stack([p[0] for p in params]).contiguous()
    h = torch.stack([p[1] for p in params]).contiguous()
    out, _ = M.query([D ** 3] * M.n, grid_origin=origin, grid_h=h, grid_dim=D, outputs=("occupancy",))
    occ = out["occupancy"].reshape(M.n, D, D, D).bool()
    grids = []
    for m in range(M.n):
        ijk = torch.nonzero(occ[m]).to(torch.float64)
        pts = origin[m][None] + (ijk + 0.5) * h[m]
        grids.append(SolidVoxelGrid(occ[m], pts, origin[m], float(h[m])))
    return grids


def solid_voxel_grid(vertices, faces, dimension=64, device=None):
    """The mesh's solid D^3 voxel grid (the reference's binvox ``-d 64`` grid, restated): SolidVoxelGrid with
    NumPy arrays for NumPy vertices, device tensors for a tensor."""
    g = solid_voxel_grid_batch([(vertices, faces)], dimension, device=device)[0]
    if isinstance(vertices, torch.Tensor):
        return g
    return SolidVoxelGrid(g.matrix.cpu().numpy(), g.points.cpu().numpy(), g.origin.cpu().numpy(), g.pitch)
