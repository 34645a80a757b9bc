"""Triangle meshes to depth / instance images, and the dataset's full grids (csrc/render.hip).

What the reference gets from ``extra.pybullet.render_cad`` (an OpenGL render of one CAD model at its pose,
datasets/rgbd_pose_estimation/base.py:139-146) and from ``_get_grid_full`` (base.py:52-76).  Here a launch
renders a list of items -- (mesh, float64 ``T_cad2cam``, target image, instance id) -- with a float64
rasteriser whose result does not depend on the execution order (include/mfhip.h ``mf_render_*``, DESIGN.md
"Mesh rendering"): items of one target occlude each other (a composite scene), items with a target each are
what ``render_cad`` draws.  Colour is not rendered; pybullet / OpenGL pixel parity is unpinned.

NumPy or tensors in, device tensors out.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .mesh_sdf import _device, _rows


def _pack(meshes, dev):
    vs = [_rows(m[0], dev) for m in meshes]
    fs = [_rows(m[1], dev, torch.int32) for m in meshes]
    v_off, f_off = [0], [0]
    for v, f in zip(vs, fs):
        v_off.append(v_off[-1] + v.shape[0])
        f_off.append(f_off[-1] + f.shape[0])
    v = torch.cat(vs) if vs else torch.zeros((0, 3), dtype=torch.float64, device=dev)
    f = torch.cat(fs) if fs else torch.zeros((0, 3), dtype=torch.int32, device=dev)
    return v, f, v_off, f_off


class RenderPlan:
    """The buffers and the descriptor of one render launch; ``setup`` / ``raster`` / ``resolve`` are the three
    stages (``render_meshes`` runs them in order; the profile scripts time them one by one)."""

    def __init__(self, meshes, Ts_cad2cam, K, height, width, targets=None, instance_ids=None, near=0.01,
                 mesh_index=None, device=None):
        first = meshes[0][0] if len(meshes) else None
        dev = _device(first, device) if first is not None or device is not None else torch.device("cuda")
        self.device = dev
        v, f, v_off, f_off = _pack(meshes, dev)
        mesh_index = list(range(len(meshes))) if mesh_index is None else [int(m) for m in mesh_index]
        n = len(mesh_index)
        T = torch.as_tensor(np.asarray(Ts_cad2cam.detach().cpu() if isinstance(Ts_cad2cam, torch.Tensor)
                                       else Ts_cad2cam, np.float64).reshape(-1, 4, 4))
        if T.shape[0] != n:
            raise ValueError(f"{n} items but {T.shape[0]} transforms")
        if any(not 0 <= m < len(meshes) for m in mesh_index):
            raise ValueError("mesh index outside the meshes")
        targets = [0] * n if targets is None else [int(t) for t in targets]
        ids = list(range(n)) if instance_ids is None else [int(i) for i in np.asarray(instance_ids).reshape(-1)]
        if len(targets) != n or len(ids) != n:
            raise ValueError("targets / instance_ids differ in length from the items")
        if targets and min(targets) < 0:
            raise ValueError("negative target")
        self.n_items, self.n_targets = n, (max(targets) + 1) if n else 1
        self.height, self.width = int(height), int(width)
        rec_off = [0]
        for m in mesh_index:
            rec_off.append(rec_off[-1] + f_off[m + 1] - f_off[m])
        self.total = rec_off[-1]
        L = _lib.lib()
        nbytes = L.mf_render_workspace_bytes(self.total, self.n_targets, self.height, self.width)
        if nbytes < 0:
            raise ValueError(f"render of {self.total} faces into {self.n_targets} x {height} x {width}: past the caps "
                             "of include/mfhip.h (MF_RENDER_MAX_*)")
        i32 = lambda x: torch.tensor(x, dtype=torch.int32).reshape(-1).to(dev)  # noqa: E731
        i64 = lambda x: torch.tensor(x, dtype=torch.int64).reshape(-1).to(dev)  # noqa: E731
        shape = (self.n_targets, self.height, self.width)
        self.out = dict(depth=torch.empty(shape, dtype=torch.float32, device=dev),
                        instance=torch.empty(shape, dtype=torch.int32, device=dev),
                        face=torch.empty(shape, dtype=torch.int32, device=dev),
                        count=torch.zeros(n, dtype=torch.int32, device=dev))
        self._keep = [v, i64(v_off), f, i64(f_off), i32(mesh_index), T.to(dev).contiguous(), i32(targets), i32(ids),
                      i64(rec_off), torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=dev)]
        if dev.type == "cuda":
            _lib.require_gpu(*self._keep)
        b = _lib.RenderBatch()
        (b.vertices, b.v_off, b.faces, b.f_off, b.item_mesh, b.item_T, b.item_target, b.item_id, b.item_rec_off,
         b.workspace) = (_lib.ptr(t) for t in self._keep)
        if b.workspace & 15:
            b.workspace += 8
        b.depth, b.instance, b.face, b.count = (_lib.ptr(self.out[k]) for k in ("depth", "instance", "face", "count"))
        b.fx, b.fy, b.cx, b.cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
        b.near = float(near)
        b.n_meshes, b.n_items, b.n_targets = len(meshes), n, self.n_targets
        b.height, b.width = self.height, self.width
        self.batch = b

    def setup(self):
        _lib.check(_lib.lib().mf_render_setup(ctypes.byref(self.batch), self.total, _lib.stream_ptr()),
                   "mf_render_setup")

    def raster(self):
        _lib.check(_lib.lib().mf_render_raster(ctypes.byref(self.batch), self.total, _lib.stream_ptr()),
                   "mf_render_raster")

    def resolve(self):
        _lib.check(_lib.lib().mf_render_resolve(ctypes.byref(self.batch), self.total, _lib.stream_ptr()),
                   "mf_render_resolve")

    def run(self):
        self.setup()
        self.raster()
        self.resolve()
        return self.out


def render_meshes(meshes, Ts_cad2cam, K, height, width, targets=None, instance_ids=None, near=0.01, device=None,
                  mesh_index=None):
    """Render item n = ``meshes[n]`` (vertices [V, 3], faces [F, 3]) at ``Ts_cad2cam[n]`` (float64 4 x 4) through
    the pinhole ``K`` into image ``targets[n]`` (default: one composite image) with the id ``instance_ids[n]``
    (default n).  With ``mesh_index`` item n draws ``meshes[mesh_index[n]]`` (a mesh uploaded once, drawn often).
    Returns dict(depth float32 [T, H, W] -- z along the optical axis, NaN where nothing was hit; instance int32
    [T, H, W], -1 there; face int32 [T, H, W] -- the face of the winning item's mesh; count int32 [N] -- the pixels
    each item won) of device tensors; pixel (row i, col j) is sampled at (u, v) = (j, i), the convention of
    ``pointcloud_from_depth``."""
    return RenderPlan(meshes, Ts_cad2cam, K, height, width, targets, instance_ids, near, mesh_index, device).run()


def full_grids(points, Ts, pitch, origin, dim=32, device=None):
    """``grid_target_full`` / ``grid_nontarget_full`` of N examples (base.py:52-76, 180-195) in one launch:
    ``points[i]`` [n_i, 3] (the solid voxel centres of example i's CAD model) at ``Ts[i]`` (float64 4 x 4) into
    the ``dim``^3 grid (``pitch[e]``, ``origin[e]``) of every example e, idx = round((T p - origin) / pitch) half
    to even.  Returns int32 [N, dim, dim, dim] device tensors: target_full[e] = 1 where example e's own points
    fall; nontarget_full[e] = k + 1 where the points of the k-th of the other examples fall (the largest k on a
    voxel, the reference's last writer)."""
    n = len(points)
    first = points[0] if n else None
    dev = _device(first, device) if first is not None or device is not None else torch.device("cuda")
    P = [_rows(p, dev) for p in points]
    p_off = [0]
    for p in P:
        p_off.append(p_off[-1] + p.shape[0])
    f64 = lambda x: torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x,  # noqa: E731
                                               np.float64)).to(dev).contiguous()
    T, h, o = f64(Ts).reshape(-1, 16), f64(pitch).reshape(-1), f64(origin).reshape(-1, 3)
    if T.shape[0] != n or h.numel() != n or o.shape[0] != n:
        raise ValueError("points, Ts, pitch and origin differ in length")
    packed = torch.cat(P) if P else torch.zeros((0, 3), dtype=torch.float64, device=dev)
    off = torch.tensor(p_off, dtype=torch.int64).to(dev)
    gt = torch.empty((n, dim, dim, dim), dtype=torch.int32, device=dev)
    gn = torch.empty((n, dim, dim, dim), dtype=torch.int32, device=dev)
    if dev.type == "cuda":
        _lib.require_gpu(packed, off, T, h, o)
    _lib.check(_lib.lib().mf_full_grids(_lib.ptr(packed), _lib.ptr(off), _lib.ptr(T), _lib.ptr(h), _lib.ptr(o), n,
                                        p_off[-1], int(dim), _lib.ptr(gt), _lib.ptr(gn), _lib.stream_ptr()),
               "mf_full_grids")
    return gt, gn
