"""Occupancy grids to welded, smoothed triangle meshes, and the render service's label test (csrc/gridmesh.hip).

``grid_msg_to_mesh`` of the reference (ros/src/morefusion_ros/nodes/voxel_grids_to_mesh_markers.py:80-97) for a batch
of grids: the 0.5-level surface over the six-tetrahedra subdivision of the padded lattice, welded, then
``trimesh.smoothing.filter_humphrey`` (include/mfhip.h ``mf_gridmesh_*``, DESIGN.md "Grid meshes": marching-cubes and
trimesh parity are unpinned).  Vertex and face order are fixed by the input alone and every sum has one order, so the
meshes are bitwise reproducible.

Host synchronisation: ONE read-back per call -- the per-grid vertex / face offsets [2, B + 1] -- because the host has
to size the output buffers.

NumPy or tensors in, device tensors out.
"""
import numpy as np
import torch

from .. import _lib
from .mesh_sdf import _device

MAX_DIM = 32  # MF_GRIDMESH_MAX_DIM
MAX_NEIGHBOURS = 12  # MF_GRIDMESH_MAX_NEIGHBOURS


def _tensor(x, dev, dtype):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


class GridMeshPlan:
    """The buffers of one ``voxel_grids_to_meshes`` call; ``count`` / ``emit`` / ``adjacency`` / ``smooth`` are its
    stages (the profile script times them one by one)."""

    def __init__(self, grids, pitch, origin, device=None):
        first = grids[0] if len(grids) else None
        dev = _device(first, device) if first is not None or device is not None else torch.device("cuda")
        self.device = dev
        gs = [_tensor(g, dev, torch.float32) for g in grids]
        for g in gs:
            if g.dim() != 3 or min(g.shape) < 1 or max(g.shape) > MAX_DIM:
                raise ValueError(f"a grid must be [X, Y, Z] with every side in 1..{MAX_DIM}, got {tuple(g.shape)}")
        self.B = B = len(gs)
        self.pitch = _tensor(pitch, dev, torch.float64).reshape(-1)
        self.origin = _tensor(origin, dev, torch.float64).reshape(-1, 3)
        if self.pitch.numel() != B or self.origin.shape[0] != B:
            raise ValueError("grids, pitch and origin differ in length")
        self.n_vertices = self.n_faces = 0
        self.v_off = self.f_off = [0] * (B + 1)
        self.vertices = torch.zeros((0, 3), dtype=torch.float64, device=dev)
        self.faces = torch.zeros((0, 3), dtype=torch.int32, device=dev)
        if B == 0:
            return
        if _lib.lib().mf_gridmesh_workspace_bytes(B, 0) < 0:
            raise ValueError(f"{B} grids: past MF_GRIDMESH_MAX_GRIDS of include/mfhip.h")
        g_off = [0]
        for g in gs:
            g_off.append(g_off[-1] + g.numel())
        self.grids = torch.cat([g.reshape(-1) for g in gs])
        self.g_off = torch.tensor(g_off, dtype=torch.int64).to(dev)
        self.dims = torch.tensor([list(g.shape) for g in gs], dtype=torch.int32).reshape(-1).to(dev)
        self.ws = torch.empty(_lib.lib().mf_gridmesh_workspace_bytes(B, 0) // 8 + 2, dtype=torch.float64, device=dev)
        self.offsets = torch.empty((2, B + 1), dtype=torch.int64, device=dev)
        if dev.type == "cuda":
            _lib.require_gpu(self.grids, self.g_off, self.dims, self.pitch, self.origin, self.ws, self.offsets)

    def count(self):
        """Launch the count and the scan; read the offsets back and size the outputs."""
        if self.B == 0:
            return
        _lib.check(_lib.lib().mf_gridmesh_count(self.grids.data_ptr(), self.g_off.data_ptr(), self.dims.data_ptr(),
                                                self.B, self.ws.data_ptr(), self.offsets.data_ptr(),
                                                _lib.stream_ptr()), "mf_gridmesh_count")
        off = self.offsets.cpu().numpy()  # the call's read-back
        self.v_off, self.f_off = off[0].tolist(), off[1].tolist()
        self.n_vertices, self.n_faces = self.v_off[-1], self.f_off[-1]
        if _lib.lib().mf_gridmesh_workspace_bytes(self.B, max(self.n_vertices, self.n_faces)) < 0:
            raise ValueError("the batch's meshes are past MF_GRIDMESH_MAX_ROWS of include/mfhip.h")
        self.vertices = torch.empty((self.n_vertices, 3), dtype=torch.float64, device=self.device)
        self.faces = torch.empty((self.n_faces, 3), dtype=torch.int32, device=self.device)

    def emit(self):
        if self.B == 0:
            return
        _lib.check(_lib.lib().mf_gridmesh_emit(
            self.grids.data_ptr(), self.g_off.data_ptr(), self.dims.data_ptr(), self.pitch.data_ptr(),
            self.origin.data_ptr(), self.B, self.ws.data_ptr(), self.offsets.data_ptr(), self.n_vertices, self.n_faces,
            self.vertices.data_ptr(), self.faces.data_ptr(), _lib.stream_ptr()), "mf_gridmesh_emit")

    def adjacency(self):
        n = self.n_vertices
        self.neighbours = torch.empty((n, MAX_NEIGHBOURS), dtype=torch.int32, device=self.device)
        self.degree = torch.empty(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return
        _lib.check(_lib.lib().mf_gridmesh_adjacency(
            self.faces.data_ptr(), self.offsets.data_ptr(), self.B, n, self.n_faces, self.neighbours.data_ptr(),
            self.degree.data_ptr(), _lib.stream_ptr()), "mf_gridmesh_adjacency")

    def smooth(self, alpha=0.1, beta=0.5, iterations=10):
        n = self.n_vertices
        if n == 0 or iterations == 0:
            return
        nbytes = _lib.lib().mf_gridmesh_workspace_bytes(0, n)
        ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().mf_gridmesh_smooth(
            self.vertices.data_ptr(), self.neighbours.data_ptr(), self.degree.data_ptr(), n, float(alpha), float(beta),
            int(iterations), ws.data_ptr(), _lib.stream_ptr()), "mf_gridmesh_smooth")

    def meshes(self):
        return [(self.vertices[self.v_off[b]:self.v_off[b + 1]], self.faces[self.f_off[b]:self.f_off[b + 1]])
                for b in range(self.B)]


def voxel_grids_to_meshes(grids, pitch, origin, smooth=True, alpha=0.1, beta=0.5, iterations=10, device=None):
    """``grids``: [B, X, Y, Z] or a list of [X, Y, Z] arrays (sides in 1..32, a cell is occupied iff its value is > 0);
    ``pitch`` [B]; ``origin`` [B, 3], the centre of voxel (0, 0, 0).  Returns a list of (vertices float64 [V, 3],
    faces int32 [F, 3]) device tensors, one per grid; a grid without an occupied cell gives an empty mesh.  The
    meshes are closed 2-manifolds wound counter-clockwise seen from the empty side; ``smooth`` applies the Humphrey
    filter (trimesh's defaults), ``iterations=0`` or ``smooth=False`` returns the extracted surface."""
    if int(iterations) < 0:
        raise ValueError("iterations must be >= 0")
    plan = GridMeshPlan(grids, pitch, origin, device)
    plan.count()
    plan.emit()
    if smooth and int(iterations) > 0:
        plan.adjacency()
        plan.smooth(alpha, beta, iterations)
    return plan.meshes()


def label_of_render(depth_rendered, instance, depth_sensor):
    """The label test of the reference's render service (nodes/render_voxel_grids.py:66-99) on [H, W] device images:
    the rendered instance where something was drawn, -2 elsewhere and where the rendered depth is more than 1 cm
    behind the sensor's (a NaN reading keeps the label)."""
    H, W = instance.shape
    dev = instance.device
    dr = depth_rendered.to(torch.float32).contiguous()
    ins = instance.to(torch.int32).contiguous()
    ds = _tensor(depth_sensor, dev, torch.float32)
    if dr.shape != (H, W) or ds.shape != (H, W):
        raise ValueError("the rendered depth, the instance image and the sensor depth differ in size")
    if dev.type == "cuda":
        _lib.require_gpu(dr, ins, ds)
    label = torch.empty((H, W), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().mf_gridmesh_label(dr.data_ptr(), ins.data_ptr(), ds.data_ptr(), H, W, label.data_ptr(),
                                            _lib.stream_ptr()), "mf_gridmesh_label")
    return label
