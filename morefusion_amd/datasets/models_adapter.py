"""What ``RGBDPoseEstimationDatasetBase`` needs of its ``models``: ``get_cad``, ``get_voxel_pitch`` and the solid
voxel centres per class.  ``YCBVideoModels`` has them; ``MeshModels`` gives them for meshes held in memory."""
import numpy as np
import torch

from ..geometry import mesh_sdf


class MeshModels:
    """``{class_id: (vertices [V, 3], faces [F, 3])}`` with the methods of ``YCBVideoModels`` that the dataset
    calls (datasets/ycb_video/models.py: bbox diagonal / dimension as the voxel pitch, a solid 64^3 grid)."""

    def __init__(self, meshes_by_class, device=None):
        self._meshes = {int(c): mesh_sdf.TriangleMesh(np.asarray(v, np.float64).reshape(-1, 3),
                                                      np.asarray(f, np.int32).reshape(-1, 3))
                        for c, (v, f) in dict(meshes_by_class).items()}
        if any(c <= 0 for c in self._meshes):
            raise ValueError("class ids start at 1 (0 is the background)")
        self._device = torch.device(device) if device is not None else torch.device("cuda")

    @property
    def class_ids(self):
        return sorted(self._meshes)

    def get_cad(self, class_id):
        if int(class_id) not in self._meshes:
            raise IndexError(f"class_id {class_id} has no mesh")
        return self._meshes[int(class_id)]

    def get_pcd(self, class_id):
        """The model's point cloud (the reference's points.xyz): the mesh's vertices."""
        return self.get_cad(class_id).vertices

    def get_bbox_diagonal(self, class_id):
        v = self.get_cad(class_id).vertices
        extents = v.max(axis=0) - v.min(axis=0)
        return float(np.sqrt((extents ** 2).sum()))

    def get_voxel_pitch(self, dimension, class_id):
        return 1.0 * self.get_bbox_diagonal(class_id) / dimension

    def get_solid_voxel_grid(self, class_id, dimension=64):
        cad = self.get_cad(class_id)
        return mesh_sdf.solid_voxel_grid(cad.vertices, cad.faces, dimension, device=self._device)


class _Adapter:
    """``models`` plus a per-class cache of the solid voxel centres as device tensors (one voxelization launch for
    all the classes a frame asks for first)."""

    def __init__(self, models, device):
        self.models, self.device = models, torch.device(device)
        self._solid = {}

    def __getattr__(self, name):
        return getattr(self.models, name)

    def solid_points(self, class_ids, dimension=64):
        todo = [c for c in dict.fromkeys(int(c) for c in class_ids) if (c, dimension) not in self._solid]
        if todo:
            cads = [self.models.get_cad(c) for c in todo]
            grids = mesh_sdf.solid_voxel_grid_batch([(c.vertices, c.faces) for c in cads], dimension,
                                                    device=self.device)
            for c, g in zip(todo, grids):
                self._solid[c, dimension] = g.points
        return [self._solid[int(c), dimension] for c in class_ids]


def as_models(models, device="cuda"):
    """``YCBVideoModels`` (anything with ``get_cad`` / ``get_voxel_pitch``) or a ``{class_id: (vertices, faces)}``
    mapping -> the adapter the dataset works with."""
    if isinstance(models, _Adapter):
        return models
    if not hasattr(models, "get_cad"):
        models = MeshModels(models, device=device)
    return _Adapter(models, device)
