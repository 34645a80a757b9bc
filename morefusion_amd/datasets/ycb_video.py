"""YCBVideoModels -- morefusion/datasets/ycb_video/models.py over meshes already on disk.

The reference downloads YCB_Video_Models, voxelizes each ``textured_simple.obj`` with binvox and takes
trimesh's signed distance; here the root directory is given, nothing is downloaded, and the solid grid and
the signed distance come from csrc/meshsdf.hip (``geometry.mesh_sdf``).  Layout: ``<root>/<NNN_name>/``
holding ``textured_simple.obj`` (or ``textured.obj``) and optionally ``points.xyz``; the class names are the
sorted ``NNN_name`` directories, class id = index + 1 (``__background__`` is 0).  ``get_sdf`` reads and
writes ``<root>/<NNN_name>/sdf.npz`` with the reference's keys (``points``, ``sdf``), so either side's cache
loads in the other.
"""
import pathlib
import re
import warnings

import numpy as np
import torch

from ..extra import _open3d
from ..geometry import mesh_sdf

_CLASS_DIR = re.compile(r"^\d{3}_\w+$")
_CAD_FILES = ("textured_simple.obj", "textured.obj")


class YCBVideoModels:

    def __init__(self, root_dir, device=None):
        self.root_dir = pathlib.Path(root_dir)
        if not self.root_dir.is_dir():
            raise FileNotFoundError(
                f"{self.root_dir}: no such model directory; expected <root>/<NNN_name>/textured_simple.obj "
                "(or textured.obj), one directory per class (e.g. 002_master_chef_can). Nothing is downloaded.")
        names = sorted(p.name for p in self.root_dir.iterdir() if p.is_dir() and _CLASS_DIR.match(p.name))
        if not names:
            raise FileNotFoundError(f"{self.root_dir}: no <NNN_name> class directories")
        self._class_names = ["__background__"] + names
        self._device = torch.device(device) if device is not None else torch.device("cuda")
        self._cad_cache, self._pcd_cache, self._sdf_cache, self._bbox_diagonal_cache = {}, {}, {}, {}

    @property
    def class_names(self):
        return self._class_names

    def _name(self, class_id):
        class_id = int(class_id)
        if not 1 <= class_id < len(self._class_names):
            raise IndexError(f"class_id {class_id} outside 1..{len(self._class_names) - 1}")
        return self._class_names[class_id]

    def get_cad_file(self, class_id):
        d = self.root_dir / self._name(class_id)
        for f in _CAD_FILES:
            if (d / f).exists():
                return d / f
        raise FileNotFoundError(f"{d}: neither of {', '.join(_CAD_FILES)}")

    def get_pcd_file(self, class_id):
        return self.root_dir / self._name(class_id) / "points.xyz"

    def _get_sdf_file(self, class_id):
        return self.root_dir / self._name(class_id) / "sdf.npz"

    def get_cad(self, class_id):
        """The CAD mesh: TriangleMesh(vertices float64 [V, 3], faces int32 [F, 3])."""
        name = self._name(class_id)
        if name not in self._cad_cache:
            self._cad_cache[name] = mesh_sdf.TriangleMesh(*mesh_sdf.load_obj(self.get_cad_file(class_id)))
        return self._cad_cache[name]

    def get_pcd(self, class_id):
        name = self._name(class_id)
        if name not in self._pcd_cache:
            f = self.get_pcd_file(class_id)
            if not f.exists():
                raise FileNotFoundError(f"{f}: no points.xyz for class {name} (get_sdf's points are the solid cloud)")
            self._pcd_cache[name] = np.loadtxt(f)
        return self._pcd_cache[name]

    def get_bbox_diagonal(self, class_id):
        name = self._name(class_id)
        if name not in self._bbox_diagonal_cache:
            v = self.get_cad(class_id).vertices
            extents = v.max(axis=0) - v.min(axis=0)
            self._bbox_diagonal_cache[name] = float(np.sqrt((extents ** 2).sum()))
        return self._bbox_diagonal_cache[name]

    def get_voxel_pitch(self, dimension, class_id):
        return 1.0 * self.get_bbox_diagonal(class_id) / dimension

    def get_solid_voxel_grid(self, class_id, dimension=64):
        """The solid grid of the CAD model (binvox ``-d 64`` in the reference): SolidVoxelGrid of NumPy arrays."""
        cad = self.get_cad(class_id)
        return mesh_sdf.solid_voxel_grid(cad.vertices, cad.faces, dimension, device=self._device)

    def get_sdf(self, class_id):
        """(points [n, 3], sdf [n]) float64: the solid grid's centres down-sampled at get_voxel_pitch(32) and their
        signed distance (positive inside).  Cached in memory and in sdf.npz."""
        return self.get_sdf_batch([class_id])[0]

    def get_sdf_batch(self, class_ids):
        """get_sdf of many classes: one solid-grid launch and one signed-distance launch for all the classes that
        are not cached (the down-sampling between them runs once per class: each has its own pitch)."""
        todo = []
        for cid in class_ids:
            name = self._name(cid)
            if name in self._sdf_cache:
                continue
            f = self._get_sdf_file(cid)
            if f.exists():
                data = np.load(f)
                self._sdf_cache[name] = (data["points"], data["sdf"])
            elif cid not in todo:
                todo.append(int(cid))
        if todo:
            cads = [self.get_cad(c) for c in todo]
            grids = mesh_sdf.solid_voxel_grid_batch([(c.vertices, c.faces) for c in cads], 64, device=self._device)
            points = [_open3d.voxel_down_sample(g.points, self.get_voxel_pitch(32, c)) for g, c in zip(grids, todo)]
            res = mesh_sdf.mesh_signed_distance_batch([(c.vertices, c.faces) for c in cads], points,
                                                      outputs=("sdf",), device=self._device)
            for c, p, r in zip(todo, points, res):
                pts, sdf = p.cpu().numpy(), r["sdf"].cpu().numpy()
                self._sdf_cache[self._name(c)] = (pts, sdf)
                try:
                    np.savez_compressed(self._get_sdf_file(c), points=pts, sdf=sdf)
                except OSError as e:  # a read-only model tree: computed again next time
                    warnings.warn(f"could not cache {self._get_sdf_file(c)}: {e}")
        return [self._sdf_cache[self._name(c)] for c in class_ids]
