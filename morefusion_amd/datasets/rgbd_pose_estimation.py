"""RGBDPoseEstimationDatasetBase -- morefusion/datasets/rgbd_pose_estimation/base.py on the device.

``get_example`` turns one frame with ground-truth poses (``get_frame``: rgb, depth, instance_label,
intrinsic_matrix, instance_ids, class_ids, Ts_cad2cam) into the reference's list of per-object example dicts.
The reference walks the instances on the host (crop, centerize, one pybullet render, one OctoMap query, two
scatter loops each); here the frame is composed from the package's batched pieces -- ``instance_crops``,
``MultiInstanceOctreeMapping.integrate_frame`` / ``get_target_grids_batch``, ``grid_origin``, one
``render_meshes`` launch for every ``mask_rend`` and one ``full_grids`` launch for every ``*_full`` grid -- and
the results come back as NumPy in one copy per array.
"""
import numpy as np
import torch

from .. import geometry
from ..contrib import MultiInstanceOctreeMapping
from ..extra._render import fovy_intrinsics
from .models_adapter import as_models


def _quaternion_matrix(q):
    """trimesh.transformations.quaternion_matrix: (w, x, y, z) -> 4 x 4."""
    q = np.array(q, np.float64)
    n = q @ q
    if n < np.finfo(np.float64).eps * 4.0:
        return np.eye(4)
    q = q * np.sqrt(2.0 / n)
    q = np.outer(q, q)
    return np.array([
        [1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0], 0.0],
        [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0], 0.0],
        [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2], 0.0],
        [0.0, 0.0, 0.0, 1.0]])


class RGBDPoseEstimationDatasetBase:

    _n_points_minimal = 1
    _image_size = 256
    _voxel_dim = 32
    _solid_dim = 64  # the CAD models' solid grid (binvox -d 64 in the reference)

    def __init__(self, models, class_ids=None, device="cuda"):
        self._device = torch.device(device)
        self._models = as_models(models, self._device)
        if class_ids is not None:
            class_ids = tuple(class_ids)
        self._class_ids = class_ids
        self._ids = []  # one image id per frame (datasets.reindex names the example files after them)

    def __len__(self):
        if self._ids:
            return len(self._ids)
        raise NotImplementedError

    def get_frame(self, index):
        """-> dict(rgb u8 [H, W, 3], depth f32 [H, W] (NaN invalid), instance_label i32 [H, W], intrinsic_matrix
        [3, 3], instance_ids [n], class_ids [n], Ts_cad2cam [n, 4, 4]); ``label`` / ``K`` are accepted for
        ``instance_label`` / ``intrinsic_matrix`` (the synthetic frames' names)."""
        raise NotImplementedError

    def _pitch(self, class_id):
        return self._models.get_voxel_pitch(self._voxel_dim, int(class_id))

    def build_octomap(self, pcd, instance_label, instance_ids, class_ids):
        """base.py:30-50: a map per foreground instance at its class pitch, the rest into map 0 at 0.01."""
        mapping = MultiInstanceOctreeMapping(device=self._device)
        dev = lambda x: torch.as_tensor(x).to(self._device)  # noqa: E731
        mapping.integrate_frame(dev(pcd).to(torch.float32), dev(instance_label), instance_ids, class_ids, self._pitch)
        return mapping

    def get_example(self, index):
        frame = self.get_frame(index)
        instance_ids = np.asarray(frame["instance_ids"]).reshape(-1)
        class_ids = np.asarray(frame["class_ids"]).reshape(-1)
        label_h = frame["instance_label"] if "instance_label" in frame else frame["label"]
        K = np.asarray(frame["intrinsic_matrix"] if "intrinsic_matrix" in frame else frame["K"], np.float64)
        Ts_cad2cam = np.asarray(frame["Ts_cad2cam"], np.float64).reshape(-1, 4, 4)
        if instance_ids.size == 0:
            return []
        dev = lambda x: torch.as_tensor(x).to(self._device)  # noqa: E731
        rgb, depth, label = dev(frame["rgb"]), dev(frame["depth"]).to(torch.float32), dev(label_h).to(torch.int32)
        H, W = depth.shape
        pcd_full = geometry.pointcloud_from_depth(depth.cpu().numpy(), fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2])
        mapping = self.build_octomap(pcd_full, label, instance_ids, class_ids)

        crops = geometry.instance_crops(rgb, depth, K, label, instance_ids.astype(np.int32),
                                        image_size=self._image_size, min_valid=max(int(self._n_points_minimal), 1))
        keep = crops["keep"].cpu().numpy()
        bbox = crops["bbox"].cpu().numpy()
        sel = []
        for k, class_id in enumerate(class_ids):
            if class_id == 0:
                continue
            if self._class_ids and class_id not in self._class_ids:
                continue
            y1, x1, y2, x2 = bbox[k]
            if (y2 - y1) * (x2 - x1) == 0:
                continue
            if not keep[k]:  # fewer than _n_points_minimal valid points
                continue
            sel.append(k)
        if not sel:
            return []
        sel_t = torch.as_tensor(sel, device=self._device)
        ids, classes, Ts = instance_ids[sel], class_ids[sel], Ts_cad2cam[sel]
        rgb_ins, pcd_ins = crops["rgb"][sel_t], crops["pcd"][sel_t].to(torch.float64)
        pitch = torch.tensor([self._pitch(c) for c in classes], dtype=torch.float64, device=self._device)
        origin = geometry.grid_origin(pcd_ins, pitch, dim=self._voxel_dim)
        dims = (self._voxel_dim,) * 3
        grid_target, grid_nontarget, grid_empty = mapping.get_target_grids_batch(ids, pitch, origin, dimensions=dims)

        # visibility = mask.sum() / mask_rend.sum(): every CAD model alone at its pose, one image each, through
        # the frustum render_cad builds from fovy = camera.fov[1] (principal point at the image centre)
        fovy = np.degrees(2.0 * np.arctan(H / 2.0 / K[1, 1]))
        cads = [self._models.get_cad(c) for c in dict.fromkeys(int(c) for c in classes)]
        slot = {c: m for m, c in enumerate(dict.fromkeys(int(c) for c in classes))}
        rend = geometry.render_meshes([(c.vertices, c.faces) for c in cads], Ts, fovy_intrinsics(fovy, H, W), H, W,
                                      targets=list(range(len(sel))), mesh_index=[slot[int(c)] for c in classes],
                                      device=self._device)
        mask_sum = (label[None] == dev(ids.astype(np.int32))[:, None, None]).sum(dim=(1, 2))

        quaternion_true = np.stack([geometry.quaternion_from_matrix(T) for T in Ts])
        translation_true = np.stack([geometry.translation_from_matrix(T) for T in Ts])
        T_true = np.stack([_quaternion_matrix(q) for q in quaternion_true])
        T_true[:, :3, 3] = translation_true
        points = self._models.solid_points(classes, self._solid_dim)
        target_full, nontarget_full = geometry.full_grids(points, T_true, pitch, origin, dim=self._voxel_dim,
                                                          device=self._device)

        host = lambda t: t.cpu().numpy()  # noqa: E731
        rgb_ins, pcd_ins, pitch_h, origin_h = host(rgb_ins), host(pcd_ins), host(pitch), host(origin)
        grid_target, grid_nontarget, grid_empty = host(grid_target), host(grid_nontarget), host(grid_empty)
        target_full, nontarget_full = host(target_full), host(nontarget_full)
        mask_sum, rend_sum = host(mask_sum), host(rend["count"])
        examples = []
        for k in range(len(sel)):
            with np.errstate(invalid="ignore", divide="ignore"):
                visibility = 1.0 * mask_sum[k] / rend_sum[k]
            examples.append(dict(
                class_id=classes[k], rgb=rgb_ins[k], pcd=pcd_ins[k], quaternion_true=quaternion_true[k],
                translation_true=translation_true[k], visibility=visibility, origin=origin_h[k], pitch=pitch_h[k],
                grid_target=grid_target[k], grid_nontarget=grid_nontarget[k], grid_empty=grid_empty[k],
                grid_target_full=target_full[k], grid_nontarget_full=nontarget_full[k]))
        return examples
