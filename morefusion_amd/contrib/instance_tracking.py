"""InstanceTracker -- stable instance ids across frames, on the device.

The per-frame loop of the reference's map server (ros/src/morefusion_ros/src/OctomapServer.cpp:95-191):
render the instance maps into the current camera (``render``, :193-281), match the detector's per-frame ids
against that rendering (utils/geometry.h:79-281, ``track_instance_id``), then insert the scan under the tracked
ids (``MultiInstanceOctreeMapping.integrate_tracked_frame``).  Every step runs in csrc/occtrack.hip
(include/mfhip.h ``mf_occtrack_*``); see DESIGN.md "Instance tracking" for the restatements and what is unpinned.

Ids: tracked instance ids are >= 1 (the counter starts behind the largest id the mapping holds); id 0 is the
mapping's background map and is never rendered.  In label images -1 is background and -2 uncertain.

Host synchronisation: ``track`` reads back ONE small int32 array per frame -- the remap table of the
detections plus the updated counter -- because the host has to name the new maps.

Inputs may be NumPy arrays or torch tensors; results come back as the same kind.
"""
import numpy as np
import torch

from .. import _lib
from .multi_instance_octree_mapping import BACKGROUND_ID

# the reference's constants (geometry.h:66-69, :179, :232-233); ``band`` is half the contour thickness of 10
DEFAULT_THRESHOLDS = dict(min_mask=40, min_bbox=80, min_side=60, iou=0.4, coverage=0.9, min_area=400, band=5)


def _ids(device, ids):
    return torch.tensor(list(ids) or [0], dtype=torch.int32).to(device)


def _image(device, x):
    if isinstance(x, torch.Tensor):
        x = x.detach().to(device)
    else:
        x = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if x.dim() != 2:
        raise ValueError("a label image must be [H, W]")
    return x.to(torch.int32).contiguous()


def _workspace(device, H, W, n_ref):
    n = _lib.lib().mf_occtrack_workspace_bytes(H, W, n_ref)
    if n < 0:
        raise ValueError("image or id list too large")
    return torch.empty(n, dtype=torch.uint8, device=device)


def transform_points(pcd, T_sensor_to_map, device="cuda"):
    """[..., 3] points of the sensor frame -> float32 device tensor [N, 3] in the map frame (NaN rows stay NaN)."""
    device = torch.device(device)
    x = pcd.detach().to(device) if isinstance(pcd, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pcd)).to(device)
    if x.shape[-1] != 3:
        raise ValueError("points must have 3 coordinates in the last axis")
    x = x.reshape(-1, 3).to(torch.float32).contiguous()
    _lib.require_gpu(x)
    T = torch.from_numpy(np.asarray(T_sensor_to_map, np.float32).reshape(4, 4).copy()).to(device)
    out = torch.empty_like(x)
    _lib.check(_lib.lib().mf_occtrack_transform(x.data_ptr(), T.data_ptr(), x.shape[0], out.data_ptr(), _lib.stream_ptr()),
               "mf_occtrack_transform")
    return out


def render_instance_maps(mapping, pts_map, K, T_sensor_to_map, height, width, instance_ids=None):
    """``OctomapServer::render``: (label_rendered [H,W] int32, depth_rendered [H,W] float32) device tensors of the
    mapping's instance maps (all but the background, ascending id = slot order) seen through ``pts_map`` [H*W,3]
    (float32 device tensor in the map frame) from the sensor at ``T_sensor_to_map[:3, 3]``."""
    device = mapping.device
    _lib.require_gpu(pts_map)
    H, W = int(height), int(width)
    if pts_map.shape != (H * W, 3) or pts_map.dtype != torch.float32 or not pts_map.is_contiguous():
        raise ValueError("pts_map must be a contiguous float32 [H*W, 3] tensor")
    ids = sorted(i for i in mapping.instance_ids if i != BACKGROUND_ID) if instance_ids is None else list(instance_ids)
    slots = torch.tensor([[mapping._index(i), i] for i in ids] or [[0, 0]], dtype=torch.int32).to(device)
    T = np.asarray(T_sensor_to_map, np.float32).reshape(4, 4)
    Kd = torch.from_numpy(np.asarray(K, np.float32).reshape(3, 3).copy()).to(device)
    Td = torch.from_numpy(T.copy()).to(device)
    label = torch.empty((H, W), dtype=torch.int32, device=device)
    depth = torch.empty((H, W), dtype=torch.float32, device=device)
    ws = _workspace(device, H, W, len(ids))
    _lib.check(_lib.lib().mf_occtrack_render(
        pts_map.data_ptr(), Kd.data_ptr(), Td.data_ptr(), float(T[0, 3]), float(T[1, 3]), float(T[2, 3]),
        mapping._descs().data_ptr(), slots.data_ptr(), len(ids), H, W, ws.data_ptr(), label.data_ptr(),
        depth.data_ptr(), _lib.stream_ptr()), "mf_occtrack_render")
    return label, depth


def render_voxel_grids(grids, depth, K, T_sensor_to_map, height, width):
    """The reference's render service (ros/src/morefusion_ros/nodes/render_voxel_grids.py): ``grids`` (the dict of
    ``OctomapServer.grids_in_map_frame``) -> meshes (``geometry.voxel_grids_to_meshes``) -> one composite render seen
    through the inverse of ``T_sensor_to_map`` with the instance ids (``geometry.render_meshes``) -> the label test
    against the sensor ``depth`` [H,W] float32 (NaN = no reading) with its 1 cm margin.  Returns the [H,W] int32 device
    label: the instance id, -2 where nothing was drawn or the surface lies behind the reading.  A grid without an
    occupied cell is skipped (:61-62); with none left every pixel is -2."""
    from ..geometry import grid_mesh, render_meshes
    H, W = int(height), int(width)
    grid = grids["grid"]
    dev = grid.device if isinstance(grid, torch.Tensor) else torch.device("cuda")
    meshes = grid_mesh.voxel_grids_to_meshes(grid, grids["pitch"], grids["origin"], device=dev)
    keep = [i for i, (_, f) in enumerate(meshes) if f.shape[0]]
    if not keep:
        return torch.full((H, W), -2, dtype=torch.int32, device=dev)
    T = np.asarray(T_sensor_to_map.cpu() if isinstance(T_sensor_to_map, torch.Tensor) else T_sensor_to_map, np.float64)
    T_map_to_sensor = np.linalg.inv(T.reshape(4, 4))
    Kh = np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K, np.float64).reshape(3, 3)
    out = render_meshes([meshes[i] for i in keep], np.stack([T_map_to_sensor] * len(keep)), Kh, H, W,
                        instance_ids=[int(grids["instance_ids"][i]) for i in keep], device=dev)
    return grid_mesh.label_of_render(out["depth"][0], out["instance"][0], depth)


def track_instance_ids(label_rendered, label_detected, ref_ids, det_ids, counter, thresholds=None):
    """``track_instance_id`` on two [H,W] int32 device images.  ``ref_ids`` / ``det_ids``: the ids that may occur in
    the rendered / detected image; ``counter``: int32 device tensor [1], advanced in place.  Returns a dict of device
    tensors: ``remap`` [n_det + 1] (tracked id per detection in ascending detection id, -2 = suspicious; last = the
    counter), ``suspicious_ref`` [n_ref], ``suspicious_det`` [n_det] (1 = edge rule, 2 = size rule), ``stats``,
    ``label_tracked``, ``label_reference`` (both cleaned) and ``label_merged``."""
    th = dict(DEFAULT_THRESHOLDS, **(thresholds or {}))
    _lib.require_gpu(label_rendered, label_detected, counter)
    device = label_rendered.device
    H, W = label_rendered.shape
    if label_detected.shape != (H, W):
        raise ValueError("label_rendered and label_detected differ in size")
    ref_ids, det_ids = sorted(int(i) for i in ref_ids), sorted(int(i) for i in det_ids)
    if min(ref_ids + det_ids + [0]) < 0 or len(set(ref_ids)) != len(ref_ids) or len(set(det_ids)) != len(det_ids):
        raise ValueError("ids must be distinct and non-negative")
    n_ref, n_det = len(ref_ids), len(det_ids)
    L = _lib.lib()
    rid, did = _ids(device, ref_ids), _ids(device, det_ids)
    n_stats = L.mf_occtrack_stats_elems(n_ref, n_det)
    if n_stats < 0:
        raise ValueError("too many ids")
    i32 = dict(dtype=torch.int32, device=device)
    stats = torch.empty(n_stats, **i32)
    remap = torch.empty(n_det + 1, **i32)
    susp_ref, susp_det = torch.empty(max(n_ref, 1), **i32), torch.empty(max(n_det, 1), **i32)
    tracked, reference, tracked_c, reference_c, merged = (torch.empty((H, W), **i32) for _ in range(5))
    ws = _workspace(device, H, W, n_ref)
    s = _lib.stream_ptr()
    rendered, detected = label_rendered.contiguous(), label_detected.contiguous()
    _lib.check(L.mf_occtrack_overlap(rendered.data_ptr(), detected.data_ptr(), H, W, rid.data_ptr(), n_ref,
                                     did.data_ptr(), n_det, stats.data_ptr(), s), "mf_occtrack_overlap")
    _lib.check(L.mf_occtrack_assign(stats.data_ptr(), rid.data_ptr(), n_ref, n_det, H, W, int(th["min_mask"]),
                                    int(th["min_bbox"]), int(th["min_side"]), float(th["iou"]), float(th["coverage"]),
                                    counter.data_ptr(), remap.data_ptr(), susp_ref.data_ptr(), susp_det.data_ptr(), s),
               "mf_occtrack_assign")
    _lib.check(L.mf_occtrack_relabel(rendered.data_ptr(), detected.data_ptr(), H, W, rid.data_ptr(), n_ref,
                                     did.data_ptr(), n_det, remap.data_ptr(), susp_ref.data_ptr(), tracked.data_ptr(),
                                     reference.data_ptr(), s), "mf_occtrack_relabel")
    for src, dst in ((tracked, tracked_c), (reference, reference_c)):
        _lib.check(L.mf_occtrack_clean(src.data_ptr(), H, W, int(th["min_area"]), int(th["band"]), ws.data_ptr(),
                                       dst.data_ptr(), s), "mf_occtrack_clean")
    _lib.check(L.mf_occtrack_merge(reference_c.data_ptr(), tracked_c.data_ptr(), H, W, rid.data_ptr(), n_ref,
                                   ws.data_ptr(), merged.data_ptr(), s), "mf_occtrack_merge")
    return dict(remap=remap, suspicious_ref=susp_ref[:n_ref], suspicious_det=susp_det[:n_det], stats=stats,
                label_tracked=tracked_c, label_reference=reference_c, label_merged=merged, ref_ids=ref_ids,
                det_ids=det_ids)


class InstanceTracker:
    """Carries instance ids from frame to frame over a ``MultiInstanceOctreeMapping``."""

    def __init__(self, mapping, thresholds=None, render="raycast", server=None):
        """``render="raycast"``: the maps are ray-cast per pixel (``render_instance_maps``).  ``render="mesh"``: the
        reference's render-service route -- ``server.grids_in_map_frame()`` meshed and rasterised
        (``render_voxel_grids``); it needs the ``OctomapServer`` that owns ``mapping`` and a ``depth`` in ``track``."""
        if render not in ("raycast", "mesh"):
            raise ValueError('render must be "raycast" or "mesh"')
        if render == "mesh" and (server is None or server.mapping is not mapping):
            raise ValueError('render="mesh" needs server=, the OctomapServer that owns the mapping')
        self.render, self.server = render, server
        self.mapping = mapping
        self.thresholds = dict(DEFAULT_THRESHOLDS, **(thresholds or {}))
        first = max([i for i in mapping.instance_ids] + [BACKGROUND_ID]) + 1
        self.counter = torch.tensor([first], dtype=torch.int32).to(mapping.device)  # lives on the device
        self.class_ids = {}       # tracked instance id -> class id, every id seen so far
        self.pts_map = None       # the last frame's points in the map frame, float32 device [H*W, 3]
        self.last = None          # the last frame's track_instance_ids result

    def track(self, pcd, label_detected, class_ids_by_detection, K, T_sensor_to_map, depth=None):
        """One frame: ``pcd`` [H,W,3] in the sensor frame (NaN holes), ``label_detected`` [H,W] the detector's
        instance label (< 0: none), ``class_ids_by_detection`` {detection id: class id}; ``depth`` [H,W] float32, the
        sensor depth (NaN = no reading), for ``render="mesh"`` only.  Returns (label_tracked,
        label_merged, instance_id_to_class_id, label_rendered); the images as NumPy arrays for NumPy inputs, device
        tensors otherwise.  ``self.pts_map`` is what ``integrate_tracked_frame`` takes next."""
        as_tensor = isinstance(pcd, torch.Tensor) or isinstance(label_detected, torch.Tensor)
        device = self.mapping.device
        detected = _image(device, label_detected)
        H, W = detected.shape
        self.pts_map = transform_points(pcd, T_sensor_to_map, device)
        if self.pts_map.shape[0] != H * W:
            raise ValueError("pcd and label_detected differ in size")
        ref_ids = sorted(i for i in self.mapping.instance_ids if i != BACKGROUND_ID)
        if self.render == "mesh":
            if depth is None:
                raise ValueError('render="mesh" needs the sensor depth')
            rendered = render_voxel_grids(self.server.grids_in_map_frame(), depth, K, T_sensor_to_map, H, W)
        else:
            rendered, _ = render_instance_maps(self.mapping, self.pts_map, K, T_sensor_to_map, H, W, ref_ids)
        det = {int(k): int(v) for k, v in dict(class_ids_by_detection).items()}
        out = track_instance_ids(rendered, detected, ref_ids, det, self.counter, self.thresholds)
        remap = out["remap"].cpu().numpy()  # the frame's one read-back: [n_det] tracked ids + the counter
        for d, tid in zip(out["det_ids"], remap[:-1]):
            if tid != -2:
                self.class_ids[int(tid)] = det[d]  # (a matched id takes the detector's current class, as :113-118)
        out["remap_host"] = remap
        self.last = out
        images = (out["label_tracked"], out["label_merged"], rendered)
        if not as_tensor:
            images = tuple(x.cpu().numpy() for x in images)
        return images[0], images[1], dict(self.class_ids), images[2]
