"""OctomapServer -- the map server's insert and grid publication, on the device.

``OctomapServer::insertScan`` and ``::publishGrids`` of the reference's ROS node
(ros/src/morefusion_ros/src/OctomapServer.cpp:283-455, :510-618) over the dense log-odds boxes of
``MultiInstanceOctreeMapping``; the kernels are csrc/occserver.hip (include/mfhip.h ``mf_occserver_*``).  See DESIGN.md
"Map server: shared free set, hit-only instance maps, grids in the sensor frame" for the model and every precision
choice.  The online path is frames -> ``InstanceTracker(server.mapping).track`` -> ``server.insert_scan`` ->
``server.publish_grids`` -> ``Model.predict`` -> ``IterativeCollisionCheckLink.refine_until_converged``
(examples/online_pose_refinement.py).  ``server.grids_in_map_frame`` feeds the render-service route of the tracker
(``contrib.render_voxel_grids``, ``InstanceTracker(render="mesh", server=server)``).

Host synchronisation per frame: the key bounds of the scan [n_trees, 6] and the per-instance statistics
[n_instances + 2, 10], read back together before the ray-cast.  ``publish_grids`` reads nothing back.
"""
import math

import numpy as np
import torch

from .. import _lib
from .multi_instance_octree_mapping import BACKGROUND_ID, MultiInstanceOctreeMapping

_MAX_TREES = 256  # mf_occserver_bounds / mf_occmap_bounds
_DIM = 32         # publishGrids: grid.dims = 32 x 32 x 32


def logodds(p):
    """OctoMap's ``logodds()``: float32(log(p / (1 - p)))."""
    return np.float32(math.log(p / (1 - p)))


class OctomapServer:
    """One background map (``BACKGROUND_ID``, pitch ``resolution``) that takes every ray's free cells, and one
    hit-only map per tracked instance id (>= 1) at its class pitch.

    ``mapping``: the ``MultiInstanceOctreeMapping`` the server owns and fills (``InstanceTracker(server.mapping)``
    renders these maps unchanged).  ``centers`` {id: float32 [3]}: the centroid of the instance's points in the first
    frame that had any, in the map frame; ``bbx`` {id: (min float32 [3], max float32 [3])}: the running bounds of its
    points.  Both also hold ``BACKGROUND_ID``, as the reference's maps hold -1."""

    def __init__(self, resolution=0.01, hit=0.7, miss=0.4, prob_min=0.12, prob_max=0.97, ground_as_noentry=True,
                 free_as_noentry=True, max_range=-1.0, device="cuda"):
        if max_range > 0:
            raise ValueError("max_range > 0 (truncated rays, OctomapServer.cpp:375-383) is not provided")
        if not resolution > 0:
            raise ValueError("resolution must be positive")
        self.resolution = float(resolution)
        self.prob_max = float(prob_max)
        self.lo_hit, self.lo_miss = logodds(hit), logodds(miss)
        self.lo_min, self.lo_max = logodds(prob_min), logodds(prob_max)
        self.ground_as_noentry, self.free_as_noentry = bool(ground_as_noentry), bool(free_as_noentry)
        self.mapping = MultiInstanceOctreeMapping(device=device)
        self.device = self.mapping.device
        self.class_ids, self.centers, self.bbx = {}, {}, {}

    def reset(self):
        """Forget every map (the mapping object stays the same one)."""
        m = self.mapping
        m._trees.clear()
        m._table = None
        m._overflow.zero_()
        self.class_ids.clear()
        self.centers.clear()
        self.bbx.clear()

    def insert_scan(self, pts_map, label_tracked, instance_id_to_class_id, pitch_of, origin=(0, 0, 0)):
        """``insertScan`` of one frame: ``pts_map`` [H,W,3] float32 in the MAP frame (``tracker.pts_map``) seen from
        ``origin``; ``label_tracked`` [H,W] with tracked ids >= 1, -1 = background, -2 = uncertain.  Only pixels with
        even row and even column and no NaN take part.  Every ray frees cells of the background map; a pixel's end
        point is one hit in its label's own map (and free in the background unless the label is -1)."""
        m = self.mapping
        get_pitch = pitch_of.__getitem__ if isinstance(pitch_of, dict) else pitch_of
        ids = sorted(int(i) for i in instance_id_to_class_id)
        if ids and ids[0] <= BACKGROUND_ID:
            raise ValueError("tracked instance ids must be >= 1")
        shape = tuple(label_tracked.shape)
        if len(shape) != 2 or tuple(pts_map.shape) != shape + (3,):
            raise ValueError("pts_map must be [H,W,3] and label_tracked [H,W]")
        H, W = shape
        if not isinstance(label_tracked, torch.Tensor):  # a host label is checked on the host; a device one by the kernel
            self._require_classes(np.unique(np.asarray(label_tracked)), ids)
        new = [i for i in ids if i not in m._trees]
        if len(m._trees) + len(new) + (BACKGROUND_ID not in m._trees) > _MAX_TREES:
            raise ValueError(f"at most {_MAX_TREES} maps")
        for i in new:
            m.initialize(i, pitch=get_pitch(int(instance_id_to_class_id[i])))
            self.class_ids[i] = int(instance_id_to_class_id[i])
        if BACKGROUND_ID not in m._trees:
            m.initialize(BACKGROUND_ID, pitch=self.resolution)
            self.class_ids[BACKGROUND_ID] = 0
        pts = m._points(pts_map)
        label = m._device(label_tracked).reshape(-1).to(torch.int32).contiguous()
        bg = m._index(BACKGROUND_ID)
        slot_ids = ids + [BACKGROUND_ID]
        slots = m._slots([(i, m._index(i), 0) for i in ids] + [(-1, bg, 0)])
        n_slots, n_trees = len(slot_ids), len(m._trees)
        L = _lib.lib()
        bounds = torch.empty((n_trees, 6), dtype=torch.int32, device=self.device)
        table = torch.empty((n_slots + 1, 10), dtype=torch.float64, device=self.device)
        _lib.check(L.mf_occserver_bounds(pts.data_ptr(), label.data_ptr(), H, W, slots.data_ptr(), n_slots,
                                         m._descs().data_ptr(), bg, n_trees, bounds.data_ptr(), _lib.stream_ptr()),
                   "mf_occserver_bounds")
        _lib.check(L.mf_occserver_stats(pts.data_ptr(), label.data_ptr(), H, W, slots.data_ptr(), n_slots,
                                        table.data_ptr(), _lib.stream_ptr()), "mf_occserver_stats")
        bounds, table = bounds.cpu().numpy(), table.cpu().numpy()  # the frame's read-back
        if table[n_slots, 0] >= 0:
            self._require_classes([int(table[n_slots, 0])], ids)
        m._fit(bounds, origin, origin_trees=(bg,))  # only the background map holds rays
        o = [float(np.float32(c)) for c in _lib.as_float3(origin)]
        _lib.check(L.mf_occserver_raycast(pts.data_ptr(), label.data_ptr(), H, W, slots.data_ptr(), n_slots,
                                          m._descs().data_ptr(), bg, *o, m._overflow.data_ptr(), _lib.stream_ptr()),
                   "mf_occserver_raycast")
        cells = [t.dim[0] * t.dim[1] * t.dim[2] for t in m._trees.values()]
        _lib.check(L.mf_occserver_apply(m._descs().data_ptr(), n_trees, max(cells), float(self.lo_hit),
                                        float(self.lo_miss), float(self.lo_min), float(self.lo_max),
                                        _lib.stream_ptr()), "mf_occserver_apply")
        for i, row in zip(slot_ids, table):
            if row[0] < 1:
                continue
            lo, hi = row[4:7].astype(np.float32), row[7:10].astype(np.float32)
            if i in self.bbx:
                lo, hi = np.minimum(self.bbx[i][0], lo), np.maximum(self.bbx[i][1], hi)
            self.bbx[i] = (lo, hi)
            self.centers.setdefault(i, row[1:4].astype(np.float32))  # centers_.insert: the first one stays

    def publish_grids(self, T_sensor_to_map):
        """``publishGrids``: for every instance with a centre, in ascending id, the 32^3 grids in the SENSOR frame
        around its centre.  -> dict(instance_ids, class_ids (lists), pitch [B] float32, origin [B,3] float64,
        grid_target / grid_noentry [B,32,32,32] float32, grid_nontarget_empty [B,32,32,32] bool), device tensors."""
        m = self.mapping
        T = np.asarray(T_sensor_to_map.cpu() if isinstance(T_sensor_to_map, torch.Tensor) else T_sensor_to_map, np.float64)
        if T.shape != (4, 4):
            raise ValueError("T_sensor_to_map must be [4,4]")
        inv = np.eye(4)
        inv[:3, :3] = T[:3, :3].T
        inv[:3, 3] = -T[:3, :3].T @ T[:3, 3]
        ids = sorted(i for i in m._trees if i != BACKGROUND_ID and i in self.centers)
        B = len(ids)
        dev = self.device
        dims = (B, _DIM, _DIM, _DIM)
        out = dict(instance_ids=ids, class_ids=[self.class_ids[i] for i in ids],
                   pitch=torch.tensor([m._trees[i].resolution for i in ids], dtype=torch.float64).to(torch.float32).to(dev),
                   origin=torch.zeros((B, 3), dtype=torch.float64, device=dev),
                   grid_target=torch.empty(dims, dtype=torch.float32, device=dev),
                   grid_noentry=torch.empty(dims, dtype=torch.float32, device=dev),
                   grid_nontarget_empty=torch.empty(dims, dtype=torch.bool, device=dev))
        if B == 0:
            return out
        order = torch.tensor([m._index(i) for i in sorted(m._trees)], dtype=torch.int32).to(dev)
        target = torch.tensor([m._index(i) for i in ids], dtype=torch.int32).to(dev)
        centers = torch.from_numpy(np.stack([self.centers[i] for i in ids]).astype(np.float32)).to(dev)
        Ts = torch.from_numpy(np.stack([inv, T]).astype(np.float32)).to(dev)  # float64 on the host, rounded once
        flags = (1 if self.ground_as_noentry else 0) | (2 if self.free_as_noentry else 0)
        _lib.check(_lib.lib().mf_occserver_publish(
            m._descs().data_ptr(), len(m._trees), order.data_ptr(), m._index(BACKGROUND_ID), target.data_ptr(),
            out["pitch"].data_ptr(), centers.data_ptr(), Ts[0].data_ptr(), Ts[1].data_ptr(), self.prob_max, flags, B,
            _DIM, out["origin"].data_ptr(), out["grid_target"].data_ptr(), out["grid_noentry"].data_ptr(),
            out["grid_nontarget_empty"].data_ptr(), _lib.stream_ptr()), "mf_occserver_publish")
        return out

    def grids_in_map_frame(self):
        """``getGridsInWorldFrame`` (OctomapServer.cpp:456-508): for every instance with a centre, in ascending id, the
        32^3 samples of its OWN map around its centre, in the MAP frame.  -> dict(instance_ids, class_ids (lists),
        pitch [B] float32, origin [B,3] float64 = centre - 15.5 pitch, grid [B,32,32,32] float32: the occupancy where it
        is > 0.5, else 0), device tensors.  What ``contrib.render_voxel_grids`` meshes; nothing is read back."""
        m = self.mapping
        ids = sorted(i for i in m._trees if i != BACKGROUND_ID and i in self.centers)
        B = len(ids)
        dev = self.device
        out = dict(instance_ids=ids, class_ids=[self.class_ids[i] for i in ids],
                   pitch=torch.tensor([m._trees[i].resolution for i in ids], dtype=torch.float64).to(torch.float32).to(dev),
                   origin=torch.zeros((B, 3), dtype=torch.float64, device=dev),
                   grid=torch.empty((B, _DIM, _DIM, _DIM), dtype=torch.float32, device=dev))
        if B == 0:
            return out
        target = torch.tensor([m._index(i) for i in ids], dtype=torch.int32).to(dev)
        centers = torch.from_numpy(np.stack([self.centers[i] for i in ids]).astype(np.float32)).to(dev)
        _lib.check(_lib.lib().mf_occserver_map_grids(
            m._descs().data_ptr(), len(m._trees), target.data_ptr(), out["pitch"].data_ptr(), centers.data_ptr(), B,
            _DIM, out["origin"].data_ptr(), out["grid"].data_ptr(), _lib.stream_ptr()), "mf_occserver_map_grids")
        return out

    @staticmethod
    def _require_classes(labels, ids):
        for u in labels:
            if int(u) >= 0 and int(u) not in ids:
                raise KeyError(f"label {int(u)} has no class in instance_id_to_class_id")
