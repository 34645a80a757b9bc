"""MultiInstanceOctreeMapping -- per-instance occupancy maps of RGB-D scans, on the device.

Call surface of morefusion/contrib/multi_instance_octree_mapping.py:6-94 (one OctoMap ``OcTree``
per instance) and the frame driver ``RGBDPoseEstimationDatasetBase.build_octomap``
(datasets/rgbd_pose_estimation/base.py:28-46) as ``integrate_frame``.  The maps are dense float32
log-odds boxes over OctoMap's keys (NaN = unknown) and every update runs in csrc/occmap.hip
(include/mfhip.h ``mf_occmap_*``); see DESIGN.md "Occupancy mapping" for the representation and
the precision contract.

Host synchronisation: each integrate batch (``integrate``, ``update``, ``integrate_frame``) reads
back ONE small int32 array -- the key bounds of the scan per instance, [n_instances, 6] -- to grow
the boxes before the ray-cast; ``integrate_frame`` with a device label image reads back its
distinct labels as well (``torch.unique``).  Everything else is asynchronous on the current stream.

Inputs may be NumPy arrays or torch tensors; results come back as the same kind (NumPy for NumPy
inputs, device tensors otherwise).  The maps always live on ``device``.
"""
import math

import numpy as np
import torch

from .. import _lib

_KEY_MAX = 32768  # octomap's tree_max_val
_MAX_SCANS = 32   # scan bits per cell and launch
BACKGROUND_ID = 0  # the background map of integrate_frame / integrate_tracked_frame (pitch 0.01)


def _key(c, res_factor):
    """OcTreeBaseImpl::coordToKey of a float32-rounded coordinate; None outside the 16-bit key range."""
    s = math.floor(float(np.float32(c)) * res_factor)
    return s + _KEY_MAX if -_KEY_MAX <= s < _KEY_MAX else None


class _Tree:
    def __init__(self, pitch):
        self.resolution = float(pitch)
        self.res_factor = 1.0 / self.resolution
        self.lo = None            # key of cell 0, [3] ints (None: nothing mapped yet)
        self.dim = (0, 0, 0)
        self.logodds = None       # [dim] float32, NaN = unknown
        self.bits = None          # [cells, 2] int32 (uint32 words): scan bits / hit counts, zero between calls

    def desc(self):
        d = _lib.OccTree()
        d.logodds = _lib.ptr(self.logodds)
        d.bits = _lib.ptr(self.bits)
        d.lo[:] = list(self.lo) if self.lo is not None else [0, 0, 0]
        d.dim[:] = list(self.dim)
        d.resolution = self.resolution
        d.res_factor = self.res_factor
        return d


def _is_tensor(*xs):
    return any(isinstance(x, torch.Tensor) for x in xs)


class MultiInstanceOctreeMapping:
    """One occupancy map per instance id (insertion order is the order ``get_target_grids`` visits)."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._trees = {}
        self._table = None        # device array of mfOccTree, rebuilt when a box changes
        self._overflow = torch.zeros(1, dtype=torch.int32, device=self.device)  # keys outside a box: stays 0

    # -- the reference's interface --------------------------------------------------------------
    @property
    def instance_ids(self):
        return list(self._trees.keys())

    def initialize(self, instance_id, *, pitch):
        if instance_id in self._trees:
            raise ValueError(f"instance {instance_id} already exists")
        if not pitch > 0:
            raise ValueError("pitch must be positive")
        self._trees[instance_id] = _Tree(pitch)
        self._table = None

    def integrate(self, instance_id, mask, pcd, origin=(0, 0, 0)):
        """insertPointCloud of the points ``pcd[mask]`` ([H,W,3], NaN rows skipped) seen from ``origin``."""
        tree = self._index(instance_id)
        pts = self._points(pcd)
        label = self._device(mask).reshape(-1).to(torch.bool).to(torch.int32).contiguous()
        if label.numel() != pts.shape[0]:
            raise ValueError("mask and pcd differ in size")
        self._scans(pts, label, [(1, tree, 0)], origin)

    def update(self, instance_id, occupied):
        """updateNodes(occupied, True): one hit per point ([N,3]); duplicates are not merged."""
        tree = self._index(instance_id)
        pts = self._points(occupied)
        n = pts.shape[0]
        if n == 0:
            return
        ones = torch.ones(n, dtype=torch.int32, device=self.device)
        self._grow(pts, ones, [(1, tree, 0)], origin=None)
        L = _lib.lib()
        _lib.check(L.mf_occmap_count_hits(pts.data_ptr(), n, self._descs().data_ptr(), tree, self._overflow.data_ptr(),
                                          _lib.stream_ptr()), "mf_occmap_count_hits")
        self._apply(mode=1)

    def get_target_grids(self, target_id, *, dimensions, pitch, origin):
        """(grid_target, grid_nontarget, grid_empty), each ``dimensions`` float32, sampled at the voxel centres
        ``origin + index * pitch``.  NumPy results unless ``origin`` is a tensor."""
        dims = tuple(int(d) for d in dimensions)
        if len(dims) != 3 or min(dims) <= 0:
            raise ValueError("dimensions must be 3 positive ints")
        if not pitch > 0:
            raise ValueError("pitch must be positive")
        if isinstance(origin, torch.Tensor):
            o = origin.detach().reshape(1, 3)
        else:
            o = np.asarray(origin, np.float64).reshape(1, 3)
            if np.isnan(o).any():
                raise ValueError("origin has NaN")
        grids = self.get_target_grids_batch([target_id], [float(pitch)], o, dimensions=dims)
        return tuple(g[0] for g in grids)

    def get_target_pcds(self, target_id, aabb_min=None, aabb_max=None):
        raise NotImplementedError(
            "get_target_pcds is not provided: its points are the centres of OctoMap's leaves, which depend on the "
            "octree's pruning, and nothing on the pose-estimation path calls it")

    # -- batched forms for the frame path --------------------------------------------------------
    def integrate_frame(self, pcd, instance_label, instance_ids, class_ids, pitch_of, origin=(0, 0, 0)):
        """``build_octomap`` (base.py:28-46) in one bounds + one ray-cast + one apply launch: every instance with
        class_id > 0 is a map of pitch ``pitch_of(class_id)`` (a callable or a dict) with one scan of its pixels;
        instance 0 (pitch 0.01) gets one scan per remaining label of ``instance_label``, in ``np.unique`` order
        (more than 32 such labels take one more ray-cast + apply per 32)."""
        ids = [int(i) for i in np.asarray(instance_ids.cpu() if isinstance(instance_ids, torch.Tensor) else instance_ids).reshape(-1)]
        cls = [int(c) for c in np.asarray(class_ids.cpu() if isinstance(class_ids, torch.Tensor) else class_ids).reshape(-1)]
        if len(ids) != len(cls):
            raise ValueError("instance_ids and class_ids differ in length")
        get_pitch = pitch_of.__getitem__ if isinstance(pitch_of, dict) else pitch_of
        fg = []
        for i, c in zip(ids, cls):
            if c <= 0:
                continue
            self.initialize(i, pitch=get_pitch(c))
            fg.append((i, self._index(i), 0))
        self.initialize(0, pitch=0.01)
        bg_tree = self._index(0)
        if isinstance(instance_label, torch.Tensor):
            labels = torch.unique(instance_label).cpu().numpy()
        else:
            labels = np.unique(np.asarray(instance_label))
        bg = [int(u) for u in labels if int(u) not in ids]
        pts = self._points(pcd)
        label = self._device(instance_label).reshape(-1).to(torch.int32).contiguous()
        if label.numel() != pts.shape[0]:
            raise ValueError("instance_label and pcd differ in size")
        chunks = [bg[k:k + _MAX_SCANS] for k in range(0, len(bg), _MAX_SCANS)] or [[]]
        # one bounds launch over every slot (the scan index plays no part in the bounds)
        self._grow(pts, label, fg + [(u, bg_tree, 0) for u in bg], origin)
        for k, chunk in enumerate(chunks):
            slots = (fg if k == 0 else []) + [(u, bg_tree, s) for s, u in enumerate(chunk)]
            self._raycast(pts, label, slots, origin)
            self._apply(mode=0)

    def integrate_tracked_frame(self, pcd, label_tracked, instance_id_to_class_id, pitch_of, origin=(0, 0, 0)):
        """``insertScan`` for frame k >= 0 of a tracked sequence (contrib.InstanceTracker): ``pcd`` [H,W,3] in the MAP
        frame seen from ``origin``, ``label_tracked`` [H,W] with tracked instance ids >= 1, -1 = background (one scan
        of the background map ``BACKGROUND_ID``, pitch 0.01) and -2 = uncertain (skipped).  Every id of
        ``instance_id_to_class_id`` that has no map yet gets one of pitch ``pitch_of(class_id)``, in ascending id,
        then the background map; each map takes one scan of its pixels: one bounds + one ray-cast + one apply
        launch, and no read-back beyond the bounds."""
        get_pitch = pitch_of.__getitem__ if isinstance(pitch_of, dict) else pitch_of
        ids = sorted(int(i) for i in instance_id_to_class_id)
        if ids and ids[0] <= BACKGROUND_ID:
            raise ValueError("tracked instance ids must be >= 1")
        for i in ids:
            if i not in self._trees:
                self.initialize(i, pitch=get_pitch(int(instance_id_to_class_id[i])))
        if BACKGROUND_ID not in self._trees:
            self.initialize(BACKGROUND_ID, pitch=0.01)
        pts = self._points(pcd)
        label = self._device(label_tracked).reshape(-1).to(torch.int32).contiguous()
        if label.numel() != pts.shape[0]:
            raise ValueError("label_tracked and pcd differ in size")
        slots = [(i, self._index(i), 0) for i in ids] + [(-1, self._index(BACKGROUND_ID), 0)]
        self._scans(pts, label, slots, origin)

    def get_target_grids_batch(self, target_ids, pitch, origin, dimensions=(32, 32, 32), network_inputs=False):
        """B grids at once: target_ids [B], pitch [B], origin [B,3] (float64 arithmetic for the voxel centres).
        Returns (grid_target, grid_nontarget, grid_empty) [B,*dimensions] float32, followed with
        ``network_inputs=True`` by the booleans of ``data_formats.grids_for_network(train=False)``
        (grid_target, grid_nontarget_empty).  Device tensors if ``pitch`` or ``origin`` is a tensor."""
        as_tensor = _is_tensor(pitch, origin)
        dims = tuple(int(d) for d in dimensions)
        tids = [int(t) for t in np.asarray(target_ids.cpu() if isinstance(target_ids, torch.Tensor) else target_ids).reshape(-1)]
        B = len(tids)
        index = {i: k for k, i in enumerate(self._trees)}
        target = torch.tensor([index.get(t, -1) for t in tids], dtype=torch.int32).to(self.device)
        p = self._device(pitch).reshape(-1).to(torch.float64).contiguous()
        o = self._device(origin).reshape(-1, 3).to(torch.float64).contiguous()
        if p.numel() != B or o.shape[0] != B:
            raise ValueError("target_ids, pitch and origin differ in length")
        kw = dict(dtype=torch.float32, device=self.device)
        gt, gn, ge = (torch.empty((B,) + dims, **kw) for _ in range(3))
        nt = nn = None
        if network_inputs:
            nt = torch.empty((B,) + dims, dtype=torch.bool, device=self.device)
            nn = torch.empty((B,) + dims, dtype=torch.bool, device=self.device)
        table = self._descs()
        _lib.check(_lib.lib().mf_occmap_extract(
            _lib.ptr(table), len(self._trees), target.data_ptr(), p.data_ptr(), o.data_ptr(), B, *dims,
            gt.data_ptr(), gn.data_ptr(), ge.data_ptr(), _lib.ptr(nt), _lib.ptr(nn), _lib.stream_ptr()),
            "mf_occmap_extract")
        out = (gt, gn, ge) + ((nt, nn) if network_inputs else ())
        return out if as_tensor else tuple(x.cpu().numpy() for x in out)

    def dense_logodds(self, instance_id):
        """(lo [3] int keys of cell 0, log-odds [X,Y,Z] float32 with NaN = unknown) of one map, as NumPy."""
        t = self._trees[instance_id]
        if t.lo is None:
            return np.zeros(3, np.int64), np.zeros((0, 0, 0), np.float32)
        return np.asarray(t.lo, np.int64), t.logodds.cpu().numpy()

    # -- internals -----------------------------------------------------------------------------
    def _index(self, instance_id):
        if instance_id not in self._trees:
            raise KeyError(f"instance {instance_id} is not initialized")
        return list(self._trees).index(instance_id)

    def _device(self, x):
        if isinstance(x, torch.Tensor):
            x = x.detach()
            if x.device != self.device:
                x = x.to(self.device)
            return x
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.device)

    def _points(self, pcd):
        # octomap's point3d: every coordinate rounded to float32 first
        x = self._device(pcd)
        if x.shape[-1] != 3:
            raise ValueError("points must have 3 coordinates in the last axis")
        return x.reshape(-1, 3).to(torch.float32).contiguous()

    def _descs(self):
        if self._table is None:
            descs = (_lib.OccTree * max(len(self._trees), 1))(*[t.desc() for t in self._trees.values()])
            raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).clone()
            self._table = raw.to(self.device)
        return self._table

    def _slots(self, slots):
        return torch.tensor(slots, dtype=torch.int32).reshape(-1, 3).to(self.device)

    def _grow(self, pts, label, slots, origin):
        """The one readback of a batch: per tree key bounds of the scan -> grow every box that they leave."""
        L = _lib.lib()
        n_trees = len(self._trees)
        table = self._descs()
        st = self._slots(slots)
        bounds = torch.empty((n_trees, 6), dtype=torch.int32, device=self.device)
        _lib.check(L.mf_occmap_bounds(pts.data_ptr(), label.data_ptr(), pts.shape[0], st.data_ptr(), len(slots),
                                      table.data_ptr(), n_trees, bounds.data_ptr(), _lib.stream_ptr()),
                   "mf_occmap_bounds")
        self._fit(bounds.cpu().numpy(), origin)

    def _fit(self, bounds, origin, origin_trees=None):
        """Grow every box that the key bounds [n_trees, 6] of a batch leave; ``origin``'s key joins the bounds of the
        trees in ``origin_trees`` (tree indices; None: every tree with points)."""
        changed = False
        for t, tree in enumerate(self._trees.values()):
            lo, hi = bounds[t, :3].astype(np.int64), bounds[t, 3:].astype(np.int64)
            if (lo > hi).any():
                continue  # no point of this tree in the batch
            if origin is not None and (origin_trees is None or t in origin_trees):
                ok = [_key(c, tree.res_factor) for c in _lib.as_float3(origin)]
                if None not in ok:
                    lo, hi = np.minimum(lo, ok), np.maximum(hi, ok)
            # one cell of margin: the DDA may pass the end key by one cell through rounding
            lo, hi = np.maximum(lo - 1, 0), np.minimum(hi + 1, 2 * _KEY_MAX - 1)
            if tree.lo is not None:
                old_lo = np.asarray(tree.lo)
                old_hi = old_lo + np.asarray(tree.dim) - 1
                if (lo >= old_lo).all() and (hi <= old_hi).all():
                    continue
                lo, hi = np.minimum(lo, old_lo), np.maximum(hi, old_hi)
            self._regrid(tree, [int(v) for v in lo], [int(v) for v in hi - lo + 1])
            changed = True
        if changed:
            self._table = None

    def _regrid(self, tree, lo, dim):
        """A new box for ``tree``: the old values copied over on the device, NaN elsewhere."""
        cells = dim[0] * dim[1] * dim[2]
        logodds = torch.empty(dim, dtype=torch.float32, device=self.device)
        bits = torch.empty((cells, 2), dtype=torch.int32, device=self.device)
        new = _Tree(tree.resolution)
        new.lo, new.dim, new.logodds, new.bits = list(lo), tuple(dim), logodds, bits
        dst = new.desc()
        src = tree.desc() if tree.lo is not None else None
        _lib.check(_lib.lib().mf_occmap_regrid(None if src is None else src, dst, _lib.stream_ptr()),
                   "mf_occmap_regrid")
        tree.lo, tree.dim, tree.logodds, tree.bits = new.lo, new.dim, logodds, bits

    def _raycast(self, pts, label, slots, origin):
        if not slots:
            return
        table = self._descs()
        st = self._slots(slots)
        o = [float(np.float32(c)) for c in _lib.as_float3(origin)]
        _lib.check(_lib.lib().mf_occmap_raycast(pts.data_ptr(), label.data_ptr(), pts.shape[0], st.data_ptr(),
                                                len(slots), table.data_ptr(), *o, self._overflow.data_ptr(),
                                                _lib.stream_ptr()), "mf_occmap_raycast")

    def _scans(self, pts, label, slots, origin):
        self._grow(pts, label, slots, origin)
        self._raycast(pts, label, slots, origin)
        self._apply(mode=0)

    def _apply(self, mode):
        cells = [t.dim[0] * t.dim[1] * t.dim[2] for t in self._trees.values()]
        _lib.check(_lib.lib().mf_occmap_apply(self._descs().data_ptr(), len(self._trees), max(cells, default=0), mode,
                                              _lib.stream_ptr()), "mf_occmap_apply")
