"""TSDF labels: a TSDF volume that also fuses the instance label of every pixel, and gives the pose stages what they
took from the map server -- the grids of every instance in the sensor frame -- from that one model (csrc/tsdflabel.hip,
include/mfhip.h ``mf_tsdf_*`` "TSDF labels", DESIGN.md "TSDF labels").

``InstanceTsdfVolume`` is a ``TsdfVolume`` with a second tensor ``labels`` int32 ``[nz, ny, nx, 2]`` of (label, count)
per voxel.  ``integrate(depth, K, T, label=...)`` fuses the depth exactly as the parent does and lets every voxel near
the surface take the vote of the pixel it projects to (``label_tracked`` of ``OctomapServer.insert_scan``: ids >= 1,
-1 = background, anything else does not vote): agreement raises the count up to ``max_count``, disagreement lowers it,
and at 0 the next vote claims the voxel.  From the two tensors:

* ``label_image``: the instance under every pixel of a depth image (e.g. ``raycast``'s, from the same pose);
* ``instance_stats``: count, centre and bounds of every instance's solid voxels, in the map frame;
* ``publish_grids``: the dict of ``OctomapServer.publish_grids`` (``Model.predict`` / ICC take either).

``ModelTracker.track(depth, label)`` (contrib/tsdf_volume.py) fuses the labels in its loop."""
import numpy as np
import torch

from .. import _lib
from .camera_tracking import _depth_tensor
from .tsdf_volume import TsdfVolume, _camera, _view

MAX_INSTANCES = 64    # MF_TSDF_MAX_INSTANCES (include/mfhip.h)
MAX_GRID_DIM = 256    # MF_TSDF_MAX_GRID_DIM


def _label_tensor(label, device, shape):
    t = label if isinstance(label, torch.Tensor) else torch.as_tensor(np.asarray(label))
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("label must be an integer image (ids >= 1, -1 background, others do not vote)")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"label must be {tuple(shape)} like the depth, got {tuple(t.shape)}")
    return t.detach().to(device=device, dtype=torch.int32).contiguous()


def _count(value, name):
    if int(value) != value or int(value) < 1:
        raise ValueError(f"{name} = {value}: an integer >= 1")
    return int(value)


def inverse_pose(T):
    """``T_map_to_sensor`` of a float64 [4, 4] ``T_sensor_to_map``: R^T and -R^T t, every sum taken left to right."""
    inv = np.eye(4)
    for a in range(3):
        for b in range(3):
            inv[a, b] = T[b, a]
        inv[a, 3] = -((T[0, a] * T[0, 3] + T[1, a] * T[1, 3]) + T[2, a] * T[2, 3])
    return inv


class InstanceTsdfVolume(TsdfVolume):
    """``TsdfVolume`` (same arguments) plus ``labels`` int32 ``[nz, ny, nx, 2]`` of (label, count), (0, 0) when fresh;
    ``max_count`` caps the count (how many contradicting frames a settled voxel outlasts)."""

    def __init__(self, dims, pitch, origin, truncation=None, max_weight=64.0, max_count=64, device=None, colors=False):
        self.max_count = _count(max_count, "max_count")
        self.labels = None
        super().__init__(dims, pitch, origin, truncation=truncation, max_weight=max_weight, device=device,
                         colors=colors)

    def reset(self):
        super().reset()
        if self.labels is None:
            nx, ny, nz = self.dims
            self.labels = torch.zeros((nz, ny, nx, 2), dtype=torch.int32, device=self.device)
        else:
            self.labels.zero_()
        return self

    def integrate(self, depth, K, T_sensor_to_map, label=None, skip_if=None, color=None):
        """``TsdfVolume.integrate``; with ``label`` (an integer [H, W] image, NumPy or tensor) every updated voxel
        within the truncation of the surface also takes the vote of its pixel.  ``skip_if`` covers every tensor.
        ``color``: as ``TsdfVolume.integrate``'s, fused after the depth and the labels."""
        if label is None:
            return super().integrate(depth, K, T_sensor_to_map, skip_if=skip_if, color=color)
        camera = _camera(K)
        d = _depth_tensor(depth, self.device, 3)
        if d.shape[0] != 1:
            raise ValueError(f"depth must be one [H, W] image, got {tuple(d.shape)}")
        lab = _label_tensor(label, self.device, d.shape[1:])
        rgb = self._color_image_of(color, d.shape[1:])
        if skip_if is not None:
            if not isinstance(skip_if, torch.Tensor) or skip_if.dtype != torch.int32 or skip_if.numel() < 1:
                raise TypeError("skip_if must be an int32 tensor on the volume's device")
            if skip_if.device != d.device:
                raise ValueError(f"skip_if on {skip_if.device}, the volume on {d.device}")
        T = self._pose(T_sensor_to_map)
        tensors = (self.volume, self.labels, d, lab, T) + (() if skip_if is None else (skip_if,))
        _lib.require_gpu(*tensors)
        _lib.check(_lib.lib().mf_tsdf_integrate_labels(
            _lib.ptr(self.volume), _lib.ptr(self.labels), *self._grid, self.truncation, self.max_weight, _lib.ptr(d),
            *_view(d, camera), _lib.ptr(T), _lib.ptr(lab), self.max_count, _lib.ptr(skip_if), _lib.stream_ptr()),
            "mf_tsdf_integrate_labels")
        if rgb is not None:
            self._integrate_colors(d, rgb, camera, T, skip_if)
        return self

    def label_image(self, depth, K, T_sensor_to_map, min_count=1):
        """The fused label under every pixel of ``depth`` (float [H, W] seen through ``K`` from ``T_sensor_to_map``;
        meant for ``raycast``'s render from the same pose) -> int32 [H, W] device tensor: the label of the voxel the
        pixel's point falls into if that voxel's count is >= ``min_count``, else 0; 0 where there is no depth."""
        camera = _camera(K)
        min_count = _count(min_count, "min_count")
        d = _depth_tensor(depth, self.device, 3)
        if d.shape[0] != 1:
            raise ValueError(f"depth must be one [H, W] image, got {tuple(d.shape)}")
        T = self._pose(T_sensor_to_map)
        out = torch.empty(tuple(d.shape[1:]), dtype=torch.int32, device=self.device)
        _lib.require_gpu(self.labels, d, T, out)
        _lib.check(_lib.lib().mf_tsdf_label_image(
            _lib.ptr(self.labels), *self._grid, _lib.ptr(d), *_view(d, camera), _lib.ptr(T), min_count, _lib.ptr(out),
            _lib.stream_ptr()), "mf_tsdf_label_image")
        return out

    def render(self, K, T_sensor_to_map, height, width, step=None, min_depth=0.0, max_depth=None, block=8,
               summary=None, return_code=False, return_stats=False, labels=False, min_count=1):
        """``TsdfVolume.render``; with ``labels`` the same launch also gives the int32 [height, width] label image,
        the bytes of ``label_image(depth, K, T_sensor_to_map, min_count)`` on the depth it returns.
        -> depth, then the label image, code and stats, each if asked for."""
        min_count = _count(min_count, "min_count")
        depth, label, code, stats = self._render(K, T_sensor_to_map, height, width, step, min_depth, max_depth, block,
                                                 summary, self.labels if labels else None, min_count, return_code,
                                                 return_stats)
        out = (depth,) + ((label,) if labels else ()) + ((code,) if return_code else ()) + \
            ((stats,) if return_stats else ())
        return out if len(out) > 1 else depth

    @staticmethod
    def _ids(ids):
        ids = [int(i) for i in ids]
        if not 1 <= len(ids) <= MAX_INSTANCES:
            raise ValueError(f"{len(ids)} ids: between 1 and {MAX_INSTANCES}")
        if any(i == 0 or i < -1 for i in ids):
            raise ValueError(f"ids = {ids}: tracked ids are >= 1, the background is -1")
        if any(b <= a for a, b in zip(ids, ids[1:])):
            raise ValueError(f"ids = {ids}: strictly ascending, no duplicates")
        return ids

    def instance_table(self, ids, min_weight=1.0, min_count=1):
        """The int64 [B, 10] table of ``mf_tsdf_instance_stats`` as a device tensor (nothing is read back)."""
        ids, min_weight, min_count = self._ids(ids), float(min_weight), _count(min_count, "min_count")
        if not min_weight > 0:
            raise ValueError(f"min_weight = {min_weight}: must be > 0")
        dev_ids = torch.tensor(ids, dtype=torch.int32).to(self.device)
        table = torch.empty((len(ids), 10), dtype=torch.int64, device=self.device)
        _lib.require_gpu(self.volume, self.labels, dev_ids, table)
        _lib.check(_lib.lib().mf_tsdf_instance_stats(
            _lib.ptr(self.volume), _lib.ptr(self.labels), *self.dims, min_weight, min_count, _lib.ptr(dev_ids),
            len(ids), _lib.ptr(table), _lib.stream_ptr()), "mf_tsdf_instance_stats")
        return table

    def instance_stats(self, ids, min_weight=1.0, min_count=1):
        """Where the instances are: over the solid voxels (``weight >= min_weight``, ``tsdf <= 0``) that carry the id
        with ``count >= min_count`` -> dict(``count`` int64 [B], ``center``, ``bbx_min``, ``bbx_max`` float64 [B, 3],
        NumPy, in the map frame: the mean and the extreme voxel centres; NaN for an id without voxels).  ``ids``:
        strictly ascending, >= 1 or -1.  One read-back."""
        table = self.instance_table(ids, min_weight, min_count).cpu().numpy()  # the call's read-back
        count = table[:, 0].copy()
        origin, empty = np.asarray(self.origin, np.float64), (count == 0)[:, None]
        with np.errstate(all="ignore"):
            center = origin + self.pitch * (table[:, 1:4].astype(np.float64) / count[:, None].astype(np.float64))
        lo = origin + self.pitch * table[:, 4:7].astype(np.float64)
        hi = origin + self.pitch * table[:, 7:10].astype(np.float64)
        return dict(count=count, center=np.where(empty, np.nan, center), bbx_min=np.where(empty, np.nan, lo),
                    bbx_max=np.where(empty, np.nan, hi))

    def publish_grids(self, T_sensor_to_map, instance_ids, pitch, centers=None, class_ids=None, dim=32, min_weight=1.0,
                      min_count=1, empty_above=0.5, ground_z=None, free_as_noentry=True):
        """The grids of ``OctomapServer.publish_grids`` from the fused model: for every id of ``instance_ids``
        (strictly ascending, >= 1) a ``dim``^3 grid of its ``pitch`` (one per id, or a dict / callable by id) in the
        SENSOR frame around its centre.  -> dict(instance_ids, class_ids (lists), pitch [B] float32, origin [B, 3]
        float64, grid_target / grid_noentry [B, dim, dim, dim] float32 (0 or 1), grid_nontarget_empty bool), device
        tensors.  A solid voxel (``weight >= min_weight``, ``tsdf <= 0``) whose label has ``count >= min_count`` is the
        target where the label is the grid's id and no-entry where it is anything else; observed space with ``tsdf >=
        empty_above`` is no-entry too if ``free_as_noentry``, and so is everything below map z = ``ground_z`` if that
        is given.  ``centers`` [B, 3] (map frame): where the grids sit; None takes them from ``instance_stats`` (one
        read-back) and drops the ids that have no voxel.  ``class_ids``: per id (list, dict or callable), passed
        through; None gives zeros."""
        ids = self._ids(instance_ids)
        if ids[0] < 1:
            raise ValueError(f"instance_ids = {ids}: the grids of tracked instances, ids >= 1")
        dim, min_weight, min_count = int(dim), float(min_weight), _count(min_count, "min_count")
        if not 1 <= dim <= MAX_GRID_DIM:
            raise ValueError(f"dim = {dim}: between 1 and {MAX_GRID_DIM}")
        if not min_weight > 0:
            raise ValueError(f"min_weight = {min_weight}: must be > 0")
        per_id = lambda x, i, n: (x[i] if isinstance(x, dict) else x(i) if callable(x) else x[n])  # noqa: E731
        if not isinstance(pitch, dict) and not callable(pitch) and len(pitch) != len(ids):
            raise ValueError(f"{len(pitch)} pitches for {len(ids)} ids")
        pitches = [float(per_id(pitch, i, n)) for n, i in enumerate(ids)]
        if not all(p > 0 for p in pitches):
            raise ValueError(f"pitch = {pitches}: each > 0")
        classes = [0 if class_ids is None else int(per_id(class_ids, i, n)) for n, i in enumerate(ids)]
        T = T_sensor_to_map.detach().cpu().numpy() if isinstance(T_sensor_to_map, torch.Tensor) else T_sensor_to_map
        T = np.asarray(T, np.float64)
        if T.shape != (4, 4):
            raise ValueError("T_sensor_to_map must be [4, 4]")
        if centers is None:
            stats = self.instance_stats(ids, min_weight, min_count)
            keep = [n for n in range(len(ids)) if stats["count"][n] > 0]
            centers = stats["center"][keep]
            ids, pitches, classes = ([x[n] for n in keep] for x in (ids, pitches, classes))
        else:
            centers = np.asarray(centers.detach().cpu() if isinstance(centers, torch.Tensor) else centers, np.float64)
            if centers.shape != (len(ids), 3):
                raise ValueError(f"centers must be [{len(ids)}, 3], got {centers.shape}")
        B, dev = len(ids), self.device
        shape = (B, dim, dim, dim)
        out = dict(instance_ids=ids, class_ids=classes,
                   pitch=torch.tensor(pitches, dtype=torch.float64).to(torch.float32).to(dev),
                   origin=torch.zeros((B, 3), dtype=torch.float64, device=dev),
                   grid_target=torch.empty(shape, dtype=torch.float32, device=dev),
                   grid_noentry=torch.empty(shape, dtype=torch.float32, device=dev),
                   grid_nontarget_empty=torch.empty(shape, dtype=torch.bool, device=dev))
        if B == 0:
            return out
        dev_ids = torch.tensor(ids, dtype=torch.int32).to(dev)
        grid_pitch = out["pitch"].to(torch.float64)  # the float32 the caller gets back, widened
        dev_centers = torch.from_numpy(np.ascontiguousarray(centers)).to(dev)
        Ts = torch.from_numpy(np.stack([inverse_pose(T), T])).to(dev)
        flags = (0 if ground_z is None else 1) | (2 if free_as_noentry else 0)
        _lib.require_gpu(self.volume, self.labels, dev_ids, grid_pitch, dev_centers, Ts, out["origin"],
                         out["grid_target"], out["grid_noentry"], out["grid_nontarget_empty"])
        _lib.check(_lib.lib().mf_tsdf_publish_grids(
            _lib.ptr(self.volume), _lib.ptr(self.labels), *self._grid, _lib.ptr(dev_ids),
            _lib.ptr(grid_pitch), _lib.ptr(dev_centers), _lib.ptr(Ts[0]), _lib.ptr(Ts[1]), min_weight, min_count,
            float(empty_above), 0.0 if ground_z is None else float(ground_z), flags, B, dim, _lib.ptr(out["origin"]),
            _lib.ptr(out["grid_target"]), _lib.ptr(out["grid_noentry"]), _lib.ptr(out["grid_nontarget_empty"]),
            _lib.stream_ptr()), "mf_tsdf_publish_grids")
        return out
