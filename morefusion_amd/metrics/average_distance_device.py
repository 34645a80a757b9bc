"""ADD and ADD-S of many (model cloud, pose, pose) items in one launch, float64 on the device (csrc/posemetric.hip).

What ``metrics.average_distance`` computes one object at a time through a k-d tree on the host, for every item of a
call at once and without the poses leaving the device: ADD = mean distance between corresponding points under the two
transforms, ADD-S = mean distance from each point under ``transform1`` to its nearest neighbour under ``transform2``
(exact brute force).  The arithmetic and the order of every sum are fixed (DESIGN.md "Pose metric"): a result is a
function of its own item alone and equals the NumPy mirror of the tests bit for bit; it agrees with the host function
to the rounding of the latter's BLAS transform.
"""
import numpy as np
import torch

from .. import _lib


def _tensor(x):
    if isinstance(x, torch.Tensor):
        return x.detach()
    a = np.asarray(x)
    return torch.as_tensor(a if a.flags.writeable else a.copy())  # (torch refuses to wrap read-only memory quietly)


def _cloud(points):
    t = _tensor(points)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("points must be [n,3] and the transforms 4x4")
    if t.shape[0] == 0:
        raise ValueError("empty point cloud")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"points must be float32 or float64, got {t.dtype}")
    return t


def _transforms(T, n, dev):
    if isinstance(T, (list, tuple)):
        if len(T) != n:
            raise ValueError("points, transform1 and transform2 must have the same length")
        if any(tuple(np.shape(x)) != (4, 4) for x in T):
            raise ValueError("points must be [n,3] and the transforms 4x4")
        T = torch.stack([x.detach() for x in T]) if n and all(isinstance(x, torch.Tensor) for x in T) \
            else np.asarray([np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x) for x in T])
    t = _tensor(T)
    if n == 0 and t.numel() == 0:
        t = t.reshape(0, 4, 4)
    if t.ndim != 3 or tuple(t.shape[1:]) != (4, 4):
        raise ValueError("points must be [n,3] and the transforms 4x4")
    if t.shape[0] != n:
        raise ValueError("points, transform1 and transform2 must have the same length")
    return t.to(device=dev, dtype=torch.float64).contiguous()


class PackedClouds:
    """Distinct model clouds concatenated on the device (float64 [sumP, 3], offsets int32 [M + 1]); build it once when
    the same clouds are scored call after call and pass it as ``points`` with a ``cloud_index``."""

    def __init__(self, clouds, device=None):
        if not isinstance(clouds, (list, tuple)):
            raise TypeError("points must be a list of [n,3] arrays (one per instance)")
        clouds = [_cloud(c) for c in clouds]
        if device is None:
            device = next((c.device for c in clouds if c.is_cuda), torch.device("cuda"))
        self.device = torch.device(device)
        self.lengths = [int(c.shape[0]) for c in clouds]
        if sum(self.lengths) >= 2 ** 31:
            raise ValueError("more than 2^31 - 1 points in one call")
        self.offsets = torch.as_tensor(np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int32)).to(self.device)
        # float32 -> float64 is exact
        self.points = (torch.cat([c.to(device=self.device, dtype=torch.float64) for c in clouds]).contiguous()
                       if clouds else torch.zeros((0, 3), dtype=torch.float64, device=self.device))


def average_distance_device(points, transform1, transform2, translate=True, cloud_index=None, device=None):
    """``points``: a list of [n,3] arrays or tensors (float32 or float64), one per item -- or, with ``cloud_index``,
    the distinct clouds (a list or a ``PackedClouds``), item i scoring cloud ``cloud_index[i]``.  ``transform1`` /
    ``transform2``: [I,4,4] arrays or tensors (or lists of 4x4).  Returns ``(adds, add_ss)``, float64 device tensors
    [I].  ``ValueError`` for an empty cloud, lengths that differ, transforms that are not 4x4 and a cloud index out of
    range, as the host function.  One launch pair on the current stream; nothing is copied to the host."""
    packed = points if isinstance(points, PackedClouds) else PackedClouds(points, device)
    dev = packed.device
    if cloud_index is None:
        index = np.arange(len(packed.lengths), dtype=np.int32)
    else:
        index = np.asarray(cloud_index.detach().cpu() if isinstance(cloud_index, torch.Tensor) else cloud_index)
        if index.ndim != 1 or (index.size and not np.issubdtype(index.dtype, np.integer)):
            raise ValueError("cloud_index must be a 1-D integer sequence")
        if index.size and (index.min() < 0 or index.max() >= len(packed.lengths)):
            raise ValueError(f"cloud_index outside 0 .. {len(packed.lengths) - 1}")
        index = index.astype(np.int32)
    n = int(index.shape[0])
    if n > 65535:
        raise ValueError("at most 65535 items per call")
    T1, T2 = _transforms(transform1, n, dev), _transforms(transform2, n, dev)
    adds = torch.empty(n, dtype=torch.float64, device=dev)
    add_ss = torch.empty(n, dtype=torch.float64, device=dev)
    if n == 0:
        return adds, add_ss
    max_points = max(packed.lengths[c] for c in set(index.tolist()))
    item_cloud = torch.as_tensor(index).to(dev)
    L = _lib.lib()
    nbytes = L.mf_average_distance_f64_workspace_bytes(n, max_points)
    if nbytes < 0:
        raise ValueError(f"{n} items of up to {max_points} points: bad sizes")
    workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    _lib.require_gpu(packed.points, packed.offsets, item_cloud, T1, T2, adds, add_ss, workspace)
    _lib.check(L.mf_average_distance_f64(_lib.ptr(packed.points), _lib.ptr(packed.offsets), _lib.ptr(item_cloud),
                                         _lib.ptr(T1), _lib.ptr(T2), len(packed.lengths), n, max_points,
                                         int(bool(translate)), _lib.ptr(adds), _lib.ptr(add_ss), _lib.ptr(workspace),
                                         _lib.stream_ptr()), "mf_average_distance_f64")
    return adds, add_ss
