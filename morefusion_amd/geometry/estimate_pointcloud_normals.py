"""estimate_pointcloud_normals -- surface normals of an organised point cloud (csrc/pickorder.hip).

Behaviour of morefusion/geometry/estimate_pointcloud_normals.py:29-81 for ``[H, W, 3]`` points: per pixel the pair
of perpendicular neighbours at offset 2 (eight candidates) with the smallest summed distance to the pixel, and the
normalised cross product of the two differences; a pixel with no complete pair is NaN.  One float64 kernel
(include/mfhip.h ``mf_pick_normals``) whose arithmetic is pinned bit for bit to the executed reference
(tests/golden/ref_pointcloud_normals.npz).  The unorganised ``[N, 3]`` form of the reference is open3d's hybrid
KD-tree search and is not provided.

NumPy or tensor in (float32 is widened exactly), float64 device tensor out.
"""
import numpy as np
import torch

from .. import _lib
from .mesh_sdf import _device


def _normals(points, rects):
    """points float64 [T, H, W, 3] on the device, rects [T, 4] (y1, x1, y2, x2) -> normals [T, H, W, 3]."""
    n, height, width = points.shape[:3]
    rect = torch.as_tensor(np.asarray(rects, np.int32).reshape(n, 4)).to(points.device)
    out = torch.empty_like(points)
    if points.device.type == "cuda":
        _lib.require_gpu(points, rect, out)
    if n and height and width:
        _lib.check(_lib.lib().mf_pick_normals(_lib.ptr(points), _lib.ptr(rect), n, height, width, _lib.ptr(out),
                                              _lib.stream_ptr()), "mf_pick_normals")
    return out


def estimate_pointcloud_normals(points, device=None):
    ndim = points.ndim
    if ndim == 2:
        raise NotImplementedError("normals of an unorganised (N, 3) point cloud are open3d's hybrid KD-tree search "
                                  "(KDTreeSearchParamHybrid) in the reference; only organised (H, W, 3) points are "
                                  "supported")
    if ndim != 3:
        raise ValueError("points shape must be either (H, W, 3) or (N, 3)")
    if points.shape[2] != 3:
        raise ValueError("points shape must be (H, W, 3)")
    dev = _device(points, device)
    t = points.detach() if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
    t = t.to(device=dev, dtype=torch.float64).contiguous()
    height, width = t.shape[:2]
    return _normals(t[None], [[0, 0, height, width]])[0]
