"""The camera's pose from the depth images alone: dense point-to-plane alignment over a depth pyramid
(csrc/camtrack.hip, include/mfhip.h ``mf_camtrack_*``, DESIGN.md "Camera tracking").

Every stage of the online path -- ``InstanceTracker``, ``OctomapServer``, the pose network's grids -- takes
``T_sensor_to_map``.  The reference gets it from ORB-SLAM2, an external ROS package (ros/src/.rosinstall); here it
comes from the tracking step of KinectFusion (Newcombe et al., ISMAR 2011): projective data association and
point-to-plane Gauss-Newton, coarse to fine, in float64 on the device.

* ``align_depth``: B independent (current, reference) depth pairs in one call.
* ``CameraTracker``: a sequence, frame to frame (``reference="previous"``), against the first frame (``"first"``) or
  against any depth image the caller sets (``set_reference``: e.g. a depth render of the map server's maps, so that
  frame-to-model tracking goes through the same call).

An alignment that fails -- fewer than ``min_pairs`` pairs, or a singular system -- is a state, not an error: its
``status`` is lost, its pose is the initial one.  Nothing is read back unless the caller asks for it.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _lib

MAX_LEVELS, MAX_BATCH = 8, 1024  # MF_CAMTRACK_MAX_LEVELS, MF_CAMTRACK_MAX_BATCH (include/mfhip.h)
PYRAMID, ALIGN = 0, 1            # MF_CAMTRACK_PYRAMID, MF_CAMTRACK_ALIGN
TRACKING, LOST_PAIRS, LOST_PIVOT = 0, 1, 2


def _align16(n):
    return (n + 15) & ~15


def _check_shape(B, height, width, levels):
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels = {levels}: 1 .. {MAX_LEVELS}")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"{B} alignments: 1 .. {MAX_BATCH} per call")
    if (height >> (levels - 1)) < 8 or (width >> (levels - 1)) < 8:
        raise ValueError(f"{height} x {width} with {levels} levels: the coarsest level must be at least 8 x 8")


def _intrinsics(K):
    K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
    if K.shape != (3, 3):
        raise ValueError(f"K must be 3 x 3, got {K.shape}")
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if fx == 0.0 or fy == 0.0:
        raise ValueError("K: fx and fy must not be 0")
    return fx, fy, cx, cy


def _knobs(iterations, levels, block_band, distance_threshold, angle_threshold, min_pairs):
    iterations = tuple(int(i) for i in iterations)
    if len(iterations) != levels:
        raise ValueError(f"{len(iterations)} iteration counts for {levels} levels (coarse to fine)")
    if min(iterations) < 0:
        raise ValueError("iteration counts must be >= 0")
    if not block_band >= 0 or not distance_threshold >= 0 or not 0 <= angle_threshold <= 180 or min_pairs < 0:
        raise ValueError("block_band, distance_threshold >= 0, angle_threshold in 0 .. 180 degrees, min_pairs >= 0")
    return iterations, math.cos(math.radians(float(angle_threshold)))


class DepthPyramid:
    """One pyramid buffer (the layout of include/mfhip.h) for B images, with typed views of its parts."""

    def __init__(self, B, height, width, levels, intrinsics, device):
        _check_shape(B, height, width, levels)
        self.B, self.height, self.width, self.levels, self.intrinsics = B, height, width, levels, intrinsics
        nbytes = _lib.lib().mf_camtrack_workspace_bytes(B, height, width, levels, PYRAMID)
        if nbytes < 0:
            raise ValueError(f"mf_camtrack_workspace_bytes refused B = {B}, {height} x {width}, {levels} levels")
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.require_gpu(self.buf)

    def fill(self, depth, block_band):
        """depth float32 [B, H, W] on the pyramid's device."""
        fx, fy, cx, cy = self.intrinsics
        _lib.require_gpu(depth)
        _lib.check(_lib.lib().mf_camtrack_prepare(_lib.ptr(depth), self.B, self.height, self.width, self.levels, fx,
                                                  fy, cx, cy, float(block_band), _lib.ptr(self.buf),
                                                  _lib.stream_ptr()), "mf_camtrack_prepare")

    def level(self, l):
        """dict(depth float32 [B, h, w], vertex / normal float64 [B, h, w, 3]): views of level ``l``."""
        off = 0
        for k in range(self.levels):
            h, w = self.height >> k, self.width >> k
            n = self.B * h * w
            parts = {}
            for name, dtype, size, shape in (("depth", torch.float32, 4 * n, (self.B, h, w)),
                                             ("vertex", torch.float64, 24 * n, (self.B, h, w, 3)),
                                             ("normal", torch.float64, 24 * n, (self.B, h, w, 3))):
                parts[name] = self.buf[off:off + size].view(dtype).view(shape)
                off = _align16(off + size)
            if k == l:
                return parts
        raise IndexError(l)


class _Aligner:
    """The buffers of ``mf_camtrack_align`` for one shape; ``run`` is its launch sequence."""

    def __init__(self, B, height, width, levels, intrinsics, iterations, distance_threshold, cos_angle_threshold,
                 min_pairs, device):
        self.shape, self.intrinsics = (B, height, width, levels), intrinsics
        self.iterations = (ctypes.c_int32 * levels)(*iterations)
        self.knobs = (float(distance_threshold), float(cos_angle_threshold), int(min_pairs))
        n_iters = sum(iterations)
        nbytes = _lib.lib().mf_camtrack_workspace_bytes(B, height, width, levels, ALIGN)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.pose = torch.empty((B, 7), dtype=torch.float64, device=device)
        self.T = torch.empty((B, 4, 4), dtype=torch.float64, device=device)
        self.status = torch.empty(B, dtype=torch.int32, device=device)
        self.stats = torch.empty((B, n_iters, 3), dtype=torch.float64, device=device)
        _lib.require_gpu(self.ws, self.pose, self.T, self.status, self.stats)

    def run(self, cur, ref, T_ref, T_init):
        B, height, width, levels = self.shape
        fx, fy, cx, cy = self.intrinsics
        _lib.require_gpu(T_ref, T_init)
        _lib.check(_lib.lib().mf_camtrack_align(
            _lib.ptr(cur.buf), _lib.ptr(ref.buf), B, height, width, levels, fx, fy, cx, cy, _lib.ptr(T_ref),
            _lib.ptr(T_init), ctypes.addressof(self.iterations), *self.knobs, _lib.ptr(self.pose), _lib.ptr(self.T),
            _lib.ptr(self.status), _lib.ptr(self.stats), _lib.ptr(self.ws), _lib.stream_ptr()), "mf_camtrack_align")


def _depth_tensor(depth, device, ndim):
    """NumPy array or tensor -> contiguous float32 tensor on ``device`` with ``ndim`` dimensions (a leading 1 added)."""
    t = depth if isinstance(depth, torch.Tensor) else torch.as_tensor(np.asarray(depth))
    if not t.dtype.is_floating_point:
        raise TypeError("depth must be a float image in metres")
    if t.dim() == ndim - 1:
        t = t[None]
    if t.dim() != ndim:
        raise ValueError(f"depth must have {ndim - 1} or {ndim} dimensions, got {tuple(t.shape)}")
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _pose_tensor(T, B, device, what):
    t = T if isinstance(T, torch.Tensor) else torch.as_tensor(np.asarray(T, np.float64))
    if tuple(t.shape) == (4, 4):
        t = t[None].expand(B, 4, 4)
    if tuple(t.shape) != (B, 4, 4):
        raise ValueError(f"{what} must be [4, 4] or [{B}, 4, 4], got {tuple(t.shape)}")
    return t.detach().to(device=device, dtype=torch.float64).contiguous()


def align_depth(depth_cur, depth_ref, K, T_ref_to_map, T_init=None, levels=3, iterations=(10, 5, 4),
                block_band=0.05, distance_threshold=0.1, angle_threshold=20.0, min_pairs=100, device=None,
                return_pose=False):
    """Align B current depth images to B reference depth images (float [B, H, W] or [H, W], metres, NaN or <= 0
    invalid; one pinhole ``K``).  ``T_ref_to_map`` [B, 4, 4] (or [4, 4] for all) are the references' poses,
    ``T_init`` the first guesses of the current images' poses (None: the references' poses).  ``iterations``: the
    Gauss-Newton iterations per level, coarse to fine; ``angle_threshold`` in degrees (its cosine is taken here).

    Returns ``(T_cur_to_map [B, 4, 4] float64, status [B] int32, stats [B, n_iters, 3] float64)``: status 0 =
    tracking, 1 = lost for fewer than ``min_pairs`` pairs, 2 = lost for a singular system (the pose is then the
    initial one); stats = (pairs, sum of squared residuals, norm of the increment) per iteration, zeros after a loss.
    With ``return_pose`` also the unit quaternion (w, x, y, z) and translation [B, 7] the matrices were made from.
    Device tensors in give device tensors out and nothing is read back; NumPy arrays in give NumPy arrays out.
    The work runs on ``device`` (default: the depth tensor's device, else "cuda"); there is no CPU fallback."""
    as_numpy = not isinstance(depth_cur, torch.Tensor)
    if device is None:
        device = depth_cur.device if isinstance(depth_cur, torch.Tensor) else torch.device("cuda")
    cur, ref = _depth_tensor(depth_cur, device, 3), _depth_tensor(depth_ref, device, 3)
    if cur.shape != ref.shape:
        raise ValueError(f"current {tuple(cur.shape)} and reference {tuple(ref.shape)} depth differ in shape")
    B, height, width = (int(s) for s in cur.shape)
    _check_shape(B, height, width, levels)
    iterations, cos_thr = _knobs(iterations, levels, block_band, distance_threshold, angle_threshold, min_pairs)
    intr = _intrinsics(K)
    T_ref = _pose_tensor(T_ref_to_map, B, device, "T_ref_to_map")
    T_0 = T_ref if T_init is None else _pose_tensor(T_init, B, device, "T_init")
    pc, pr = (DepthPyramid(B, height, width, levels, intr, device) for _ in range(2))
    pc.fill(cur, block_band)
    pr.fill(ref, block_band)
    al = _Aligner(B, height, width, levels, intr, iterations, distance_threshold, cos_thr, min_pairs, device)
    al.run(pc, pr, T_ref, T_0)
    out = (al.T, al.status, al.stats) + ((al.pose,) if return_pose else ())
    return tuple(o.cpu().numpy() for o in out) if as_numpy else out


class CameraTracker:
    """Track a depth sequence of ``height`` x ``width`` images through the pinhole ``K``.

    ``track(depth, T_init=None)`` aligns the image to the held reference and returns ``T_cur_to_map`` (a float64
    [4, 4] tensor on the device; ``T_init`` None: the last pose).  The first call makes the image the reference at
    ``T_first`` (default: the identity) and returns ``T_first``.  ``reference="previous"`` then replaces the
    reference by every tracked image at its estimated pose (also after a loss, where that pose is the initial one:
    the status is not read back to decide); ``"first"`` keeps it.  ``set_reference(depth, T_ref_to_map)`` installs
    any depth image as the reference, e.g. a depth render of the map server's maps (``contrib.render_voxel_grids``,
    or the tracker's ray-cast) from the last pose: frame-to-model tracking through the same call.

    ``status`` / ``lost`` / ``stats`` of the last alignment are read back only when asked for."""

    def __init__(self, K, height, width, levels=3, iterations=(10, 5, 4), reference="previous", T_first=None,
                 block_band=0.05, distance_threshold=0.1, angle_threshold=20.0, min_pairs=100, device=None):
        if reference not in ("previous", "first"):
            raise ValueError(f"reference = {reference!r}: 'previous' or 'first'")
        self.height, self.width, self.levels = int(height), int(width), int(levels)
        _check_shape(1, self.height, self.width, self.levels)
        iterations, cos_thr = _knobs(iterations, self.levels, block_band, distance_threshold, angle_threshold,
                                     min_pairs)
        self.reference, self.block_band = reference, float(block_band)
        self.device = torch.device("cuda" if device is None else device)
        intr = _intrinsics(K)
        self._T_first = _pose_tensor(np.eye(4) if T_first is None else T_first, 1, self.device, "T_first")
        self._cur, self._ref = (DepthPyramid(1, self.height, self.width, self.levels, intr, self.device)
                                for _ in range(2))
        self._al = _Aligner(1, self.height, self.width, self.levels, intr, iterations, distance_threshold, cos_thr,
                            min_pairs, self.device)
        self._T_ref = self._T_last = None
        self._aligned = False

    def _depth(self, depth):
        d = _depth_tensor(depth, self.device, 3)
        if tuple(d.shape) != (1, self.height, self.width):
            raise ValueError(f"depth {tuple(d.shape[1:])}: the tracker was made for {self.height} x {self.width}")
        return d

    def set_reference(self, depth, T_ref_to_map):
        self._ref.fill(self._depth(depth), self.block_band)
        self._T_ref = _pose_tensor(T_ref_to_map, 1, self.device, "T_ref_to_map").clone()
        if self._T_last is None:
            self._T_last = self._T_ref
        return self

    def track(self, depth, T_init=None):
        d = self._depth(depth)
        if self._T_ref is None:
            self.set_reference(d, self._T_first)
            return self._T_last[0].clone()
        self._cur.fill(d, self.block_band)
        T_0 = self._T_last if T_init is None else _pose_tensor(T_init, 1, self.device, "T_init")
        self._al.run(self._cur, self._ref, self._T_ref, T_0)
        self._aligned = True
        self._T_last = self._al.T.clone()
        if self.reference == "previous":
            self._cur, self._ref = self._ref, self._cur
            self._T_ref = self._T_last
        return self._T_last[0].clone()

    def _asked(self):
        if not self._aligned:
            raise RuntimeError("no alignment yet: the first track() only sets the reference")

    @property
    def status(self):
        self._asked()
        return int(self._al.status.cpu()[0])

    @property
    def lost(self):
        return self.status != TRACKING

    @property
    def stats(self):
        self._asked()
        return self._al.stats[0].cpu().numpy()
