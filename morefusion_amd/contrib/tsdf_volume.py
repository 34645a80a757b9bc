"""TSDF fusion: depth frames integrated into a truncated-signed-distance volume, the volume ray-cast into a depth
image, and a camera tracker that aligns every frame to that model (csrc/tsdf.hip, include/mfhip.h ``mf_tsdf_*``,
DESIGN.md "TSDF fusion").

``CameraTracker`` aligns a depth image to a reference depth image; against the previous frame every error is inherited,
against the first frame tracking ends when the view has moved on.  The mapping half of KinectFusion (Newcombe et al.,
ISMAR 2011) removes both: ``TsdfVolume.integrate`` fuses each frame into a volume of (tsdf, weight) pairs at its
estimated pose, ``TsdfVolume.raycast`` renders the fused surface from any pose with sub-voxel depth, and
``ModelTracker`` hands that render to ``CameraTracker.set_reference`` before every alignment.

* ``TsdfVolume``: the volume and its two kernels; ``extract_mesh`` takes the fused surface out as a triangle mesh
  with normals (csrc/tsdfmesh.hip, ``mf_tsdfmesh_*``, DESIGN.md "TSDF mesh").
* ``TsdfVolume(colors=True)``: a float32 colour per voxel fused from the frames' RGB images next to the depth;
  ``color_image`` colours a render, ``sample_colors`` any map-frame points, ``extract_mesh(colors=True)`` the mesh's
  vertices (csrc/tsdfcolor.hip, ``mf_tsdf_*_colors`` / ``mf_tsdf_color_image``, DESIGN.md "TSDF colour").
* ``ModelTracker``: ray-cast, align, integrate per frame; no host synchronisation in the loop, and a lost alignment is
  kept out of the model by the device status word, not by reading it back.
"""
import math

import numpy as np
import torch

from .. import _lib
from .camera_tracking import CameraTracker, _depth_tensor, _intrinsics, _pose_tensor

MAX_STEPS = 65536  # MF_TSDF_MAX_STEPS (include/mfhip.h)
RAY_HIT, RAY_LEFT, RAY_BACKFACE, RAY_MISS, RAY_CAP = range(5)  # MF_TSDF_RAY_*
BLOCK_MIXED, BLOCK_FREE, BLOCK_UNKNOWN = range(3)  # MF_TSDF_BLOCK_*
BLOCK_EDGES = (2, 4, 8, 16)


def _camera(K):
    fx, fy, cx, cy = _intrinsics(K)
    if not (fx > 0 and fy > 0):
        raise ValueError("K: fx and fy must be > 0")
    return fx, fy, cx, cy


def _view(d, camera):
    """The image and camera arguments of a kernel that reads the depth tensor ``d`` [1, H, W]: H, W, fx, fy, cx, cy."""
    return (int(d.shape[1]), int(d.shape[2]), *camera)


def _color_tensor(color, device, shape):
    t = color if isinstance(color, torch.Tensor) else torch.as_tensor(np.asarray(color))
    if t.dtype != torch.uint8:
        raise TypeError(f"color must be a uint8 [H, W, 3] image, got {t.dtype}")
    if tuple(t.shape) != tuple(shape) + (3,):
        raise ValueError(f"color must be {tuple(shape) + (3,)} like the depth, got {tuple(t.shape)}")
    return t.detach().to(device=device).contiguous()


class TsdfVolume:
    """``dims`` = (nx, ny, nz) voxels of ``pitch`` metres; voxel (i, j, k) has its centre at ``origin + pitch *
    (i, j, k)`` in the map frame.  ``truncation`` (default ``4 * pitch``) is the distance at which the signed distance
    saturates, ``max_weight`` the cap of the running average's weight.  The storage is one float32 tensor
    ``[nz, ny, nx, 2]`` of (tsdf, weight) on ``device`` (default "cuda"; there is no CPU fallback), (1, 0) when fresh;
    ``.tsdf`` and ``.weight`` are views of it.  With ``colors=True`` the volume also owns ``.colors``, float32
    ``[nz, ny, nx, 4]`` of (r, g, b, colour weight) per voxel, zeros when fresh, r, g, b on the 0 .. 255 scale;
    ``integrate(..., color=)`` fuses into it.  Without it ``.colors`` is None and nothing is allocated."""

    def __init__(self, dims, pitch, origin, truncation=None, max_weight=64.0, device=None, colors=False):
        dims = tuple(int(n) for n in dims)
        if len(dims) != 3 or min(dims) < 2:
            raise ValueError(f"dims = {dims}: three sizes (nx, ny, nz), each >= 2")
        if dims[0] * dims[1] * dims[2] >= 1 << 31:
            raise ValueError(f"dims = {dims}: fewer than 2^31 voxels")
        self.dims, self.pitch = dims, float(pitch)
        if not self.pitch > 0:
            raise ValueError(f"pitch = {pitch}: must be > 0")
        self.origin = tuple(_lib.as_float3(origin))
        self.truncation = 4.0 * self.pitch if truncation is None else float(truncation)
        if not self.truncation > 0:
            raise ValueError(f"truncation = {truncation}: must be > 0")
        self.max_weight = float(max_weight)
        if not self.max_weight >= 1:
            raise ValueError(f"max_weight = {max_weight}: must be >= 1")
        self.device = torch.device("cuda" if device is None else device)
        nx, ny, nz = dims
        self.volume = torch.empty((nz, ny, nx, 2), dtype=torch.float32, device=self.device)
        _lib.require_gpu(self.volume)
        self.colors = torch.empty((nz, ny, nx, 4), dtype=torch.float32, device=self.device) if colors else None
        self.reset()

    def reset(self):
        self.volume[..., 0] = 1.0
        self.volume[..., 1] = 0.0
        if self.colors is not None:
            self.colors.zero_()
        return self

    @property
    def _grid(self):
        """The volume's geometry as the C ABI takes it: nx, ny, nz, origin_x, origin_y, origin_z, pitch."""
        return (*self.dims, *self.origin, self.pitch)

    @property
    def tsdf(self):
        return self.volume[..., 0]

    @property
    def weight(self):
        return self.volume[..., 1]

    def _pose(self, T):
        """NumPy [4, 4] -> a device copy; a device tensor is used in place (no copy if float64 and contiguous)."""
        return _pose_tensor(T, 1, self.device, "T_sensor_to_map")

    def max_steps(self, step):
        """floor(the diagonal of the box of voxel centres / step) + 2."""
        nx, ny, nz = self.dims
        diagonal = self.pitch * math.sqrt(float((nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2))
        return int(math.floor(diagonal / step)) + 2

    def _color_image_of(self, color, shape):
        """The checked uint8 [H, W, 3] device tensor of ``integrate``'s ``color``; None stays None."""
        if color is None:
            return None
        if self.colors is None:
            raise TypeError("color= needs a volume built with colors=True")
        return _color_tensor(color, self.device, shape)

    def _integrate_colors(self, d, rgb, camera, T, skip_if):
        """``mf_tsdf_integrate_colors`` on the depth tensor, pose tensor and skip word of the integrate just issued."""
        _lib.require_gpu(self.colors, d, rgb, T)
        _lib.check(_lib.lib().mf_tsdf_integrate_colors(
            _lib.ptr(self.colors), *self._grid, self.truncation, self.max_weight, _lib.ptr(d), _lib.ptr(rgb),
            *_view(d, camera), _lib.ptr(T), _lib.ptr(skip_if), _lib.stream_ptr()), "mf_tsdf_integrate_colors")

    def integrate(self, depth, K, T_sensor_to_map, skip_if=None, color=None):
        """Fuse ``depth`` (float [H, W] in metres, NumPy or tensor; NaN or <= 0: a hole) seen through the pinhole ``K``
        from ``T_sensor_to_map`` ([4, 4]; a float64 device tensor is read in place by the kernel, e.g. the pose
        ``CameraTracker.track`` just returned).  ``skip_if``: an int32 device tensor; if its first word is nonzero
        when the kernel runs, the call changes nothing (the status of an alignment: lost frames stay out).
        ``color`` (a volume with ``colors=True``): the frame's uint8 [H, W, 3] image, NumPy or tensor; after the depth
        every voxel the frame wrote within the truncation of the surface averages its pixel's colour into ``colors``
        (a second launch on the same stream, pose tensor and skip word; the (tsdf, weight) bytes are the same)."""
        camera = _camera(K)
        d = _depth_tensor(depth, self.device, 3)
        if d.shape[0] != 1:
            raise ValueError(f"depth must be one [H, W] image, got {tuple(d.shape)}")
        rgb = self._color_image_of(color, d.shape[1:])
        if skip_if is not None:
            if not isinstance(skip_if, torch.Tensor) or skip_if.dtype != torch.int32 or skip_if.numel() < 1:
                raise TypeError("skip_if must be an int32 tensor on the volume's device")
            if skip_if.device != d.device:
                raise ValueError(f"skip_if on {skip_if.device}, the volume on {d.device}")
        T = self._pose(T_sensor_to_map)
        tensors = (self.volume, d, T) + (() if skip_if is None else (skip_if,))
        _lib.require_gpu(*tensors)
        _lib.check(_lib.lib().mf_tsdf_integrate(
            _lib.ptr(self.volume), *self._grid, self.truncation, self.max_weight, _lib.ptr(d), *_view(d, camera),
            _lib.ptr(T), _lib.ptr(skip_if), _lib.stream_ptr()), "mf_tsdf_integrate")
        if rgb is not None:
            self._integrate_colors(d, rgb, camera, T, skip_if)
        return self

    def color_image(self, depth, K, T_sensor_to_map):
        """The fused colour under every pixel of ``depth`` (float [H, W] seen through ``K`` from ``T_sensor_to_map``;
        meant for ``raycast``'s or ``render``'s depth from the same pose) -> uint8 [H, W, 4] device tensor of
        (r, g, b, alpha): the colour at the pixel's point, trilinear over the coloured corners of its cell, alpha 255;
        (0, 0, 0, 0) where there is no depth, outside the volume and where no corner has a colour."""
        if self.colors is None:
            raise TypeError("color_image needs a volume built with colors=True")
        camera = _camera(K)
        d = _depth_tensor(depth, self.device, 3)
        if d.shape[0] != 1:
            raise ValueError(f"depth must be one [H, W] image, got {tuple(d.shape)}")
        T = self._pose(T_sensor_to_map)
        out = torch.empty(tuple(d.shape[1:]) + (4,), dtype=torch.uint8, device=self.device)
        _lib.require_gpu(self.colors, d, T, out)
        _lib.check(_lib.lib().mf_tsdf_color_image(
            _lib.ptr(self.colors), *self._grid, _lib.ptr(d), *_view(d, camera), _lib.ptr(T), _lib.ptr(out),
            _lib.stream_ptr()), "mf_tsdf_color_image")
        return out

    def sample_colors(self, points):
        """The fused colour at map-frame ``points`` ([N, 3], NumPy or tensor: mesh vertices, instance centres, ICP
        targets) -> uint8 [N, 4] device tensor of (r, g, b, alpha), ``color_image``'s rule per point.  No points: an
        empty tensor and no launch."""
        if self.colors is None:
            raise TypeError("sample_colors needs a volume built with colors=True")
        p = points.detach() if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
        if p.dim() != 2 or p.shape[1] != 3:
            raise ValueError(f"points must be [N, 3], got {tuple(p.shape)}")
        p = p.to(device=self.device, dtype=torch.float64).contiguous()
        out = torch.empty((p.shape[0], 4), dtype=torch.uint8, device=self.device)
        if p.shape[0] == 0:
            return out
        _lib.require_gpu(self.colors, p, out)
        _lib.check(_lib.lib().mf_tsdf_sample_colors(
            _lib.ptr(self.colors), *self._grid, _lib.ptr(p), int(p.shape[0]), _lib.ptr(out), _lib.stream_ptr()),
            "mf_tsdf_sample_colors")
        return out

    def raycast(self, K, T_sensor_to_map, height, width, step=None, min_depth=0.0, max_depth=None, return_code=False):
        """The fused surface seen through ``K`` from ``T_sensor_to_map``: a float32 [height, width] device tensor of
        camera-frame depths, 0 where the ray finds no surface (the tracker's "no depth").  The ray is sampled every
        ``step`` metres of depth (default ``truncation / 2``) between ``min_depth`` and ``max_depth`` (default: no
        limit) inside the volume and the zero crossing is interpolated between the two samples around it.  With
        ``return_code`` also a uint8 image of how each ray ended (``RAY_HIT`` .. ``RAY_CAP``)."""
        camera, (height, width), (step, min_depth, max_depth, max_steps) = self._ray_arguments(
            K, height, width, step, min_depth, max_depth)
        T = self._pose(T_sensor_to_map)
        depth = torch.empty((height, width), dtype=torch.float32, device=self.device)
        code = torch.empty((height, width), dtype=torch.uint8, device=self.device) if return_code else None
        _lib.require_gpu(self.volume, T, depth)
        _lib.check(_lib.lib().mf_tsdf_raycast(
            _lib.ptr(self.volume), *self._grid, step, min_depth, max_depth, max_steps, height, width, *camera,
            _lib.ptr(T), _lib.ptr(depth), _lib.ptr(code), _lib.stream_ptr()), "mf_tsdf_raycast")
        return (depth, code) if return_code else depth

    def _ray_arguments(self, K, height, width, step, min_depth, max_depth):
        """The checks and defaults that ``raycast`` and ``render`` share -> ((fx, fy, cx, cy), (height, width), (step,
        min_depth, max_depth, max_steps))."""
        camera = _camera(K)
        height, width = int(height), int(width)
        if height < 1 or width < 1:
            raise ValueError(f"height x width = {height} x {width}: each >= 1")
        step = self.truncation / 2.0 if step is None else float(step)
        if not step > 0:
            raise ValueError(f"step = {step}: must be > 0")
        min_depth = float(min_depth)
        max_depth = math.inf if max_depth is None else float(max_depth)
        if not 0 <= min_depth < max_depth:
            raise ValueError(f"min_depth = {min_depth}, max_depth = {max_depth}: 0 <= min_depth < max_depth")
        max_steps = self.max_steps(step)
        if max_steps > MAX_STEPS:
            raise ValueError(f"step = {step}: {max_steps} samples per ray, at most {MAX_STEPS}")
        return camera, (height, width), (step, min_depth, max_depth, max_steps)

    def summary_shape(self, block=8):
        """(nb_z, nb_y, nb_x) of ``block_summary``: ``ceil((n - 1) / block)`` blocks of cells per axis."""
        block = int(block)
        if block not in BLOCK_EDGES:
            raise ValueError(f"block = {block}: one of {BLOCK_EDGES}")
        nx, ny, nz = self.dims
        return tuple((n - 2) // block + 1 for n in (nz, ny, nx))

    def block_summary(self, block=8):
        """The coarse occupancy that ``render`` skips with: a uint8 device tensor ``[nb_z, nb_y, nb_x]`` with one code
        per block of ``block``^3 cells (2, 4, 8 or 16) -- ``BLOCK_FREE`` if every voxel the block's cells touch was
        seen (weight > 0) with tsdf exactly 1, ``BLOCK_UNKNOWN`` if none of them was seen, ``BLOCK_MIXED`` otherwise.
        One launch that reads the volume once.  It describes the volume as it is now: any integrate makes it stale."""
        summary = torch.empty(self.summary_shape(block), dtype=torch.uint8, device=self.device)
        _lib.require_gpu(self.volume, summary)
        _lib.check(_lib.lib().mf_tsdf_block_summary(_lib.ptr(self.volume), *self.dims, int(block), _lib.ptr(summary),
                                                    _lib.stream_ptr()), "mf_tsdf_block_summary")
        return summary

    def _render(self, K, T_sensor_to_map, height, width, step, min_depth, max_depth, block, summary, labels, min_count,
                want_code, want_stats):
        """-> (depth, label or None, code or None, stats or None) of one ``mf_tsdf_render`` launch."""
        camera, (height, width), (step, min_depth, max_depth, max_steps) = self._ray_arguments(
            K, height, width, step, min_depth, max_depth)
        shape = self.summary_shape(block)
        if summary is None:
            summary = self.block_summary(block)
        elif (not isinstance(summary, torch.Tensor) or summary.dtype != torch.uint8 or tuple(summary.shape) != shape
              or not summary.is_contiguous()):
            raise ValueError(f"summary must be a contiguous uint8 tensor {shape}: block_summary({int(block)})")
        elif summary.device != self.volume.device:
            raise ValueError(f"summary on {summary.device}, the volume on {self.volume.device}")
        T = self._pose(T_sensor_to_map)
        new = lambda dtype, *tail: torch.empty((height, width) + tail, dtype=dtype, device=self.device)  # noqa: E731
        depth = new(torch.float32)
        label = None if labels is None else new(torch.int32)
        code = new(torch.uint8) if want_code else None
        stats = new(torch.int32, 2) if want_stats else None
        _lib.require_gpu(self.volume, summary, T, depth, *(() if labels is None else (labels,)))
        _lib.check(_lib.lib().mf_tsdf_render(
            _lib.ptr(self.volume), *self._grid, step, min_depth, max_depth, max_steps, height, width, *camera,
            _lib.ptr(T), _lib.ptr(summary), int(block), _lib.ptr(labels), int(min_count), _lib.ptr(depth),
            _lib.ptr(code), _lib.ptr(label), _lib.ptr(stats), _lib.stream_ptr()), "mf_tsdf_render")
        return depth, label, code, stats

    def render(self, K, T_sensor_to_map, height, width, step=None, min_depth=0.0, max_depth=None, block=8,
               summary=None, return_code=False, return_stats=False):
        """``raycast`` (same arguments, same checks, the same bytes in depth and code) without the loads that free and
        unseen space cost: a sample inside a ``BLOCK_FREE`` or ``BLOCK_UNKNOWN`` block of ``block_summary(block)`` reads
        one byte of the summary, and the ray goes to its last sample inside such a block in one step (csrc/tsdfrender.hip,
        include/mfhip.h "TSDF render").  The summary is made again on every call -- one read of the volume -- unless
        ``summary`` is given; a summary made before the last integrate is stale and gives a wrong render: passing one is
        the caller's risk.  ``return_stats``: also an int32 ``[height, width, 2]`` tensor of (samples evaluated by
        loading voxels, samples whose position was computed) per ray.  -> depth, then code and stats if asked for."""
        depth, _, code, stats = self._render(K, T_sensor_to_map, height, width, step, min_depth, max_depth, block,
                                             summary, None, 1, return_code, return_stats)
        out = (depth,) + ((code,) if return_code else ()) + ((stats,) if return_stats else ())
        return out if len(out) > 1 else depth

    def extract_mesh(self, min_weight=1.0, normals=False, colors=False):
        """The fused surface as a welded triangle mesh (csrc/tsdfmesh.hip, include/mfhip.h "TSDF mesh"): ``(vertices
        float64 [V, 3], faces int32 [F, 3])`` on the volume's device, in the map frame, plus ``normals`` float64
        [V, 3] (unit, towards positive tsdf: out of the surface) when asked for.  The surface is the zero level of
        the tsdf (``tsdf <= 0`` is inside) over the six-tetrahedra subdivision of the cells whose eight corners all
        have ``weight >= min_weight``: what the camera never saw is left out, so the mesh is open where the
        observation ends.  Faces are counter-clockwise seen from the outside; vertex and face order are fixed by the
        volume alone.  One read-back: the two totals, to size the outputs.  An empty surface gives empty tensors.
        ``colors`` (a volume with ``colors=True``): also ``sample_colors(vertices)``, uint8 [V, 4], last in the tuple;
        no further read-back."""
        min_weight = float(min_weight)
        if not min_weight > 0:
            raise ValueError(f"min_weight = {min_weight}: must be > 0")
        if colors and self.colors is None:
            raise TypeError("extract_mesh(colors=True) needs a volume built with colors=True")
        L = _lib.lib()
        nbytes = L.mf_tsdfmesh_workspace_bytes(*self.dims)
        if nbytes < 0:
            raise ValueError(f"dims = {self.dims}: refused by mf_tsdfmesh_workspace_bytes")
        workspace = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=self.device)
        totals = torch.empty(2, dtype=torch.int64, device=self.device)
        _lib.require_gpu(self.volume, workspace, totals)
        _lib.check(L.mf_tsdfmesh_count(_lib.ptr(self.volume), *self.dims, min_weight, _lib.ptr(workspace),
                                       _lib.ptr(totals), _lib.stream_ptr()), "mf_tsdfmesh_count")
        n_vertices, n_faces = totals.cpu().tolist()  # the call's read-back
        if n_vertices >= 1 << 31 or n_faces >= 1 << 31:
            raise ValueError(f"{n_vertices} vertices, {n_faces} faces: each must be below 2^31")
        vertices = torch.empty((n_vertices, 3), dtype=torch.float64, device=self.device)
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device=self.device)
        normal = torch.empty((n_vertices, 3), dtype=torch.float64, device=self.device) if normals else None
        if n_vertices > 0:
            _lib.check(L.mf_tsdfmesh_emit(
                _lib.ptr(self.volume), *self._grid, min_weight, _lib.ptr(workspace), n_vertices, n_faces,
                _lib.ptr(vertices), _lib.ptr(faces), _lib.ptr(normal), _lib.stream_ptr()), "mf_tsdfmesh_emit")
        out = (vertices, faces, normal) if normals else (vertices, faces)
        return out + (self.sample_colors(vertices),) if colors else out


class ModelTracker:
    """Track a depth sequence of ``height`` x ``width`` images against the fused model in ``volume``.

    ``track(depth)`` returns ``T_cur_to_map`` (a float64 [4, 4] device tensor).  The first call integrates the image
    at ``T_first`` (default: the identity) and returns ``T_first``.  Every later call ray-casts the volume from the
    last pose, installs that render as the reference of its ``CameraTracker`` (``set_reference``), aligns the image
    to it starting from the last pose and integrates the image at the pose found -- unless the alignment was lost:
    the kernel reads the tracker's status word on the device and leaves the model untouched, and the pose returned is
    the last one (``CameraTracker`` restores the initial pose).  Nothing is read back in the loop.
    ``track(depth, label)`` also fuses the frame's instance labels; ``volume`` must then be an ``InstanceTsdfVolume``.
    ``tracker_kwargs`` go to ``CameraTracker`` (levels, iterations, block_band, the thresholds, min_pairs).
    ``skip_empty``: the reference comes from ``volume.render(..., block=block)`` -- the same bytes as the ray-cast's,
    so the same poses and the same model; the summary is made again for every frame, on the device.

    ``status`` / ``lost`` / ``stats`` are the inner tracker's, read back only when asked for."""

    def __init__(self, K, height, width, volume, T_first=None, skip_empty=False, block=8, **tracker_kwargs):
        if not isinstance(volume, TsdfVolume):
            raise TypeError(f"volume must be a TsdfVolume, got {type(volume).__name__}")
        self.skip_empty, self.block = bool(skip_empty), int(block)
        volume.summary_shape(self.block)  # (refuses a block edge that is not allowed)
        for name in ("reference", "device"):
            if name in tracker_kwargs:
                raise TypeError(f"{name} is fixed by ModelTracker: the reference is the model, the device the volume's")
        _camera(K)
        self.K, self.height, self.width, self.volume = K, int(height), int(width), volume
        self.tracker = CameraTracker(K, height, width, reference="first", T_first=T_first, device=volume.device,
                                     **tracker_kwargs)
        self._T_first = _pose_tensor(np.eye(4) if T_first is None else T_first, 1, volume.device, "T_first")[0].clone()
        self._T_last = None

    def track(self, depth, label=None, color=None):
        """``label``: the frame's instance labels, fused next to its depth by ``InstanceTsdfVolume.integrate`` under
        the same device skip word (the labels do not move the camera) -- an integer [H, W] image, or a callable that
        gets the pose just found (float64 [4, 4] device tensor) and returns one, for labels that are made with the
        pose.  None: the plain integrate.  ``color``: the frame's uint8 [H, W, 3] image, fused into the colours of a
        volume built with ``colors=True`` under that skip word too (the colour does not move the camera either)."""
        if label is not None and not hasattr(self.volume, "labels"):
            raise TypeError(f"labels need an InstanceTsdfVolume, the volume is a {type(self.volume).__name__}")
        if color is not None and self.volume.colors is None:
            raise TypeError("color= needs a volume built with colors=True")
        fused = {} if color is None else dict(color=color)
        labelled = lambda T: dict(fused, **({} if label is None else  # noqa: E731
                                            dict(label=label(T) if callable(label) else label)))
        d = self.tracker._depth(depth)[0]
        if self._T_last is None:
            self.volume.integrate(d, self.K, self._T_first, **labelled(self._T_first))
            self._T_last = self._T_first
            return self._T_last.clone()
        if self.skip_empty:
            reference = self.volume.render(self.K, self._T_last, self.height, self.width, block=self.block)
        else:
            reference = self.volume.raycast(self.K, self._T_last, self.height, self.width)
        self.tracker.set_reference(reference, self._T_last)
        T = self.tracker.track(d, T_init=self._T_last)
        # (the device word: no read-back)
        self.volume.integrate(d, self.K, T, skip_if=self.tracker._al.status, **labelled(T))
        self._T_last = T
        return T.clone()

    @property
    def status(self):
        return self.tracker.status

    @property
    def lost(self):
        return self.tracker.lost

    @property
    def stats(self):
        return self.tracker.stats
