"""OccupancyRegistration -- single-object pose registration against occupancy grids.

API of morefusion/contrib/occupancy_registration.py:10-139: the
predecessor of ICC.  The soft occupancy grid of the transformed source points is rewarded
for overlapping ``grid_target[0]`` (occupied) and penalised for overlapping
``grid_target[1]`` (or ``max(grid_target[1], grid_target[2])``).  The reference builds
the grid from three dense [X,Y,Z,P] tensors per iteration; here it is the fused HIP
``occupancy_grid_3d`` (csrc/occgrid_knn.hip), so one iteration is a handful of launches.

``occupancy_registration_batch`` runs every iteration of every object of a frame in one launch
(csrc/occreg.hip, DESIGN.md "Occupancy registration"); ``OccupancyRegistration.register_fused`` is the
single-object door to it.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .. import functions as functions_module
from .. import geometry as geometry_module
from ..geometry.quaternion_from_matrix import quaternion_from_matrix, translation_from_matrix
from ..optimizers import Adam


MAX_THRESHOLD = 64.0  # MF_OCCREG_MAX_THRESHOLD (include/mfhip.h)


class OccupancyRegistrationLink(torch.nn.Module):
    def __init__(self, quaternion_init=None, translation_init=None):
        super().__init__()
        if quaternion_init is None:
            quaternion_init = np.array([1, 0, 0, 0], dtype=np.float32)
        if translation_init is None:
            translation_init = np.zeros((3,), dtype=np.float32)
        self.quaternion = torch.nn.Parameter(torch.as_tensor(quaternion_init, dtype=torch.float32))
        self.translation = torch.nn.Parameter(torch.as_tensor(translation_init, dtype=torch.float32))

    @property
    def xp(self):
        """``link.xp`` of the reference's call sites (``link.xp.asarray(points)``): arrays on this link's device."""
        from ..chainer_compat import link_xp
        return link_xp(self)

    def to_gpu(self, device=None):
        return self.to("cuda" if device is None else f"cuda:{device}")

    def cleargrads(self):
        for p in self.parameters():
            p.grad = None

    def forward(self, points_source, grid_target, *, pitch, origin, threshold):
        if grid_target.dtype != torch.float32 or grid_target.shape[0] not in (2, 3):
            raise TypeError("grid_target must be float32 [2|3, X, Y, Z]")
        transform = functions_module.transformation_matrix(self.quaternion, self.translation)
        moved = functions_module.transform_points(points_source, transform)
        grid_source = functions_module.occupancy_grid_3d(
            moved, pitch=pitch, origin=origin, dims=tuple(grid_target.shape[1:]), threshold=threshold)
        occupied = grid_target[0]
        reward = (occupied * grid_source).sum() / occupied.sum()
        unoccupied = grid_target[1] if grid_target.shape[0] == 2 else torch.maximum(grid_target[1], grid_target[2])
        penalty = (unoccupied * grid_source).sum() / grid_source.sum()
        return penalty - reward


class OccupancyRegistration:
    def __init__(self, points_source, grid_target, *, pitch, origin, threshold, transform_init,
                 gpu=0, alpha=0.1):
        if gpu < 0:
            raise RuntimeError("OccupancyRegistration runs on the MI355X (gpu >= 0)")
        transform_init = np.asarray(transform_init)
        link = OccupancyRegistrationLink(quaternion_from_matrix(transform_init).astype(np.float32),
                                         translation_from_matrix(transform_init).astype(np.float32))
        link.to_gpu(gpu)
        dev = link.quaternion.device
        self._points_source = torch.as_tensor(points_source, dtype=torch.float32).to(dev)
        self._grid_target = torch.as_tensor(grid_target, dtype=torch.float32).to(dev)
        self._pitch, self._origin, self._threshold = pitch, origin, threshold
        self._optimizer = Adam(alpha=alpha).setup(link)
        link.translation.update_rule.hyperparam.alpha *= 0.1

    @property
    def _transform(self):
        link = self._optimizer.target
        with torch.no_grad():
            R = functions_module.quaternion_matrix(link.quaternion)[:3, :3]
            return geometry_module.compose_transform(R, link.translation).cpu().numpy()

    def register_iterative(self, iteration=None):
        iteration = 100 if iteration is None else iteration
        yield self._transform
        link = self._optimizer.target
        for _ in range(iteration):
            loss = link(points_source=self._points_source, grid_target=self._grid_target,
                        pitch=self._pitch, origin=self._origin, threshold=self._threshold)
            loss.backward()
            self._optimizer.update()
            link.cleargrads()
            yield self._transform

    def register(self, iteration=None):
        for _ in self.register_iterative(iteration=iteration):
            pass
        return self._transform

    def register_fused(self, iteration=None):
        """``register`` from this object's CURRENT pose through ``occupancy_registration_batch`` (one launch, fresh
        Adam moments, no per-step readback); the link is left at the refined pose.  Returns the same 4 x 4."""
        link = self._optimizer.target
        alpha = self._optimizer.hyperparam.alpha
        res = occupancy_registration_batch(
            [self._points_source], [self._grid_target], pitch=self._pitch, origin=_lib.as_float3(self._origin),
            threshold=self._threshold, transforms_init=self._transform[None],
            iteration=100 if iteration is None else iteration, alpha=alpha, return_history=True,
            pose_init=(link.quaternion.detach()[None], link.translation.detach()[None]))
        pose = res[3][-1, 0]
        with torch.no_grad():
            if not bool(res[1][0]):
                link.quaternion.copy_(pose[:4])
                link.translation.copy_(pose[4:])
        return self._transform


def _per_object(value, B, width, name):
    """scalar, [width] (width > 1) or [B(, width)] -> float32 [B, width]"""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    a = np.asarray(value, dtype=np.float32)
    if a.ndim == 0:
        a = np.full((B, width), float(a), np.float32)
    elif width > 1 and a.shape == (width,):
        a = np.tile(a[None], (B, 1))
    elif a.shape == (B,) and width == 1:
        a = a.reshape(B, 1)
    if a.shape != (B, width):
        raise ValueError(f"{name} must be a scalar or have one {'row of ' + str(width) if width > 1 else 'value'} "
                         f"per object; got shape {tuple(np.shape(value))} for {B} objects")
    return np.ascontiguousarray(a)


def occupancy_registration_batch(points_source, grids_target, *, pitch, origin, threshold, transforms_init,
                                 iteration=100, alpha=0.1, active=None, return_history=False, device=None,
                                 pose_init=None):
    """``OccupancyRegistration(points_source[b], grids_target[b], pitch=pitch[b], origin=origin[b],
    threshold=threshold[b], transform_init=transforms_init[b], alpha=alpha).register(iteration)`` for every b in one
    launch: a workgroup per object runs all iterations on the device (csrc/occreg.hip).

    points_source: list of B [P_b, 3] clouds.  grids_target: list of B float32 [2 | 3, X_b, Y_b, Z_b] arrays or one
    stacked tensor [B, 2 | 3, X, Y, Z] (channel 0 occupied; unoccupied = channel 1, or max(channel 1, channel 2)).
    pitch, threshold: scalar or [B]; origin: [3] or [B, 3].  transforms_init: [B, 4, 4].  active: [B] bool (False:
    the pose passes through).  pose_init: optional (quaternion [B, 4] wxyz, translation [B, 3]) to start from instead
    of the decomposition of ``transforms_init`` (which is still what a NaN or inactive object returns) -- for callers
    that hold the pose in that form, so that it is not taken through a matrix and back.  threshold: at most 64 voxels
    (``MF_OCCREG_MAX_THRESHOLD``).  The translation's step size is ``alpha`` x 0.1 and Adam starts fresh, as in
    ``OccupancyRegistration``.

    Returns device tensors ``(transform [B, 4, 4] float32, nan [B] bool)``: where a loss or the refined pose is not
    finite, ``nan`` is set and the transform is ``transforms_init[b]``.  With ``return_history`` also
    ``losses [iteration, B]`` and ``trajectory [iteration + 1, B, 7]`` (quaternion wxyz then translation; entry 0 the
    initial pose)."""
    iteration = int(iteration)
    if iteration < 0:
        raise ValueError("iteration must be >= 0")
    if not isinstance(points_source, (list, tuple)):
        raise TypeError("points_source must be a list of [P, 3] arrays")
    B = len(points_source)
    if B == 0:
        raise ValueError("no objects")
    if isinstance(grids_target, (list, tuple)):
        grids = list(grids_target)
    elif isinstance(grids_target, (torch.Tensor, np.ndarray)) and grids_target.ndim == 5:
        grids = [grids_target[b] for b in range(grids_target.shape[0])]
    else:
        raise TypeError("grids_target must be a list of [2|3, X, Y, Z] arrays or one [B, 2|3, X, Y, Z] tensor")
    if len(grids) != B:
        raise ValueError(f"{len(grids)} target grids for {B} objects")
    if device is None:
        cand = [x for x in list(points_source) + grids if isinstance(x, torch.Tensor)]
        device = cand[0].device if cand else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    f32 = dict(dtype=torch.float32, device=device)

    def dev(x):
        return x.detach().to(device) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(device)

    pts, pts_off, occ, unocc, dims, grid_off = [], [0], [], [], [], [0]
    for b in range(B):
        g = grids[b]
        g_dtype = g.dtype if isinstance(g, torch.Tensor) else torch.from_numpy(np.empty(0, np.asarray(g).dtype)).dtype
        if g_dtype != torch.float32 or g.ndim != 4 or g.shape[0] not in (2, 3):
            raise TypeError("grid_target must be float32 [2|3, X, Y, Z]")  # (OccupancyRegistrationLink.forward)
        g = dev(g)
        p = dev(points_source[b]).to(torch.float32)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"points_source[{b}] must be [P, 3], got {tuple(p.shape)}")
        pts.append(p)
        pts_off.append(pts_off[-1] + p.shape[0])
        occ.append(g[0].reshape(-1))
        unocc.append((g[1] if g.shape[0] == 2 else torch.maximum(g[1], g[2])).reshape(-1))
        dims.append([int(d) for d in g.shape[1:]])
        grid_off.append(grid_off[-1] + dims[-1][0] * dims[-1][1] * dims[-1][2])
    pitch_h = _per_object(pitch, B, 1, "pitch").reshape(B)
    thr_h = _per_object(threshold, B, 1, "threshold").reshape(B)
    origin_h = _per_object(origin, B, 3, "origin")
    if not (np.isfinite(pitch_h).all() and (pitch_h > 0).all()):
        raise ValueError("pitch must be finite and positive")
    if not (np.isfinite(thr_h).all() and (thr_h > 0).all()):
        raise ValueError("threshold must be finite and positive")
    if (thr_h > MAX_THRESHOLD).any():
        raise ValueError(f"threshold must be at most {MAX_THRESHOLD:g} voxels (MF_OCCREG_MAX_THRESHOLD)")
    if isinstance(transforms_init, torch.Tensor):
        init = transforms_init.detach().to(device=device, dtype=torch.float32)
    else:
        init = torch.as_tensor(np.asarray(transforms_init, np.float32)).to(device)
    if tuple(init.shape) != (B, 4, 4):
        raise ValueError(f"transforms_init must be [{B}, 4, 4], got {tuple(init.shape)}")
    if pose_init is None:
        init_h = init.cpu().numpy().astype(np.float64)
        q = torch.as_tensor(np.stack([quaternion_from_matrix(T) for T in init_h]).astype(np.float32)).to(device)
        t = torch.as_tensor(np.stack([translation_from_matrix(T) for T in init_h]).astype(np.float32)).to(device)
    else:
        q, t = (torch.as_tensor(x).detach().to(**f32).clone() for x in pose_init)
        if tuple(q.shape) != (B, 4) or tuple(t.shape) != (B, 3):
            raise ValueError(f"pose_init must be (quaternion [{B}, 4], translation [{B}, 3])")
    q, t = q.contiguous(), t.contiguous()
    act = None
    if active is not None:
        act = torch.as_tensor(np.asarray(active.cpu() if isinstance(active, torch.Tensor) else active)).reshape(-1)
        if act.shape[0] != B:
            raise ValueError("active must have one flag per object")
        act = act.to(device=device).to(torch.uint8).contiguous()

    L = _lib.lib()
    max_vox = max(d[0] * d[1] * d[2] for d in dims)
    ws_bytes = L.mf_occreg_workspace_bytes(B, pts_off[-1], max_vox)
    if ws_bytes < 0:
        raise ValueError(f"{B} objects, {pts_off[-1]} points, grids of up to {max_vox} voxels: outside the limits of "
                         "mf_occreg (include/mfhip.h)")
    points = (torch.cat(pts) if pts_off[-1] else torch.zeros((1, 3), **f32)).contiguous()
    occ_d, unocc_d = torch.cat(occ).contiguous(), torch.cat(unocc).contiguous()
    if device.type == "cuda":
        _lib.require_gpu(points, occ_d, unocc_d, q, t)
    host = dict(pts_off=np.asarray(pts_off, np.int32), pitch=pitch_h, dims=np.asarray(dims, np.int32).reshape(B, 3),
                threshold=thr_h)
    on_dev = {k: torch.from_numpy(v).to(device) for k, v in host.items()}
    origin_d = torch.from_numpy(origin_h).to(device)
    grid_off_d = torch.tensor(grid_off, dtype=torch.int32, device=device)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=device)
    d = _lib.OccRegBatch()
    d.points, d.pts_off, d.pitch, d.origin = _lib.ptr(points), _lib.ptr(on_dev["pts_off"]), _lib.ptr(on_dev["pitch"]), \
        _lib.ptr(origin_d)
    d.dims, d.threshold = _lib.ptr(on_dev["dims"]), _lib.ptr(on_dev["threshold"])
    d.grid_occ, d.grid_unocc, d.grid_off, d.active = _lib.ptr(occ_d), _lib.ptr(unocc_d), _lib.ptr(grid_off_d), \
        _lib.ptr(act)
    d.host_pts_off, d.host_pitch = host["pts_off"].ctypes.data, host["pitch"].ctypes.data
    d.host_dims, d.host_threshold = host["dims"].ctypes.data, host["threshold"].ctypes.data
    d.n_objects, d.n_points_total, d.max_voxels, d.reserved = B, pts_off[-1], max_vox, 0
    adam_m, adam_v = torch.zeros((B, 7), **f32), torch.zeros((B, 7), **f32)
    losses = torch.zeros((iteration, B), **f32)
    traj = torch.empty((iteration + 1, B, 7), **f32) if return_history else None
    alpha = float(alpha)
    _lib.check(L.mf_occreg_refine(ctypes.byref(d), _lib.ptr(q), _lib.ptr(t), _lib.ptr(adam_m), _lib.ptr(adam_v),
                                  iteration, 0, alpha, alpha * 0.1, _lib.ptr(losses), _lib.ptr(traj), _lib.ptr(ws),
                                  _lib.stream_ptr()), "mf_occreg_refine")
    nan = ~(torch.isfinite(losses).all(dim=0) & torch.isfinite(q).all(dim=1) & torch.isfinite(t).all(dim=1))
    transform = functions_module.quaternion_matrix(q)  # composed as OccupancyRegistration._transform does
    transform[:, :3, 3] = t
    keep = nan if act is None else nan | (act == 0)
    transform = torch.where(keep[:, None, None], init, transform)
    if return_history:
        return transform, nan, losses, traj
    return transform, nan
