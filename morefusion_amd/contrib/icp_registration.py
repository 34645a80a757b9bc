"""ICPRegistration -- open3d's point-to-point ICP on the device, batched over objects.

Call surface of morefusion/contrib/icp_registration.py (``register`` / ``register_iterative``) over
csrc/icpreg.hip (include/mfhip.h ``mf_icpreg_*``): voxel_down_sample of both clouds, nearest target
within ``2 * voxel_size``, closed-form Umeyama update per iteration.  ``icp_registration_batch`` is the
node's refinement loop (ros/.../singleview_3d_pose_estimation.py:236-262) in one call: B objects, one
workgroup each, every iteration in one launch.  DESIGN.md "ICP registration" has the precision contract.

Host synchronisation: each batch reads back ONE small int32 array -- the voxel extents of every set
that is down-sampled, [n_sets, 4] -- to size the voxel boxes.  Prepared CAD targets (down-sampled cloud
+ grid) can be kept per ``(key, voxel_size)`` (``cad_keys``), so a stream of frames prepares each class once.
"""
import collections
import math

import numpy as np
import torch

from .. import _lib

_CELL_FACTOR = 1.0009765625  # target grid cell = r * (1 + 2^-10): >= r, so the 27 cells hold every point within r
_CACHE_SIZE = 64


def _device_of(*xs, device=None):
    if device is not None:
        return torch.device(device)
    for x in xs:
        if isinstance(x, torch.Tensor):
            return x.device
        if isinstance(x, (list, tuple)):
            for y in x:
                if isinstance(y, torch.Tensor):
                    return y.device
    return torch.device("cuda")


def _rows(x, device):
    """Any [..., 3] array / tensor -> contiguous float64 [n, 3] on ``device``."""
    t = torch.as_tensor(x) if not isinstance(x, torch.Tensor) else x.detach()
    if t.shape[-1] != 3:
        raise ValueError(f"points must be [..., 3], got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()


def _pack(sets, device):
    """list of [..., 3] | [n, ..., 3] tensor (one set per leading index) | (packed [N, 3], offsets [B + 1])
    -> packed float64 [N, 3], host row offsets (list)."""
    if isinstance(sets, tuple) and len(sets) == 2 and torch.as_tensor(sets[1]).dim() == 1:
        off = [int(o) for o in torch.as_tensor(sets[1]).tolist()]
        return _rows(sets[0], device), off
    if isinstance(sets, (np.ndarray, torch.Tensor)):
        if sets.ndim < 3:
            raise ValueError("a single array is one set per leading index: [n, ..., 3]")
        n = sets.shape[0]
        per = int(np.prod(sets.shape[1:-1]))
        return _rows(sets, device), [b * per for b in range(n + 1)]
    parts = [_rows(s, device) for s in sets]
    off = [0]
    for p in parts:
        off.append(off[-1] + p.shape[0])
    packed = torch.cat(parts) if parts else torch.zeros((0, 3), dtype=torch.float64, device=device)
    return packed, off


class _Target:
    """A down-sampled CAD cloud and its grid (views into one prepare call's outputs)."""

    def __init__(self, pts, cnt, grid_origin, grid_dim, grid_start, grid_idx):
        self.pts, self.cnt, self.grid_origin = pts, cnt, grid_origin
        self.grid_dim, self.grid_start, self.grid_idx = grid_dim, grid_start, grid_idx


_CACHE = collections.OrderedDict()  # (key, voxel_size, device) -> _Target


def clear_cache():
    _CACHE.clear()


def _grid_dims(ext, voxel_size, cell):
    return [math.floor(int(n) * voxel_size / cell) + 3 for n in ext[:3]] if int(ext[3]) > 0 else [0, 0, 0]


def _prepare(packed, off, voxel_size, gridded, device):
    """bounds -> (readback of the extents) -> down-sample (+ grid the sets flagged in ``gridded``).
    Returns out [N, 3], out_cnt [n_sets] int32 (device), and the grid arrays + host offsets."""
    L = _lib.lib()
    n_sets = len(off) - 1
    if device.type == "cuda":
        _lib.require_gpu(packed)
    off_d = torch.tensor(off, dtype=torch.int64, device=device)
    vmin = torch.empty((n_sets, 3), dtype=torch.float64, device=device)
    ext = torch.empty((n_sets, 4), dtype=torch.int32, device=device)
    _lib.check(L.mf_icpreg_bounds(_lib.ptr(packed), _lib.ptr(off_d), n_sets, float(voxel_size), _lib.ptr(vmin),
                                  _lib.ptr(ext), _lib.stream_ptr()), "mf_icpreg_bounds")
    ext_h = ext.cpu().tolist()  # the batch's one readback
    cell = 2.0 * voxel_size * _CELL_FACTOR
    box_off, grid_off, grid_dim = [0], [0], []
    for e, g in zip(ext_h, gridded):
        if min(e[:3]) < 0:
            raise ValueError(f"point set spans too many voxels of {voxel_size} (extents {e[:3]})")
        box_off.append(box_off[-1] + e[0] * e[1] * e[2])
        d = _grid_dims(e, voxel_size, cell) if g else [0, 0, 0]
        grid_dim.append(d)
        grid_off.append(grid_off[-1] + (d[0] * d[1] * d[2] + 1 if g and e[3] > 0 else 0))
    n_points = packed.shape[0]
    ws_bytes = L.mf_icpreg_workspace_bytes(box_off[-1], grid_off[-1], n_points)
    if ws_bytes < 0:
        raise ValueError(f"voxel boxes of {box_off[-1]} / grids of {grid_off[-1]} cells: past the cap of "
                         f"{1 << 24} cells per call (use a larger voxel_size or smaller batches)")
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=device)
    out = torch.full((n_points, 3), float("nan"), dtype=torch.float64, device=device)  # rows past out_cnt: NaN
    out_cnt = torch.empty(n_sets, dtype=torch.int32, device=device)
    grid_origin = torch.zeros((n_sets, 3), dtype=torch.float64, device=device)
    grid_start = torch.empty(grid_off[-1] + 1, dtype=torch.int32, device=device)
    grid_idx = torch.empty(n_points + 1, dtype=torch.int32, device=device)
    box_off_d = torch.tensor(box_off, dtype=torch.int64, device=device)
    grid_off_d = torch.tensor(grid_off, dtype=torch.int64, device=device)
    grid_dim_d = torch.tensor(grid_dim, dtype=torch.int32, device=device).reshape(n_sets, 3)
    _lib.check(L.mf_icpreg_prepare(_lib.ptr(packed), _lib.ptr(off_d), n_sets, float(voxel_size), _lib.ptr(vmin),
                                   _lib.ptr(ext), _lib.ptr(box_off_d), box_off[-1], _lib.ptr(grid_off_d),
                                   _lib.ptr(grid_dim_d), grid_off[-1], cell, n_points, _lib.ptr(ws), _lib.ptr(out),
                                   _lib.ptr(out_cnt), _lib.ptr(grid_origin), _lib.ptr(grid_start), _lib.ptr(grid_idx),
                                   _lib.stream_ptr()), "mf_icpreg_prepare")
    return dict(out=out, out_cnt=out_cnt, off=off, grid_origin=grid_origin, grid_dim=grid_dim, grid_off=grid_off,
                grid_start=grid_start, grid_idx=grid_idx, cell=cell)


def voxel_down_sample_batch(sets, voxel_size, device=None):
    """open3d's voxel_down_sample of every set: (packed float64 [N, 3], host row offsets, out_cnt [n_sets] int32);
    set b's result is rows off[b] .. off[b] + out_cnt[b] (voxel means in (i, j, k) order, NaN rows dropped)."""
    if not voxel_size > 0:
        raise ValueError("voxel_size must be positive")
    device = _device_of(sets, device=device)
    packed, off = _pack(sets, device)
    p = _prepare(packed, off, float(voxel_size), [False] * (len(off) - 1), device)
    return p["out"], off, p["out_cnt"]


def icp_registration_batch(pcds_depth, pcds_cad, transforms_init=None, iteration=100, voxel_size=0.01, active=None,
                           return_history=False, *, cad_keys=None, iterative=False, device=None):
    """``ICPRegistration(pcd_depth[b], pcd_cad[b], transforms_init[b]).register(iteration, voxel_size)`` for every b
    in one bounds, one prepare and one ICP launch.

    pcds_depth: list of [..., 3] clouds (NaN rows dropped), a crop tensor [B, S, S, 3] or (packed [N, 3], offsets).
    pcds_cad: list of B clouds, or one cloud shared by every object.  cad_keys: optional B hashable keys (e.g.
    class ids); targets are then prepared once per (key, voxel_size) and kept.  transforms_init: [B, 4, 4]
    cad -> cam (None: identity).  active: [B] bool (False: skipped, the pose passes through, n_iter 0).
    iterative: register_iterative's steps (``iteration`` one-update steps, no convergence test).

    Returns device tensors (transform [B, 4, 4] float64 cad -> cam, fitness [B], inlier_rmse [B], n_iter [B] int32)
    and, with ``return_history``, a fifth element (transforms [B, iteration + 1, 4, 4], fitness, inlier_rmse
    [B, iteration + 1]): entry 0 = transforms_init and the result there, entry k = after update k."""
    iteration = int(iteration)
    if iteration < 0:
        raise ValueError("iteration must be >= 0")
    if not voxel_size > 0:
        raise ValueError("voxel_size must be positive")
    voxel_size = float(voxel_size)
    device = _device_of(pcds_depth, pcds_cad, transforms_init, device=device)
    src, src_off = _pack(pcds_depth, device)
    B = len(src_off) - 1
    if isinstance(pcds_cad, (list, tuple)):
        if len(pcds_cad) != B:
            raise ValueError(f"{len(pcds_cad)} CAD clouds for {B} objects")
        cads = list(pcds_cad)
    else:
        cads = [pcds_cad] * B
    if cad_keys is not None:
        keys = [(k, voxel_size, str(device)) for k in cad_keys]
        if len(keys) != B:
            raise ValueError("cad_keys must have one key per object")
    elif isinstance(pcds_cad, (list, tuple)):
        keys = [("obj", b) for b in range(B)]
    else:
        keys = [("shared",)] * B
    # unique targets; the ones not cached are prepared together with the sources (one readback)
    uniq, new = [], []
    for b, k in enumerate(keys):
        if k not in uniq:
            uniq.append(k)
            if cad_keys is None or k not in _CACHE:
                new.append((k, b))
    new_packed, new_off = _pack([cads[b] for _, b in new], device) if new else (None, [0])
    packed = torch.cat([src, new_packed]) if new else src
    off = src_off + [src_off[-1] + o for o in new_off[1:]]
    prep = _prepare(packed, off, voxel_size, [False] * B + [True] * len(new), device)
    targets = {}
    for j, (k, _) in enumerate(new):
        s = B + j
        r0, r1, g0, g1 = off[s], off[s + 1], prep["grid_off"][s], prep["grid_off"][s + 1]
        tg = _Target(prep["out"][r0:r1], prep["out_cnt"][s:s + 1], prep["grid_origin"][s], prep["grid_dim"][s],
                     prep["grid_start"][g0:g1], prep["grid_idx"][r0:r1])
        targets[k] = tg
        if cad_keys is not None:
            _CACHE[k] = tg
            while len(_CACHE) > _CACHE_SIZE:
                _CACHE.popitem(last=False)
    for k in uniq:
        if k not in targets:
            targets[k] = _CACHE[k]
            _CACHE.move_to_end(k)
    # the target pool: one copy of each unique target
    pool = [targets[k] for k in uniq]
    rows, gents = [0], [0]
    for tg in pool:
        rows.append(rows[-1] + tg.pts.shape[0])
        gents.append(gents[-1] + tg.grid_start.shape[0])
    slot = {k: i for i, k in enumerate(uniq)}
    which = [slot[k] for k in keys]
    pad_i = [torch.zeros(1, dtype=torch.int32, device=device)]  # keeps every array non-empty
    tgt = torch.cat([tg.pts for tg in pool] + [torch.zeros((1, 3), dtype=torch.float64, device=device)])
    tgt_cnt_pool = torch.cat([tg.cnt for tg in pool])
    grid_start = torch.cat([tg.grid_start for tg in pool] + pad_i)
    grid_idx = torch.cat([tg.grid_idx for tg in pool] + pad_i)
    grid_origin_pool = torch.stack([tg.grid_origin for tg in pool])
    idx = torch.tensor(which, dtype=torch.int64, device=device)
    tgt_off = torch.tensor([rows[w] for w in which], dtype=torch.int64, device=device)
    grid_off = torch.tensor([gents[w] for w in which], dtype=torch.int64, device=device)
    grid_dim = torch.tensor([pool[w].grid_dim for w in which], dtype=torch.int32, device=device).reshape(B, 3)
    tgt_cnt = tgt_cnt_pool[idx].contiguous()
    grid_origin = grid_origin_pool[idx].contiguous()

    if transforms_init is None:
        init = torch.eye(4, dtype=torch.float64, device=device).repeat(B, 1, 1)
    elif isinstance(transforms_init, (list, tuple)):
        init = torch.stack([torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t)
                            .to(device=device, dtype=torch.float64).reshape(4, 4) for t in transforms_init])
    else:
        init = torch.as_tensor(transforms_init).to(device=device, dtype=torch.float64).reshape(B, 4, 4)
    init = init.contiguous()
    act = None
    if active is not None:
        act = torch.as_tensor(active).to(device=device).reshape(B).to(torch.uint8).contiguous()

    f64 = dict(dtype=torch.float64, device=device)
    transform = torch.empty((B, 4, 4), **f64)
    transformation = torch.empty((B, 4, 4), **f64)
    fitness = torch.empty(B, **f64)
    rmse = torch.empty(B, **f64)
    n_iter = torch.empty(B, dtype=torch.int32, device=device)
    cur = torch.empty((max(src.shape[0], 1), 3), **f64)
    corr = torch.empty(max(src.shape[0], 1), dtype=torch.int32, device=device)
    hist = None
    if return_history:
        hist = (torch.empty((B, iteration + 1, 4, 4), **f64), torch.empty((B, iteration + 1), **f64),
                torch.empty((B, iteration + 1), **f64))
    src_off_d = torch.tensor(src_off, dtype=torch.int64, device=device)
    d = _lib.IcpRegBatch()
    d.src, d.src_off, d.src_cnt = _lib.ptr(prep["out"]), _lib.ptr(src_off_d), _lib.ptr(prep["out_cnt"])
    d.tgt, d.tgt_off, d.tgt_cnt = _lib.ptr(tgt), _lib.ptr(tgt_off), _lib.ptr(tgt_cnt)
    d.grid_off, d.grid_dim, d.grid_origin = _lib.ptr(grid_off), _lib.ptr(grid_dim), _lib.ptr(grid_origin)
    d.grid_start, d.grid_idx = _lib.ptr(grid_start), _lib.ptr(grid_idx)
    d.transform_init, d.active = _lib.ptr(init), _lib.ptr(act)
    d.cur, d.corr = _lib.ptr(cur), _lib.ptr(corr)
    d.transform, d.transformation = _lib.ptr(transform), _lib.ptr(transformation)
    d.fitness, d.inlier_rmse, d.n_iter = _lib.ptr(fitness), _lib.ptr(rmse), _lib.ptr(n_iter)
    if hist is not None:
        d.hist_transform, d.hist_fitness, d.hist_rmse = (_lib.ptr(h) for h in hist)
    d.max_corr_dist = 2.0 * voxel_size
    d.cell = prep["cell"]
    d.n_objects, d.max_iter, d.mode, d.reserved = B, iteration, 1 if iterative else 0, 0
    _lib.check(_lib.lib().mf_icpreg_run(d, _lib.stream_ptr()), "mf_icpreg_run")
    result = (transform, fitness, rmse, n_iter)
    return result + (hist,) if return_history else result


class ICPRegistration:
    """morefusion/contrib/icp_registration.py: source = ``pcd_depth``, target = ``pcd_cad``; ``transform_init`` and
    the results map cad -> camera.  NumPy or device inputs; ``register`` returns a NumPy float64 4 x 4."""

    def __init__(self, pcd_depth, pcd_cad, transform_init=None, *, device=None):
        self._pcd_depth = pcd_depth
        self._pcd_cad = pcd_cad
        if transform_init is None:
            transform_init = np.eye(4)
        self._transform = transform_init
        self._device = _device_of(pcd_depth, pcd_cad, transform_init, device=device)

    def _run(self, iteration, voxel_size, iterative):
        return icp_registration_batch([self._pcd_depth], [self._pcd_cad], [self._init()], iteration, voxel_size,
                                      return_history=iterative, iterative=iterative, device=self._device)

    def _init(self):
        t = self._transform
        return t.detach().to(self._device, torch.float64) if isinstance(t, torch.Tensor) else \
            torch.as_tensor(np.asarray(t, np.float64), device=self._device)

    def register(self, iteration=None, voxel_size=None):
        iteration = 100 if iteration is None else iteration
        voxel_size = 0.01 if voxel_size is None else voxel_size
        transform = self._run(iteration, voxel_size, False)[0]
        return transform[0].cpu().numpy()

    def register_iterative(self, iteration=None, voxel_size=None):
        iteration = 100 if iteration is None else iteration
        voxel_size = 0.01 if voxel_size is None else voxel_size

        yield self._transform

        hist_t, hist_f, hist_r = (h[0].cpu().numpy() for h in self._run(iteration, voxel_size, True)[4])
        for i in range(iteration):
            print(f"[{i:08d}] fitness={hist_f[i + 1]:.2g} inlier_rmse={hist_r[i + 1]:.2g}")
            self._transform = hist_t[i + 1]
            yield self._transform
